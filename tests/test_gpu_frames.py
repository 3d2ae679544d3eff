"""GPU tests of the ragged-batch entry points: Engine.resize_frames / Engine.detect_frames / DetectPipeline.submit_frames
(include/yfv2.h yfv2_resize_frames_u8, yfv2_detect_frames_u8).  Run with ``-m gpu`` on an MI355X.

The claims: frame b of a mixed batch resizes bit-identically to resizing that frame alone (Engine.resize, and the oracle's
restatement of cv2.resize INTER_LINEAR); detect_frames equals the composition resize -> detect -> the frame-coordinate
scaling of test.py:58-68 (tests/frames_ref.py) bit for bit, on every plan; bad arguments fail before anything is launched.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from frames_ref import MAX_DET, to_frame_coords
from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0    # output buffers are pre-filled with it: rows beyond count must come back untouched


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert os.path.exists(yolo_fastestv2_amd.LIB_PATH), "libyfv2.so not built"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _engine(yfv2, dev, cfg, weights, max_batch=1, plan=None):
    eng = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=max_batch,
                      plan={} if plan is None else plan)
    eng.load_state_dict(weights)
    return eng


@pytest.fixture(scope="module")
def engine(yfv2, dev, cfg, coco_weights):
    return _engine(yfv2, dev, cfg, coco_weights, max_batch=8)


def _out(eng, B):
    dets, idx, cnt = eng.new_det_buffers(B)
    dets.fill_(SENTINEL)
    idx.fill_(-7)
    cnt.fill_(-9)
    return dets, idx, cnt


def _picture(images_u8, k, h, w, seed):
    """a plausible (h, w, 3) frame: reference image k resized by the oracle, plus a little seeded noise"""
    hwc = np.ascontiguousarray(images_u8[k % len(images_u8)].transpose(1, 2, 0))
    rng = np.random.default_rng(seed)
    f = oracle.resize_linear_u8(hwc, w, h)
    return np.clip(f.astype(np.int16) + rng.integers(-3, 4, f.shape), 0, 255).astype(np.uint8)


def _compose(eng, frames, conf, iou, groups=None):
    """the composition detect_frames replaces: resize (one call per group of equally sized frames, or per frame), detect,
    scale to frame coordinates in numpy float64 -> host (dets, idx, cnt) with sentinel padding"""
    B = len(frames)
    sizes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
    if groups is None:
        groups = [[i] for i in range(B)]
    dets = np.full((B, MAX_DET, 6), SENTINEL, np.float32)
    idx = np.full((B, MAX_DET), -7, np.int32)
    cnt = np.zeros(B, np.int32)
    for g in groups:
        x = eng.resize(torch.stack([frames[i].contiguous() for i in g]))
        d, i, c = eng.detect(x, conf, iou, out=_out(eng, len(g)))
        d, i, c = d.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()
        for j, b in enumerate(g):
            dets[b], idx[b], cnt[b] = d[j], i[j], c[j]
    return to_frame_coords(dets, cnt, sizes, eng.width, eng.height), idx, cnt


def _assert_same(got, want, what):
    gd, gi, gc = (t.cpu().numpy() for t in got)
    wd, wi, wc = want
    assert np.array_equal(gc, wc), "%s: counts %s vs %s" % (what, gc.tolist(), wc.tolist())
    assert np.array_equal(gi, wi), "%s: survivor indices differ" % what
    bad = np.argwhere(gd.view(np.uint32) != wd.view(np.uint32))
    assert bad.size == 0, "%s: %d dets words differ, first at %s: %r vs %r" % (what, len(bad), bad[0].tolist(), gd[tuple(bad[0])], wd[tuple(bad[0])])


def _by_size(frames):
    groups = {}
    for i, f in enumerate(frames):
        groups.setdefault((int(f.shape[0]), int(f.shape[1])), []).append(i)
    return list(groups.values())


# ---- 1. resize ---------------------------------------------------------------------------------------------------------
def test_resize_frames_is_per_frame_resize(yfv2, dev):
    """Mixed sizes, a one-pixel frame, a 20 000-pixel row, frames carved from one flat buffer at byte offsets 1, 2, 3 (one of
    them ending on the buffer's last byte) and crop views (pitch > 3w, odd start, one in the bottom-right corner of its parent):
    each output equals the oracle's resize of that frame and Engine.resize of that frame alone, byte for byte."""
    rng = np.random.default_rng(11)
    shapes = [(480, 640), (1080, 1920), (1, 1), (2, 3), (353, 351), (352, 352), (704, 704), (120, 160), (2, 20000)]
    host = [(rng.random(s + (3,)) * 255).astype(np.uint8) for s in shapes]
    frames = [torch.from_numpy(h).to(dev) for h in host]
    # carved from one flat buffer at byte offsets 1, 2, 3; the last one ends on the buffer's last byte
    carve = [(37, 45), (5, 7), (61, 33)]
    sizes = [h * w * 3 for h, w in carve]
    offs, o = [], 0
    for k, n in enumerate(sizes):
        o += (k + 1 - o) % 4                  # the next offset that is k + 1 (mod 4)
        offs.append(o)
        o += n
    flat = torch.zeros(o, dtype=torch.uint8, device=dev)
    for (h, w), o in zip(carve, offs):
        a = (rng.random((h, w, 3)) * 255).astype(np.uint8)
        flat[o:o + h * w * 3] = torch.from_numpy(a.reshape(-1)).to(dev)
        host.append(a)
        frames.append(flat[o:o + h * w * 3].view(h, w, 3))
    assert [f.data_ptr() % 4 for f in frames[-3:]] == [1, 2, 3]
    # crop views of a larger frame: pitch 3 * 101 > 3w, odd start; and the bottom-right corner (the extent ends at the allocation's end)
    parent = torch.from_numpy((rng.random((90, 101, 3)) * 255).astype(np.uint8)).to(dev)
    for crop in (parent[3:50, 7:36], parent[-41:, -29:], parent[10:11, 1:2]):
        assert crop.stride(0) == 303 and crop.stride(1) == 3
        frames.append(crop)
        host.append(crop.cpu().numpy())
    ptrs = [f.data_ptr() for f in frames]

    eng = yfv2.Engine(dev, 352, 352, max_batch=1, plan={})
    got = eng.resize_frames(frames)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(frames), 352, 352, 3)
    assert eng.max_batch >= len(frames)
    assert [f.data_ptr() for f in frames] == ptrs
    got = got.cpu().numpy()
    for b, (f, h) in enumerate(zip(frames, host)):
        want = oracle.resize_linear_u8(h, 352, 352)
        assert np.array_equal(got[b], want), "frame %d %s differs from the oracle" % (b, h.shape)
        alone = eng.resize(f.contiguous()[None]).cpu().numpy()[0]
        assert np.array_equal(got[b], alone), "frame %d %s differs from Engine.resize" % (b, h.shape)
    # out= and a list of one
    out = torch.empty((1, 352, 352, 3), dtype=torch.uint8, device=dev)
    assert eng.resize_frames((frames[0],), out=out) is out
    assert np.array_equal(out.cpu().numpy()[0], got[0])


# ---- 2. detect ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conf,iou", [(0.3, 0.4), (0.01, 0.4)])
def test_detect_frames_is_resize_detect_scale(yfv2, dev, cfg, engine, images_u8, conf, iou):
    sizes = [(480, 640), (1080, 1920), (720, 1280), (352, 352), (300, 500), (200, 260), (704, 704), (353, 351)]
    frames = [torch.from_numpy(_picture(images_u8, k, h, w, 100 + k)).to(dev) for k, (h, w) in enumerate(sizes)]
    frames.append(frames[2][100:600, 200:900])          # a crop view of the 1280x720 frame
    got = engine.detect_frames(frames, conf, iou, out=_out(engine, len(frames)))
    want = _compose(engine, frames, conf, iou)
    _assert_same(got, want, "detect_frames conf %g" % conf)
    assert (want[2] > 0).sum() >= 4, want[2]
    # frame coordinates: boxes of the frames wider than the network reach beyond its 352 columns
    wd, wc = want[0], want[2]
    assert max(float(wd[b, :wc[b], 2].max()) for b in range(len(frames)) if wc[b] > 0 and frames[b].shape[1] > 600) > 352.0


# ---- 3. all frames at the network size: exact copy, scale 1 ---------------------------------------------------------------
def test_detect_frames_at_network_size_equals_detect(yfv2, dev, cfg, engine, images_u8):
    x = torch.from_numpy(np.ascontiguousarray(images_u8.transpose(0, 2, 3, 1))).to(dev)
    frames = list(x.unbind(0))
    got = engine.detect_frames(frames, 0.3, 0.4, out=_out(engine, len(frames)))
    ref = engine.detect(x, 0.3, 0.4, out=_out(engine, len(frames)))
    for g, r, what in zip(got, ref, ("dets", "idx", "count")):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), r.cpu().numpy().view(np.uint32)), what
    assert int(got[2].sum()) > 0


# ---- 4. a large shuffled batch of many sizes --------------------------------------------------------------------------
def _many_frames(dev, images_u8, sizes, n, seed):
    base = [torch.from_numpy(_picture(images_u8, k, h, w, seed + k)).to(dev) for k, (h, w) in enumerate(sizes)]
    order = np.random.default_rng(seed).permutation(np.arange(n) % len(sizes))
    gen = torch.Generator(device=dev).manual_seed(seed)
    frames = []
    for k in order:
        noise = torch.randint(-2, 3, base[k].shape, generator=gen, device=dev, dtype=torch.int16)
        frames.append((base[k].to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8))
    return frames


def test_detect_frames_256_shuffled_sizes_grows_the_batch(yfv2, dev, cfg, coco_weights, images_u8):
    sizes = [(1080, 1920), (720, 1280), (480, 640), (352, 352), (240, 320), (600, 800), (100, 150), (288, 512), (704, 704)]
    frames = _many_frames(dev, images_u8, sizes, 256, 7)
    eng = _engine(yfv2, dev, cfg, coco_weights, max_batch=1)
    got = eng.detect_frames(frames, 0.3, 0.4, out=_out(eng, 256))
    assert eng.max_batch >= 256
    want = _compose(eng, frames, 0.3, 0.4, groups=_by_size(frames))
    _assert_same(got, want, "256 shuffled frames")
    assert (want[2] > 0).sum() > 64


# ---- 5. other plans ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,n", [({"lanes": 2}, 80), ({"fp32_matrix": 1}, 12)], ids=["lanes2", "fp32_matrix"])
def test_detect_frames_on_other_plans(yfv2, dev, cfg, coco_weights, images_u8, plan, n):
    sizes = [(480, 640), (720, 1280), (352, 352), (200, 260)]
    frames = _many_frames(dev, images_u8, sizes, n, 21)
    eng = _engine(yfv2, dev, cfg, coco_weights, max_batch=n, plan=plan)
    got = eng.detect_frames(frames, 0.3, 0.4, out=_out(eng, n))
    want = _compose(eng, frames, 0.3, 0.4, groups=_by_size(frames) if n > 16 else None)
    _assert_same(got, want, str(plan))
    assert (want[2] > 0).sum() >= n // 4


# ---- 6. argument errors --------------------------------------------------------------------------------------------------
def test_frame_argument_errors_launch_nothing(yfv2, dev, cfg, coco_weights, images_u8):
    from yolo_fastestv2_amd import _lib
    eng = _engine(yfv2, dev, cfg, coco_weights, max_batch=4)
    good = torch.from_numpy(_picture(images_u8, 0, 480, 640, 3)).to(dev)
    for bad in (good.float(), good.cpu(), good[:, :, 0], good[..., :2], torch.zeros((4, 4, 4), dtype=torch.uint8, device=dev), good[None]):
        with pytest.raises(ValueError):
            eng.resize_frames([good, bad])
        with pytest.raises(ValueError):
            eng.detect_frames([bad, good], 0.3, 0.4)
    for bad in ([], (), good):
        with pytest.raises(ValueError):
            eng.resize_frames(bad)
    out = _out(eng, 2)
    dst = torch.full((3, 352, 352, 3), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    # the native checks, through the Python surface
    for bad, msg in ((good[:0], "height and width"), (good[:, :0], "height and width"),
                     (torch.zeros((2, 27200, 3), dtype=torch.uint8, device=dev), "wider than 27128")):
        for call in (lambda: eng.resize_frames([good, bad], out=dst[:2]), lambda: eng.detect_frames([good, bad], 0.3, 0.4, out=out)):
            with pytest.raises(_lib.Yfv2Error) as e:
                call()
            assert e.value.code == _lib.ERR_ARG and msg in str(e.value), str(e.value)
    # ... and through the C ABI directly: what the Python layer cannot produce
    L = _lib.lib()
    h = eng._h
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def table(*fs):
        arr = (_lib.Frame * len(fs))()
        for i, (p, hh, ww, pitch) in enumerate(fs):
            arr[i].data, arr[i].height, arr[i].width, arr[i].row_pitch = p, hh, ww, pitch
        return arr

    g = (good.data_ptr(), 480, 640, 1920)
    d0 = dst.data_ptr()
    cases = [
        (table(g, (good.data_ptr(), 480, 640, 1919)), 2, d0, "row_pitch 1919 < 3 * width"),
        (table(g, (None, 480, 640, 1920)), 2, d0, "null data"),
        (table(g), 0, d0, "B < 1"),
        (table(g), -3, d0, "B < 1"),
        (None, 1, d0, "null pointer"),
        (table(g), 1, d0 + 2, "4-byte aligned"),
        (table(g), 1, None, "null pointer"),
        (table((good.data_ptr(), 0, 640, 1920)), 1, d0, "height and width"),
        (table((good.data_ptr(), 480, -1, 1920)), 1, d0, "height and width"),
    ]
    for arr, B, dptr, msg in cases:
        rc = L.yfv2_resize_frames_u8(h, arr, B, C.c_void_p(dptr) if dptr else None, st)
        assert rc == _lib.ERR_ARG and msg in _lib.last_error(h), (msg, rc, _lib.last_error(h))
        if dptr == d0:
            rc = L.yfv2_detect_frames_u8(h, arr, B, 0.3, 0.4, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), st)
            want_rc = _lib.ERR_BATCH if B < 1 else _lib.ERR_ARG      # check_call reports B outside [1, max_batch] as a batch error
            assert rc == want_rc, (msg, rc, _lib.last_error(h))
    five = table(*([g] * 5))
    assert L.yfv2_resize_frames_u8(h, five, 5, C.c_void_p(d0), st) == _lib.ERR_BATCH
    assert L.yfv2_detect_frames_u8(h, five, 5, 0.3, 0.4, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), st) == _lib.ERR_BATCH
    assert L.yfv2_detect_frames_u8(h, table(g), 1, 0.3, 0.4, None, _ptr(out[1]), _ptr(out[2]), st) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == 77).all()), "a failed call wrote its output"
    assert bool((out[0] == SENTINEL).all()) and bool((out[2] == -9).all()), "a failed call wrote its output"
    # the engine is intact
    frames = [good, torch.from_numpy(_picture(images_u8, 1, 720, 1280, 4)).to(dev)]
    got = eng.detect_frames(frames, 0.3, 0.4, out=_out(eng, 2))
    _assert_same(got, _compose(eng, frames, 0.3, 0.4), "after the errors")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ---- 7. the pipeline -----------------------------------------------------------------------------------------------------
def test_pipeline_submit_frames(yfv2, dev, cfg, coco_weights, images_u8):
    pipe = yfv2.DetectPipeline(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=6,
                               depth=3, plan={})
    pipe.load_state_dict(coco_weights)
    ref = _engine(yfv2, dev, cfg, coco_weights, max_batch=6)
    batches = [_many_frames(dev, images_u8, [(480, 640), (720, 1280), (352, 352)], n, 40 + n) for n in (3, 6, 5)]
    tickets = [pipe.submit_frames(fr, 0.3, 0.4) for fr in batches]
    for t, fr in zip(tickets, batches):
        d, i, c = pipe.result(t)
        rd, ri, rc = ref.detect_frames(fr, 0.3, 0.4)
        n = len(fr)
        assert tuple(d.shape) == (n, MAX_DET, 6)
        assert torch.equal(c, rc)
        for b in range(n):
            k = int(c[b])
            assert torch.equal(i[b, :k], ri[b, :k])
            assert np.array_equal(d[b, :k].cpu().numpy().view(np.uint32), rd[b, :k].cpu().numpy().view(np.uint32))
    assert sum(int(pipe.result(t)[2].sum()) for t in tickets) > 0
    pipe.synchronize()
