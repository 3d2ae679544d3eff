"""What the GPU tests of the YUV frame formats share (test_gpu_yuv.py: NV12 / NV21 / I420; test_gpu_yuv16.py: P010 / I010;
test_gpu_yuv_any.py: the other 8-bit samplings): the fixtures, the helpers and the bodies of the tests that every family runs.
One claim, everywhere: the result for YUV `frames` is bit-identical to passing `bgr` - the same frames converted by
tests/yuv_model.py - to the B, G, R entry point of the same name ON THE DEVICE.  A body takes the family's (frames, bgr, ...); the
shapes, rectangles and pinned numbers are the test files'."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import yuv_model as ym
from frames_ref import MAX_DET
from oracle import yfv2_oracle as oracle

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert os.path.exists(yolo_fastestv2_amd.LIB_PATH), "libyfv2.so not built"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def new_engine(yfv2, dev, cfg, weights, max_batch):
    eng = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=max_batch, plan={})
    eng.load_state_dict(weights)
    return eng


@pytest.fixture(scope="module")
def engine(yfv2, dev, cfg, coco_weights):
    return new_engine(yfv2, dev, cfg, coco_weights, 16)


def _out(eng, B):
    dets, idx, cnt = eng.new_det_buffers(B)
    dets.fill_(SENTINEL)
    idx.fill_(-7)
    cnt.fill_(-9)
    return dets, idx, cnt


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _to(dev, planes):
    """planes -> device tensors; uint16 words as int16 (the same bits)"""
    return tuple(torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(dev) for p in planes)


def _bgr(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what):
    """bit for bit: dtype, shape, then every value's bit pattern (so -0.0 is not 0.0, and a NaN equals only itself)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    view = {4: np.uint32, 2: np.uint16, 1: np.uint8}[got.element_size()]
    g, w = got.contiguous().cpu().numpy(), want.contiguous().cpu().numpy()
    bad = np.argwhere(g.view(view) != w.view(view))
    assert bad.size == 0, "%s: %d values differ, first at %s: %r vs %r" % (what, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _picture(images_u8, k, h, w, seed):
    hwc = np.ascontiguousarray(images_u8[k % len(images_u8)].transpose(1, 2, 0))
    rng = np.random.default_rng(seed)
    f = oracle.resize_linear_u8(hwc, w, h)
    return np.clip(f.astype(np.int16) + rng.integers(-3, 4, f.shape), 0, 255).astype(np.uint8)


def _frame(yfv2, dev, planes, fmt, colour, *rect):
    return yfv2.YuvFrame(_to(dev, planes), ym.NAMES[fmt], colour, *rect)


def _pair(yfv2, dev, planes, fmt, colour, x0, y0, w, h):
    """a frame of `planes` on the device and the model's conversion of it"""
    return _frame(yfv2, dev, planes, fmt, colour, x0, y0, w, h), _bgr(dev, ym.yuv_to_bgr(planes, fmt, colour, x0, y0, w, h))


def _plane_set(dev, planes, pitches, residues, poison=None):
    """the planes (bytes or words) in ONE device tensor that ends with the last plane's last sample: plane k at a sample offset that
    is residues[k][0] modulo residues[k][1], allocated exactly ((rows - 1) * pitch + row samples), `poison` in the padding and
    between the planes -> (the tensor, its host copy, the planes as views of it, their offsets)"""
    dtype = planes[0].dtype
    poison = (ym.POISON if dtype.itemsize == 1 else ym.POISON16) if poison is None else poison
    flats = [ym.pad_plane(p, q, poison) for p, q in zip(planes, pitches)]
    offs, o = [], 0
    for f, (r, m) in zip(flats, residues):
        o += (r - o) % m
        offs.append(o)
        o += len(f)
    host = np.full(o, poison, dtype)
    for f, q in zip(flats, offs):
        host[q:q + len(f)] = f
    flat = torch.from_numpy(host.view(np.int16) if dtype == np.uint16 else host).to(dev)
    assert flat.data_ptr() % 4 == 0 and all(q % m == r for q, (r, m) in zip(offs, residues)) and offs[-1] + len(flats[-1]) == flat.numel()
    views = tuple(torch.as_strided(flat, p.shape, (q, 1), off) for p, q, off in zip(planes, pitches, offs))
    for v, p in zip(views, planes):
        assert np.array_equal(v.cpu().numpy().view(dtype), p)
    return flat, host, views, offs


def _hand_rows(frames, rows):
    """hand-made detections: rows(w, h) -> the (x1, y1, x2, y2, conf, cls) rows of a w x h frame -> (dets (B, 8, 6), count)"""
    dets = np.full((len(frames), 8, 6), -3.0, np.float32)
    count = np.zeros(len(frames), np.int32)
    for b, f in enumerate(frames):
        mine = rows(f.width, f.height)
        dets[b, :len(mine)], count[b] = mine, len(mine)
    return dets, count


def _check_plan(got, want, least, parities=(), R=8):
    """the crop plans are equal; at least `least` crops; per entry of `parities` - a set of frames, None: all of them - rectangles
    at odd and even x and y"""
    total = int(want[3][-1])
    assert total >= least
    for group in parities:
        mine = [r for r, s in zip(want[2][:total].tolist(), want[1][:total].tolist()) if group is None or s // R in group]
        assert {r[0] & 1 for r in mine} == {0, 1} and {r[1] & 1 for r in mine} == {0, 1}, mine
    for g, w_, name in zip(got[1:], want[1:], ("crop_src", "crop_rect", "crop_offset", "crop_skipped")):
        n = total if name in ("crop_src", "crop_rect") else len(w_)          # (slots beyond the total are not written)
        assert torch.equal(g[:n], w_[:n]), name
    return total


# ---- the bodies ----------------------------------------------------------------------------------------------------------------
def check_detect_frames(engine, frames, bgr, conf):
    B = len(frames)
    got = engine.detect_frames_yuv(frames, conf, 0.4, out=_out(engine, B))
    want = engine.detect_frames(bgr, conf, 0.4, out=_out(engine, B))
    assert torch.equal(got[2], want[2]), (got[2].tolist(), want[2].tolist())
    assert torch.equal(got[1], want[1])
    _same(got[0], want[0], "dets at conf %g" % conf)
    assert int(want[2].sum()) > 0, want[2].tolist()
    return want


def check_detect_tiled(yfv2, engine, frames, bgr, planned_by_the_call=False):
    """F = 2 frames of 500 x 420; 352 x 352 tiles 75 pixels apart, so a column of tiles starts at x = 75 and a row at y = 68: odd
    origins read in place"""
    tiles = [t for f in range(2) for t in yfv2.plan_tiles(420, 500, tile=(352, 352), overlap=(277, 277), frame=f)]
    assert len(tiles) <= engine.max_batch and any(t[1] % 2 == 1 for t in tiles) and any(t[1] % 2 == 0 and t[1] > 0 for t in tiles)

    def buffers():
        d, s, c = engine.new_tiled_buffers(2)
        d.fill_(SENTINEL)
        s.fill_(-7)
        c.fill_(-9)
        return d, s, c

    got = engine.detect_tiled_yuv(frames, tiles=tiles, conf_thres=0.3, iou_thres=0.4, out=buffers())
    want = engine.detect_tiled(bgr, tiles=tiles, conf_thres=0.3, iou_thres=0.4, out=buffers())
    assert torch.equal(got[2], want[2]) and torch.equal(got[1], want[1]), (got[2].tolist(), want[2].tolist())
    _same(got[0], want[0], "tiled dets")
    assert int(want[2].sum()) > 0
    if planned_by_the_call:      # the plan made by the call itself (tiles=None) is the B, G, R call's plan
        got = engine.detect_tiled_yuv(frames, conf_thres=0.3, iou_thres=0.4, overlap=(277, 277), out=buffers())
        assert torch.equal(got[2], want[2]) and torch.equal(got[1], want[1])
        _same(got[0], want[0], "tiled dets, planned by the call")


def check_pipeline(yfv2, dev, cfg, weights, engine, batches, max_batch):
    """batches: (frames, bgr) each - bgr None: the reference is engine.detect_frames_yuv.  Two submits in flight, then the rest: the
    third reuses the first slot."""
    pipe = yfv2.DetectPipeline(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=max_batch, depth=2, plan={})
    pipe.load_state_dict(weights)
    tickets = [pipe.submit_frames_yuv(fr, 0.3, 0.4) for fr, _ in batches[:2]]
    results = [tuple(t.clone() for t in pipe.result(t)) for t in tickets]
    torch.cuda.synchronize()      # the copies are complete before a further submit reuses the first slot
    for fr, _ in batches[2:]:
        results.append(tuple(t.clone() for t in pipe.result(pipe.submit_frames_yuv(fr, 0.3, 0.4))))
    pipe.synchronize()
    total = 0
    for (d, i, c), (fr, ref) in zip(results, batches):
        rd, ri, rc = engine.detect_frames_yuv(fr, 0.3, 0.4) if ref is None else engine.detect_frames(ref, 0.3, 0.4)
        assert tuple(d.shape) == (len(fr), MAX_DET, 6) and torch.equal(c, rc)
        for b in range(len(fr)):
            k = int(c[b])
            total += k
            assert torch.equal(i[b, :k], ri[b, :k])
            _same(d[b, :k], rd[b, :k], "pipeline frame %d" % b)
    assert total > 0


def check_train_batch(yfv2, dev, frames, bgr, alpha, beta):
    B = len(frames)
    eng = yfv2.Engine(dev, 64, 96, max_batch=B, plan={})
    for a, b in ((alpha, beta), (None, None)):
        got = eng.train_batch_frames_yuv(frames, a, b)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, 3, 64, 96)
        _same(got, eng.train_batch_frames(bgr, a, b), "training batch")
    from yolo_fastestv2_amd import datasets
    labels = [np.zeros((0, 6), np.float32)] * B
    imgs, _ = datasets.TrainBatcher(eng)(frames, labels)
    _same(imgs, eng.train_batch_frames(bgr), "TrainBatcher")


def check_crop_detections(yfv2, dev, frames, bgr, rows, pad, least, parities):
    """the crop plan folds each rectangle into the plane pointers ON THE DEVICE, whatever the samples are"""
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(frames), plan={})
    dets, count = _hand_rows(frames, rows)
    d, c = torch.from_numpy(dets).to(dev), torch.from_numpy(count).to(dev)
    got = eng.crop_detections_yuv(frames, d, c, (32, 32), pad=pad)
    want = eng.crop_detections(bgr, d, c, (32, 32), pad=pad)
    torch.cuda.synchronize()
    total = _check_plan(got, want, least, parities)
    _same(got[0][:total], want[0][:total], "crops")


def check_crop_tensors(yfv2, dev, frames, bgr, rows, pad, least, parities, dtype, letterbox):
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(frames), plan={})
    dets, count = _hand_rows(frames, rows)
    d, c = torch.from_numpy(dets).to(dev), torch.from_numpy(count).to(dev)
    kw = dict(pad=pad, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), rgb=True, letterbox=letterbox, fill=(114, 7, 201), dtype=dtype)
    got = eng.crop_tensors_yuv(frames, d, c, (32, 32), **kw)
    want = eng.crop_tensors(bgr, d, c, (32, 32), **kw)
    torch.cuda.synchronize()
    total = _check_plan(got, want, least, parities)
    assert got[0].dtype == dtype
    _same(got[0][:total], want[0][:total], "tensors")


def check_widest_frame_and_limit(yfv2, dev, engine, rng, fmts, limit, wide, by_oracle=False):
    """one frame of `limit` x 2 pixels per format of fmts (bt709_full) resizes like its conversion - by_oracle: against the oracle's
    resize, where the frame is wider than the B, G, R entry point admits (test_gpu_frames pins that entry point to the oracle) - and
    each frame of `wide` (limit + 1 pixels) behind it is refused with the limit in the message, nothing launched
    -> (the engine of the resize, the frames, the two untouched outputs)"""
    from yolo_fastestv2_amd import _lib
    eng = yfv2.Engine(dev, 352, 352, max_batch=max(len(fmts), 2), plan={})
    frames, bgr = [], []
    for fmt in fmts:
        planes = ym.random_planes(rng, 2, limit, fmt)
        frames.append(_frame(yfv2, dev, planes, fmt, ym.BT709_FULL, 0, 0, limit, 2))
        bgr.append(ym.yuv_to_bgr(planes, fmt, ym.BT709_FULL, 0, 0, limit, 2))
    got = eng.resize_frames_yuv(frames)
    want = [_bgr(dev, oracle.resize_linear_u8(a, 352, 352)) for a in bgr] if by_oracle else eng.resize_frames([_bgr(dev, a) for a in bgr])
    for b, fmt in enumerate(fmts):
        _same(got[b], want[b], "the widest %s frame" % ym.NAMES[fmt])
    dst = torch.full((2, 352, 352, 3), 77, dtype=torch.uint8, device=dev)
    out = _out(engine, 2)
    torch.cuda.synchronize()
    for bad in wide:
        for call in (lambda: eng.resize_frames_yuv([frames[0], bad], out=dst), lambda: engine.detect_frames_yuv([frames[0], bad], 0.3, 0.4, out=out)):
            with pytest.raises(_lib.Yfv2Error) as e:
                call()
            assert e.value.code == _lib.ERR_ARG and "frame 1" in str(e.value) and "wider than %d" % limit in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((dst == 77).all()) and bool((out[0] == SENTINEL).all()) and bool((out[2] == -9).all()), "a failed call wrote its output"
    return eng, frames, dst, out
