"""GPU tests of the 10-bit YUV front door: P010 and I010 frames through every *_yuv entry point (include/yfv2.h YFV2_YUV_P010 /
YFV2_YUV_I010).  Run with ``-m gpu`` on an MI355X.

One claim, everywhere: the result for a 10-bit frame is bit-identical to converting that frame to B, G, R with the integer rule of
include/yfv2.h (tests/yuv16_model.py states it in numpy) and passing it to the B, G, R entry point of the same name ON THE DEVICE.
Every comparison is exact.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rows_model
import yuv16_model as m16
from frames_ref import MAX_DET
from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
NAMES = {m16.P010: "p010", m16.I010: "i010"}


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert os.path.exists(yolo_fastestv2_amd.LIB_PATH), "libyfv2.so not built"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engine(yfv2, dev, cfg, coco_weights):
    eng = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=16, plan={})
    eng.load_state_dict(coco_weights)
    return eng


def _out(eng, B):
    dets, idx, cnt = eng.new_det_buffers(B)
    dets.fill_(SENTINEL)
    idx.fill_(-7)
    cnt.fill_(-9)
    return dets, idx, cnt


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _to(dev, planes):
    """planes of uint16 words -> int16 device tensors (the same bits)"""
    return tuple(torch.from_numpy(np.ascontiguousarray(p).view(np.int16)).to(dev) for p in planes)


def _bgr(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_words(got, want, what):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    view = {4: np.uint32, 2: np.uint16, 1: np.uint8}
    bad = np.argwhere(g.view(view[g.dtype.itemsize]) != w.view(view[w.dtype.itemsize]))
    assert bad.size == 0, "%s: %d words differ, first at %s: %r vs %r" % (what, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- 1. resize equals convert-then-resize ------------------------------------------------------------------------------------
SIZES_WH = [(1, 1), (2, 3), (3, 2), (17, 31), (352, 352), (353, 351), (640, 360), (1279, 721)]


@pytest.mark.parametrize("fmt", m16.FORMATS, ids=["p010", "i010"])
def test_resize_yuv_is_convert_then_resize(yfv2, dev, fmt):
    """One ragged batch: 1 x 1 up to 1279 x 721, 352 x 352 being the identity resize - the pure conversion - each with the colour
    standard k % 4 (all four occur), random values over all of 0..1023 (the clamps fire) and random junk in the ignored bits."""
    rng = np.random.default_rng(100 + fmt)
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(SIZES_WH), plan={})
    frames, bgr = [], []
    for k, (w, h) in enumerate(SIZES_WH):
        planes = m16.random_planes(rng, h, w, fmt)
        frames.append(yfv2.YuvFrame(_to(dev, planes), NAMES[fmt], k % 4))
        bgr.append(_bgr(dev, m16.yuv_to_bgr(planes, fmt, k % 4, 0, 0, w, h)))
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(SIZES_WH), 352, 352, 3)
    for b, (w, h) in enumerate(SIZES_WH):
        _same_words(got[b], want[b], "frame %d (%d x %d, colour %d)" % (b, w, h, b % 4))
    k = SIZES_WH.index((352, 352))
    assert torch.equal(got[k], bgr[k]), "the identity resize is the pure conversion"
    assert bool((got == 0).any()) and bool((got == 255).any())


# ---- 2. crops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", m16.FORMATS, ids=["p010", "i010"])
def test_crops_of_padded_planes_read_in_place(yfv2, dev, fmt):
    """One 97 x 131 plane set in ONE int16 tensor that ends with the last plane's last sample: every plane at a byte offset that is
    2 mod 4, allocated exactly ((rows - 1) * pitch + width words), odd pitches in words (so rows alternate between misalignment 2
    and 0), the padding between rows poison words.  Frames: every (x0, y0) parity, inside the planes and ending on their last sample."""
    rng = np.random.default_rng(200 + fmt)
    rows, cols = 97, 131
    planes = m16.random_planes(rng, rows, cols, fmt)
    pitches = [137] + [planes[1].shape[1] + 5] * (len(planes) - 1)             # words
    flats = [m16.pad_plane(p, q) for p, q in zip(planes, pitches)]
    offs, o = [], 0
    for f in flats:
        o += 1 - o % 2                                                         # an odd word offset
        offs.append(o)
        o += len(f)
    host = np.full(o, m16.POISON, np.uint16)
    for f, q in zip(flats, offs):
        host[q:q + len(f)] = f
    flat = torch.from_numpy(host.view(np.int16)).to(dev)
    assert flat.data_ptr() % 4 == 0 and all(2 * q % 4 == 2 for q in offs) and offs[-1] + len(flats[-1]) == flat.numel()
    views = tuple(torch.as_strided(flat, p.shape, (q, 1), off) for p, q, off in zip(planes, pitches, offs))
    for v, p in zip(views, planes):
        assert np.array_equal(v.cpu().numpy().view(np.uint16), p)
    rects = []
    for x0, y0 in ((0, 0), (1, 0), (0, 1), (1, 1)):
        rects.append((10 + x0, 20 + y0, 50 + x0, 40 + y0))            # inside: poison on both sides of every row
        rects.append((cols - 3 - x0, rows - 4 - y0, 3 + x0, 4 + y0))  # the bottom-right corner: ends at the planes' last sample
    rects += [(1, 1, cols - 1, rows - 1), (cols - 1, rows - 1, 1, 1), (0, 0, 1, 1), (cols - 2, 0, 2, rows), (0, rows - 1, cols, 1)]
    assert {(x0 & 1, y0 & 1) for x0, y0, _w, _h in rects} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert any(x0 + w == cols and y0 + h == rows for x0, y0, w, h in rects)
    frames = [yfv2.YuvFrame(views, NAMES[fmt], k % 4, x0, y0, w, h) for k, (x0, y0, w, h) in enumerate(rects)]
    bgr = [_bgr(dev, m16.yuv_to_bgr(planes, fmt, k % 4, x0, y0, w, h)) for k, (x0, y0, w, h) in enumerate(rects)]
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(rects), plan={})
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    for b, r in enumerate(rects):
        _same_words(got[b], want[b], "crop %d %s" % (b, r))
    # the same planes as uint8 tensors of the bytes (pitch = stride(0)), and a frame made with crop(): the same descriptors
    bytes_ = flat.view(torch.uint8)
    bviews = tuple(torch.as_strided(bytes_, (p.shape[0], 2 * p.shape[1]), (2 * q, 1), 2 * off) for p, q, off in zip(planes, pitches, offs))
    again = eng.resize_frames_yuv([yfv2.YuvFrame(bviews, NAMES[fmt], 1, 0, 0, cols, rows).crop(*rects[3]), yfv2.YuvFrame(views, NAMES[fmt], 1).crop(*rects[3])])
    ref = eng.resize_frames([_bgr(dev, m16.yuv_to_bgr(planes, fmt, 1, *rects[3]))])[0]
    _same_words(again[0], ref, "byte planes")
    _same_words(again[1], ref, "crop()")
    assert np.array_equal(flat.cpu().numpy().view(np.uint16), host)


# ---- 3. the widest frame, and one pixel more -----------------------------------------------------------------------------------
def test_widest_frame_and_the_limit(yfv2, dev, engine):
    from yolo_fastestv2_amd import _lib
    limit = m16.max_width(rows_model.U8, 352)
    assert limit == yfv2.yuv.max_width(352, bits=10) == 20343 <= rows_model.max_width(rows_model.U8, False, 352)
    rng = np.random.default_rng(300)
    eng = yfv2.Engine(dev, 352, 352, max_batch=2, plan={})
    frames, bgr = [], []
    for fmt in m16.FORMATS:
        planes = m16.random_planes(rng, 2, limit, fmt)
        frames.append(yfv2.YuvFrame(_to(dev, planes), NAMES[fmt], m16.BT709_FULL))
        bgr.append(_bgr(dev, m16.yuv_to_bgr(planes, fmt, m16.BT709_FULL, 0, 0, limit, 2)))
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    for b in range(2):
        _same_words(got[b], want[b], "the widest %s frame" % NAMES[m16.FORMATS[b]])
    # limit + 1: refused with a message, nothing launched
    wide = yfv2.YuvFrame((torch.zeros((2, limit + 1), dtype=torch.int16, device=dev), torch.zeros((1, limit + 2), dtype=torch.int16, device=dev)), "p010")
    dst = torch.full((2, 352, 352, 3), 77, dtype=torch.uint8, device=dev)
    out = _out(engine, 2)
    torch.cuda.synchronize()
    for call in (lambda: eng.resize_frames_yuv([frames[0], wide], out=dst), lambda: engine.detect_frames_yuv([frames[0], wide], 0.3, 0.4, out=out)):
        with pytest.raises(_lib.Yfv2Error) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and "frame 1" in str(e.value) and "wider than %d" % limit in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((dst == 77).all()) and bool((out[0] == SENTINEL).all()) and bool((out[2] == -9).all()), "a failed call wrote its output"


# ---- 4. detection ----------------------------------------------------------------------------------------------------------------
def _picture(images_u8, k, h, w, seed):
    hwc = np.ascontiguousarray(images_u8[k % len(images_u8)].transpose(1, 2, 0))
    rng = np.random.default_rng(seed)
    f = oracle.resize_linear_u8(hwc, w, h)
    return np.clip(f.astype(np.int16) + rng.integers(-3, 4, f.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def p010_batch(yfv2, dev, images_u8):
    """a mixed-size batch of P010 frames made from the reference pictures, and the same frames converted by the model: computed once"""
    frames, bgr = [], []
    for k, (w, h) in enumerate([(352, 352), (480, 360), (640, 480)]):
        planes = m16.bgr_to_p010(_picture(images_u8, k, h, w, 500 + k))
        frames.append(yfv2.YuvFrame(_to(dev, planes), "p010", "bt601"))
        bgr.append(_bgr(dev, m16.yuv_to_bgr(planes, m16.P010, m16.BT601_LIMITED, 0, 0, w, h)))
    return frames, bgr


@pytest.mark.parametrize("conf", [0.3, 0.01])
def test_detect_frames_yuv_is_detect_frames_on_the_converted_frames(engine, p010_batch, conf):
    frames, bgr = p010_batch
    B = len(frames)
    got = engine.detect_frames_yuv(frames, conf, 0.4, out=_out(engine, B))
    want = engine.detect_frames(bgr, conf, 0.4, out=_out(engine, B))
    assert torch.equal(got[2], want[2]), (got[2].tolist(), want[2].tolist())
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0], want[0])
    _same_words(got[0], want[0], "dets at conf %g" % conf)
    assert int(want[2].sum()) > 0, want[2].tolist()


def test_detect_tiled_yuv_is_detect_tiled_on_the_converted_frames(yfv2, engine, dev, images_u8):
    """F = 2 frames of 500 x 420; 352 x 352 tiles 75 pixels apart, so a column of tiles starts at x = 75: odd origins read in place"""
    tiles = [t for f in range(2) for t in yfv2.plan_tiles(420, 500, tile=(352, 352), overlap=(277, 277), frame=f)]
    assert len(tiles) <= engine.max_batch and any(t[1] % 2 == 1 for t in tiles) and any(t[1] % 2 == 0 and t[1] > 0 for t in tiles)
    frames, bgr = [], []
    for f in range(2):
        planes = m16.bgr_to_p010(_picture(images_u8, 1 + f, 420, 500, 600 + f))
        frames.append(yfv2.YuvFrame(_to(dev, planes), "p010", "bt601"))
        bgr.append(_bgr(dev, m16.yuv_to_bgr(planes, m16.P010, m16.BT601_LIMITED, 0, 0, 500, 420)))

    def buffers():
        d, s, c = engine.new_tiled_buffers(2)
        d.fill_(SENTINEL)
        s.fill_(-7)
        c.fill_(-9)
        return d, s, c

    got = engine.detect_tiled_yuv(frames, tiles=tiles, conf_thres=0.3, iou_thres=0.4, out=buffers())
    want = engine.detect_tiled(bgr, tiles=tiles, conf_thres=0.3, iou_thres=0.4, out=buffers())
    assert torch.equal(got[2], want[2]) and torch.equal(got[1], want[1]), (got[2].tolist(), want[2].tolist())
    _same_words(got[0], want[0], "tiled dets")
    assert int(want[2].sum()) > 0


def test_pipeline_submit_frames_yuv(yfv2, dev, cfg, coco_weights, engine, p010_batch):
    frames, bgr = p010_batch
    pipe = yfv2.DetectPipeline(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=4, depth=2, plan={})
    pipe.load_state_dict(coco_weights)
    d, i, c = (t.clone() for t in pipe.result(pipe.submit_frames_yuv(frames, 0.3, 0.4)))
    pipe.synchronize()
    rd, ri, rc = engine.detect_frames(bgr, 0.3, 0.4)
    assert tuple(d.shape) == (len(frames), MAX_DET, 6) and torch.equal(c, rc) and int(c.sum()) > 0
    for b in range(len(frames)):
        k = int(c[b])
        assert torch.equal(i[b, :k], ri[b, :k])
        _same_words(d[b, :k], rd[b, :k], "pipeline frame %d" % b)


# ---- 5. training batches and second-stage crops --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(yfv2, dev):
    """3 small frames - P010 at an odd origin, I010 whole, P010 one pixel high - and their model conversions"""
    rng = np.random.default_rng(41)
    frames, bgr = [], []
    for fmt, colour, (rows, cols), (x0, y0, w, h) in ((m16.P010, m16.BT709_LIMITED, (45, 83), (3, 1, 77, 41)), (m16.I010, m16.BT601_FULL, (64, 96), (0, 0, 96, 64)),
                                                      (m16.P010, m16.BT601_LIMITED, (9, 30), (2, 7, 25, 1))):
        planes = m16.random_planes(rng, rows, cols, fmt)
        frames.append(yfv2.YuvFrame(_to(dev, planes), NAMES[fmt], colour, x0, y0, w, h))
        bgr.append(_bgr(dev, m16.yuv_to_bgr(planes, fmt, colour, x0, y0, w, h)))
    return frames, bgr


def test_train_batch_frames_yuv(yfv2, dev, small):
    frames, bgr = small
    eng = yfv2.Engine(dev, 64, 96, max_batch=3, plan={})
    alpha, beta = [1.0, 0.5, 1.75], [0.0, 0.25, -7.25]
    for a, b in ((alpha, beta), (None, None)):
        got = eng.train_batch_frames_yuv(frames, a, b)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 64, 96)
        _same_words(got, eng.train_batch_frames(bgr, a, b), "training batch")
    from yolo_fastestv2_amd import datasets
    labels = [np.zeros((0, 6), np.float32)] * 3
    imgs, _ = datasets.TrainBatcher(eng)(frames, labels)
    _same_words(imgs, eng.train_batch_frames(bgr), "TrainBatcher")


def _hand_rows(frames):
    """hand-made rows on the first 2 frames: inside, odd and even origins, touching the far corner, one outside (skipped)"""
    dets = np.full((2, 8, 6), -3.0, np.float32)
    count = np.zeros(2, np.int32)
    for b, f in enumerate(frames[:2]):
        w, h = f.width, f.height
        rows = [(0.31 * w, 0.22 * h, 0.74 * w, 0.81 * h, 0.9, 0), (5.0, 3.0, 30.0, 28.0, 0.8, 1), (6.5, 4.0, 31.0, 29.5, 0.7, 2), (w - 9.0, h - 7.0, w + 4.0, h + 4.0, 0.6, 3),
                (0.0, 0.0, 1.0, 1.0, 0.5, 0), (w + 5.0, 2.0, w + 9.0, 8.0, 0.4, 0), (0.0, 0.0, float(w), float(h), 0.3, 4)]
        dets[b, :len(rows)], count[b] = rows, len(rows)
    return dets, count


def test_crop_detections_yuv(yfv2, dev, small):
    """the crop plan folds each rectangle into the plane pointers ON THE DEVICE: two-byte samples there too"""
    frames, bgr = small
    eng = yfv2.Engine(dev, 352, 352, max_batch=2, plan={})
    dets, count = _hand_rows(frames)
    d, c = torch.from_numpy(dets).to(dev), torch.from_numpy(count).to(dev)
    got = eng.crop_detections_yuv(frames[:2], d, c, (32, 32), pad=0.1)
    want = eng.crop_detections(bgr[:2], d, c, (32, 32), pad=0.1)
    torch.cuda.synchronize()
    total = int(want[3][-1])
    assert total >= 10 and {int(r[0]) & 1 for r in want[2][:total]} == {0, 1} and {int(r[1]) & 1 for r in want[2][:total]} == {0, 1}
    for g, w_, name in zip(got[1:], want[1:], ("crop_src", "crop_rect", "crop_offset", "crop_skipped")):
        n = total if name in ("crop_src", "crop_rect") else len(w_)          # (slots beyond the total are not written)
        assert torch.equal(g[:n], w_[:n]), name
    _same_words(got[0][:total], want[0][:total], "crops")


@pytest.mark.parametrize("dtype,letterbox", [(torch.float32, False), (torch.float16, True)], ids=["fp32", "fp16_letterboxed"])
def test_crop_tensors_yuv(yfv2, dev, small, dtype, letterbox):
    frames, bgr = small
    eng = yfv2.Engine(dev, 352, 352, max_batch=2, plan={})
    dets, count = _hand_rows(frames)
    d, c = torch.from_numpy(dets).to(dev), torch.from_numpy(count).to(dev)
    kw = dict(pad=0.1, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), rgb=True, letterbox=letterbox, fill=(114, 7, 201), dtype=dtype)
    got = eng.crop_tensors_yuv(frames[:2], d, c, (32, 32), **kw)
    want = eng.crop_tensors(bgr[:2], d, c, (32, 32), **kw)
    torch.cuda.synchronize()
    total = int(want[3][-1])
    assert total >= 10 and got[0].dtype == dtype
    for g, w_, name in zip(got[1:], want[1:], ("crop_src", "crop_rect", "crop_offset", "crop_skipped")):
        n = total if name in ("crop_src", "crop_rect") else len(w_)          # (slots beyond the total are not written)
        assert torch.equal(g[:n], w_[:n]), name
    _same_words(got[0][:total], want[0][:total], "tensors")


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(yfv2, dev, engine, p010_batch):
    from yolo_fastestv2_amd import _lib
    frames, bgr = p010_batch
    y, uv = frames[2].planes           # 640 x 480 samples
    u = torch.zeros((240, 320), dtype=torch.int16, device=dev)
    y8, uv8 = torch.zeros((480, 640), dtype=torch.uint8, device=dev), torch.zeros((240, 640), dtype=torch.uint8, device=dev)
    # what the Python layer refuses itself
    for bad in (yfv2.YuvFrame((y, uv), "p010", width=641), yfv2.YuvFrame((y, uv[:, :638]), "p010"), yfv2.YuvFrame((y, uv), "i010"), yfv2.YuvFrame((y, uv.float()), "p010")):
        with pytest.raises(ValueError):
            engine.resize_frames_yuv([frames[0], bad])
    with pytest.raises(ValueError, match="frame 1"):
        engine.detect_frames_yuv([frames[0], yfv2.YuvFrame((y8, uv8), "nv12")], 0.3, 0.4)
    out = _out(engine, 4)
    dst = torch.full((4, 352, 352, 3), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L, h = _lib.lib(), engine._h
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    good = dict(y=y.data_ptr(), u=uv.data_ptr(), v=None, pitch_y=1280, pitch_c=1280, x0=0, y0=0, width=640, height=480, format=m16.P010, colour=0)
    planar = dict(good, u=u.data_ptr(), v=u.data_ptr(), pitch_c=640, format=m16.I010)
    nv12 = dict(good, y=y8.data_ptr(), u=uv8.data_ptr(), pitch_y=640, pitch_c=640, format=0)

    def table(*fs):
        arr = (_lib.FrameYuv * len(fs))()
        for i, f in enumerate(fs):
            for k, v in f.items():
                setattr(arr[i], k, v)
        return arr

    cases = [   # (frames, words of the message)
        (table(good, dict(good, y=y.data_ptr() + 1)), ["frame 1", "y must be 2-byte aligned"]),
        (table(dict(good, u=uv.data_ptr() + 1)), ["frame 0", "u must be 2-byte aligned"]),
        (table(dict(planar, v=u.data_ptr() + 1)), ["frame 0", "v must be 2-byte aligned"]),
        (table(dict(good, pitch_c=1281)), ["frame 0", "pitch_c 1281 must be even"]),
        (table(dict(good, pitch_y=1283)), ["frame 0", "pitch_y 1283 must be even"]),
        (table(dict(good, pitch_y=1278)), ["frame 0", "pitch_y 1278 < 2 * (x0 + width)"]),
        (table(dict(good, x0=1, pitch_y=1280)), ["frame 0", "pitch_y 1280 < 2 * (x0 + width)"]),
        (table(dict(good, pitch_c=1278)), ["frame 0", "pitch_c 1278 < 1280"]),
        (table(dict(planar, pitch_c=638)), ["frame 0", "pitch_c 638 < 640"]),
        (table(good, dict(planar, v=None)), ["frame 1", "null v", "I010"]),
        (table(good, nv12), ["frame 1", "sample width"]),
        (table(nv12, nv12, good), ["frame 2", "sample width"]),
        (table(dict(good, format=18)), ["frame 0", "unknown format 18"]),
        (table(dict(good, format=3)), ["frame 0", "unknown format 3"]),
        (table(dict(good, width=20344, pitch_y=40688, pitch_c=40688)), ["frame 0", "wider than 20343"]),
    ]
    for arr, words in cases:
        rc = L.yfv2_resize_frames_yuv(h, arr, len(arr), _ptr(dst), st)
        msg = _lib.last_error(h)
        assert rc == _lib.ERR_ARG and all(w in msg for w in words) and "yfv2_resize_frames_yuv" in msg, (words, rc, msg)
        rc = L.yfv2_detect_frames_yuv(h, arr, len(arr), 0.3, 0.4, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), st)
        msg = _lib.last_error(h)
        assert rc == _lib.ERR_ARG and all(w in msg for w in words) and "yfv2_detect_frames_yuv" in msg, (words, rc, msg)
    torch.cuda.synchronize()
    assert bool((dst == 77).all()), "a failed call wrote its output"
    assert bool((out[0] == SENTINEL).all()) and bool((out[1] == -7).all()) and bool((out[2] == -9).all()), "a failed call wrote its output"
    # the engine is intact
    got = engine.detect_frames_yuv(frames[:2], 0.3, 0.4, out=_out(engine, 2))
    want = engine.detect_frames(bgr[:2], 0.3, 0.4, out=_out(engine, 2))
    assert torch.equal(got[2], want[2]) and torch.equal(got[1], want[1])
    _same_words(got[0], want[0], "after the errors")
