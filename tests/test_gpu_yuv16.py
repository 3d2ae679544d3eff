"""GPU tests of the 10-bit YUV front door: P010 and I010 frames through every *_yuv entry point (include/yfv2.h YFV2_YUV_P010 /
YFV2_YUV_I010).  Run with ``-m gpu`` on an MI355X.

One claim, everywhere: the result for a 10-bit frame is bit-identical to converting that frame to B, G, R with the integer rule of
include/yfv2.h (tests/yuv_model.py states it in numpy) and passing it to the B, G, R entry point of the same name ON THE DEVICE.
Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rows_model
import yuv_model as ym
from yuv_frames import (SENTINEL, _bgr, _out, _pair, _picture, _plane_set, _ptr, _same, _to, check_crop_detections, check_crop_tensors, check_detect_frames,
                        check_detect_tiled, check_pipeline, check_train_batch, check_widest_frame_and_limit, dev, engine, yfv2)  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu
FORMATS = ym.FORMATS16
NAMES = ym.NAMES


# ---- 1. resize equals convert-then-resize ------------------------------------------------------------------------------------
SIZES_WH = [(1, 1), (2, 3), (3, 2), (17, 31), (352, 352), (353, 351), (640, 360), (1279, 721)]


@pytest.mark.parametrize("fmt", FORMATS, ids=["p010", "i010"])
def test_resize_yuv_is_convert_then_resize(yfv2, dev, fmt):
    """One ragged batch: 1 x 1 up to 1279 x 721, 352 x 352 being the identity resize - the pure conversion - each with the colour
    standard k % 4 (all four occur), random values over all of 0..1023 (the clamps fire) and random junk in the ignored bits."""
    rng = np.random.default_rng(100 + fmt)
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(SIZES_WH), plan={})
    frames, bgr = [], []
    for k, (w, h) in enumerate(SIZES_WH):
        planes = ym.random_planes(rng, h, w, fmt)
        frames.append(yfv2.YuvFrame(_to(dev, planes), NAMES[fmt], k % 4))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, fmt, k % 4, 0, 0, w, h)))
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(SIZES_WH), 352, 352, 3)
    for b, (w, h) in enumerate(SIZES_WH):
        _same(got[b], want[b], "frame %d (%d x %d, colour %d)" % (b, w, h, b % 4))
    k = SIZES_WH.index((352, 352))
    assert torch.equal(got[k], bgr[k]), "the identity resize is the pure conversion"
    assert bool((got == 0).any()) and bool((got == 255).any())


# ---- 2. crops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=["p010", "i010"])
def test_crops_of_padded_planes_read_in_place(yfv2, dev, fmt):
    """One 97 x 131 plane set in ONE int16 tensor that ends with the last plane's last sample: every plane at a byte offset that is
    2 mod 4, allocated exactly ((rows - 1) * pitch + width words), odd pitches in words (so rows alternate between misalignment 2
    and 0), the padding between rows poison words.  Frames: every (x0, y0) parity, inside the planes and ending on their last sample."""
    rng = np.random.default_rng(200 + fmt)
    rows, cols = 97, 131
    planes = ym.random_planes(rng, rows, cols, fmt)
    pitches = [137] + [planes[1].shape[1] + 5] * (len(planes) - 1)             # words
    flat, host, views, offs = _plane_set(dev, planes, pitches, [(1, 2)] * 3)                                # odd word offsets
    assert all(2 * q % 4 == 2 for q in offs)
    rects = []
    for x0, y0 in ((0, 0), (1, 0), (0, 1), (1, 1)):
        rects.append((10 + x0, 20 + y0, 50 + x0, 40 + y0))            # inside: poison on both sides of every row
        rects.append((cols - 3 - x0, rows - 4 - y0, 3 + x0, 4 + y0))  # the bottom-right corner: ends at the planes' last sample
    rects += [(1, 1, cols - 1, rows - 1), (cols - 1, rows - 1, 1, 1), (0, 0, 1, 1), (cols - 2, 0, 2, rows), (0, rows - 1, cols, 1)]
    assert {(x0 & 1, y0 & 1) for x0, y0, _w, _h in rects} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert any(x0 + w == cols and y0 + h == rows for x0, y0, w, h in rects)
    frames = [yfv2.YuvFrame(views, NAMES[fmt], k % 4, x0, y0, w, h) for k, (x0, y0, w, h) in enumerate(rects)]
    bgr = [_bgr(dev, ym.yuv_to_bgr(planes, fmt, k % 4, x0, y0, w, h)) for k, (x0, y0, w, h) in enumerate(rects)]
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(rects), plan={})
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    for b, r in enumerate(rects):
        _same(got[b], want[b], "crop %d %s" % (b, r))
    # the same planes as uint8 tensors of the bytes (pitch = stride(0)), and a frame made with crop(): the same descriptors
    bytes_ = flat.view(torch.uint8)
    bviews = tuple(torch.as_strided(bytes_, (p.shape[0], 2 * p.shape[1]), (2 * q, 1), 2 * off) for p, q, off in zip(planes, pitches, offs))
    again = eng.resize_frames_yuv([yfv2.YuvFrame(bviews, NAMES[fmt], 1, 0, 0, cols, rows).crop(*rects[3]), yfv2.YuvFrame(views, NAMES[fmt], 1).crop(*rects[3])])
    ref = eng.resize_frames([_bgr(dev, ym.yuv_to_bgr(planes, fmt, 1, *rects[3]))])[0]
    _same(again[0], ref, "byte planes")
    _same(again[1], ref, "crop()")
    assert np.array_equal(flat.cpu().numpy().view(np.uint16), host)


# ---- 3. the widest frame, and one pixel more -----------------------------------------------------------------------------------
def test_widest_frame_and_the_limit(yfv2, dev, engine):
    limit = rows_model.max_width(rows_model.U8, rows_model.YUV16, 352)
    assert limit == yfv2.yuv.max_width(352, bits=10) == 20343 <= rows_model.max_width(rows_model.U8, rows_model.BGR, 352)
    wide = yfv2.YuvFrame((torch.zeros((2, limit + 1), dtype=torch.int16, device=dev), torch.zeros((1, limit + 2), dtype=torch.int16, device=dev)), "p010")
    check_widest_frame_and_limit(yfv2, dev, engine, np.random.default_rng(300), FORMATS, limit, [wide])


# ---- 4. detection ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def p010_batch(yfv2, dev, images_u8):
    """a mixed-size batch of P010 frames made from the reference pictures, and the same frames converted by the model: computed once"""
    frames, bgr = [], []
    for k, (w, h) in enumerate([(352, 352), (480, 360), (640, 480)]):
        planes = ym.bgr_to_p010(_picture(images_u8, k, h, w, 500 + k))
        frames.append(yfv2.YuvFrame(_to(dev, planes), "p010", "bt601"))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, ym.P010, ym.BT601_LIMITED, 0, 0, w, h)))
    return frames, bgr


@pytest.mark.parametrize("conf", [0.3, 0.01])
def test_detect_frames_yuv_is_detect_frames_on_the_converted_frames(engine, p010_batch, conf):
    check_detect_frames(engine, *p010_batch, conf)


def test_detect_tiled_yuv_is_detect_tiled_on_the_converted_frames(yfv2, engine, dev, images_u8):
    frames, bgr = [], []
    for f in range(2):
        planes = ym.bgr_to_p010(_picture(images_u8, 1 + f, 420, 500, 600 + f))
        frames.append(yfv2.YuvFrame(_to(dev, planes), "p010", "bt601"))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, ym.P010, ym.BT601_LIMITED, 0, 0, 500, 420)))
    check_detect_tiled(yfv2, engine, frames, bgr)


def test_pipeline_submit_frames_yuv(yfv2, dev, cfg, coco_weights, engine, p010_batch):
    check_pipeline(yfv2, dev, cfg, coco_weights, engine, [p010_batch], 4)


# ---- 5. training batches and second-stage crops --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(yfv2, dev):
    """3 small frames - P010 at an odd origin, I010 whole, P010 one pixel high - and their model conversions"""
    rng = np.random.default_rng(41)
    pairs = [_pair(yfv2, dev, ym.random_planes(rng, rows, cols, fmt), fmt, colour, *rect)
             for fmt, colour, (rows, cols), rect in ((ym.P010, ym.BT709_LIMITED, (45, 83), (3, 1, 77, 41)), (ym.I010, ym.BT601_FULL, (64, 96), (0, 0, 96, 64)),
                                                     (ym.P010, ym.BT601_LIMITED, (9, 30), (2, 7, 25, 1)))]
    return [f for f, _ in pairs], [b for _, b in pairs]


def test_train_batch_frames_yuv(yfv2, dev, small):
    check_train_batch(yfv2, dev, *small, [1.0, 0.5, 1.75], [0.0, 0.25, -7.25])


def _rows(w, h):
    """inside, odd and even origins, touching the far corner, one outside (skipped), the whole frame"""
    return [(0.31 * w, 0.22 * h, 0.74 * w, 0.81 * h, 0.9, 0), (5.0, 3.0, 30.0, 28.0, 0.8, 1), (6.5, 4.0, 31.0, 29.5, 0.7, 2), (w - 9.0, h - 7.0, w + 4.0, h + 4.0, 0.6, 3),
            (0.0, 0.0, 1.0, 1.0, 0.5, 0), (w + 5.0, 2.0, w + 9.0, 8.0, 0.4, 0), (0.0, 0.0, float(w), float(h), 0.3, 4)]


def test_crop_detections_yuv(yfv2, dev, small):
    """the first 2 frames; two-byte samples in the fold on the device too"""
    frames, bgr = small
    check_crop_detections(yfv2, dev, frames[:2], bgr[:2], _rows, 0.1, 10, [None])


@pytest.mark.parametrize("dtype,letterbox", [(torch.float32, False), (torch.float16, True)], ids=["fp32", "fp16_letterboxed"])
def test_crop_tensors_yuv(yfv2, dev, small, dtype, letterbox):
    frames, bgr = small
    check_crop_tensors(yfv2, dev, frames[:2], bgr[:2], _rows, 0.1, 10, [], dtype, letterbox)


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
    good = dict(y=y.data_ptr(), u=uv.data_ptr(), v=None, pitch_y=1280, pitch_c=1280, x0=0, y0=0, width=640, height=480, format=ym.P010, colour=0)
    planar = dict(good, u=u.data_ptr(), v=u.data_ptr(), pitch_c=640, format=ym.I010)
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
    _same(got[0], want[0], "after the errors")
