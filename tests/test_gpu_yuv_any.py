"""GPU tests of the 8-bit YUV samplings beyond 4:2:0: I422, I440, I444, YUYV, UYVY and GREY frames, alone and mixed with NV12 / NV21 /
I420, through every *_yuv entry point (include/yfv2.h YFV2_YUV_I422 .. YFV2_YUV_GREY).  Run with ``-m gpu`` on an
MI355X.

One claim, everywhere: the result for such a frame is bit-identical to converting that frame to B, G, R with the integer rule of
include/yfv2.h (tests/yuv_model.py states it in numpy) and passing it to the B, G, R entry point of the same name ON THE DEVICE.
Every comparison is exact: the file has no tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rows_model
import yuv_model as ym
from yuv_frames import (SENTINEL, _bgr, _frame, _out, _pair, _picture, _plane_set, _ptr, _same, _to, check_crop_detections, check_crop_tensors, check_detect_frames,
                        check_detect_tiled, check_pipeline, check_train_batch, check_widest_frame_and_limit, dev, engine, yfv2)  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu
NEW = ym.NEW_FORMATS
FORMATS = ym.FORMATS8
IDS = [ym.NAMES[f] for f in NEW]


# ---- 1. resize equals convert-then-resize ------------------------------------------------------------------------------------
SIZES_WH = [(1, 1), (2, 3), (3, 2), (5, 4), (17, 31), (352, 352), (353, 351), (640, 360)]


@pytest.mark.parametrize("fmt", NEW, ids=IDS)
def test_resize_is_convert_then_resize(yfv2, dev, fmt):
    """One ragged batch at W = H = 352: one pixel, a macropixel and a half, odd ends, up-scaling (chroma rows coincide), 1:1 - the
    pure conversion - and down-scaling; bt601_full everywhere and all four colours on 17 x 31; random bytes over all of 0..255."""
    rng = np.random.default_rng(100 + fmt)
    cases = [(w, h, ym.BT601_FULL) for w, h in SIZES_WH] + [(17, 31, c) for c in ym.COLOURS if c != ym.BT601_FULL]
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(cases), plan={})
    frames, bgr = [], []
    for w, h, colour in cases:
        planes = ym.random_planes(rng, h, w, fmt)
        frames.append(yfv2.YuvFrame(_to(dev, planes), ym.NAMES[fmt], colour, 0, 0, w, h))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, fmt, colour, 0, 0, w, h)))
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(cases), 352, 352, 3)
    for b, case in enumerate(cases):
        _same(got[b], want[b], "frame %d %s" % (b, case))
    k = SIZES_WH.index((352, 352))
    assert torch.equal(got[k], bgr[k]), "the identity resize is the pure conversion"
    assert bool((got == 0).any()) and bool((got == 255).any())


# ---- 2. crops of padded planes ---------------------------------------------------------------------------------------------------
def _odd_plane_set(dev, planes, delta, poison):
    """every plane at an odd byte address, pitch = row bytes + delta"""
    return _plane_set(dev, planes, [p.shape[1] + delta for p in planes], [(1, 2)] * 3, poison)[:3]


@pytest.mark.parametrize("fmt", NEW, ids=IDS)
def test_crops_of_padded_planes_read_in_place(yfv2, dev, fmt):
    """A 21 x 37 picture at pitches of its row bytes + 1, + 2, + 3 and + 13 (rows at every misalignment), the planes at odd byte
    addresses.  Per pitch: at each origin parity the rectangle from there to the planes' LAST pixel (its last byte is the last byte
    of the allocation), and one inside the picture with poison on both sides of every row.  Run again with another poison."""
    rng = np.random.default_rng(200 + fmt)
    rows, cols = 21, 37
    planes = ym.random_planes(rng, rows, cols, fmt)
    rects = []
    for x0, y0 in ((0, 0), (1, 0), (0, 1), (1, 1)):
        rects.append((x0, y0, cols - x0, rows - y0))
        rects.append((4 + x0, 2 + y0, 9 + x0, 7))
    rects += [(cols - 1, rows - 1, 1, 1), (cols - 2, 0, 2, rows)]
    assert {(x0 & 1, y0 & 1) for x0, y0, _w, _h in rects} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(rects), plan={})
    want = eng.resize_frames([_bgr(dev, ym.yuv_to_bgr(planes, fmt, k % 4, *r)) for k, r in enumerate(rects)])
    for delta in (1, 2, 3, 13):
        outs = []
        for poison in (ym.POISON, 0x3C):
            flat, host, views = _odd_plane_set(dev, planes, delta, poison)
            frames = [yfv2.YuvFrame(views, ym.NAMES[fmt], k % 4, *r) for k, r in enumerate(rects)]
            outs.append(eng.resize_frames_yuv(frames))
            for b, r in enumerate(rects):
                _same(outs[-1][b], want[b], "pitch + %d, poison %#x, crop %d %s" % (delta, poison, b, r))
            assert np.array_equal(flat.cpu().numpy(), host)
        assert torch.equal(outs[0], outs[1]), "the bytes around the planes changed the result"
    # crop() of a whole frame is the same descriptor
    flat, host, views = _odd_plane_set(dev, planes, 13, ym.POISON)
    again = eng.resize_frames_yuv([yfv2.YuvFrame(views, ym.NAMES[fmt], 1, 0, 0, cols, rows).crop(*rects[3])])
    _same(again[0], eng.resize_frames([_bgr(dev, ym.yuv_to_bgr(planes, fmt, 1, *rects[3]))])[0], "crop()")


# ---- 3. one call mixes the formats --------------------------------------------------------------------------------------------------
MIX_WH = [(640, 360), (37, 21), (352, 352), (353, 351), (100, 75), (480, 270), (333, 111), (64, 200), (1, 9)]


@pytest.fixture(scope="module")
def mixed(yfv2, dev):
    """nine frames, one of each 8-bit format, of different sizes and colours, and their model conversions: computed once"""
    rng = np.random.default_rng(300)
    frames, bgr = [], []
    for k, (fmt, (w, h)) in enumerate(zip(FORMATS, MIX_WH)):
        planes = ym.random_planes(rng, h + 1, w + 3, fmt)
        rect = (k % 3, k % 2, w, h)
        frames.append(_frame(yfv2, dev, planes, fmt, k % 4, *rect))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, fmt, k % 4, *rect)))
    return frames, bgr


def test_mixed_batch_is_each_frame_alone(yfv2, dev, mixed):
    frames, bgr = mixed
    eng = yfv2.Engine(dev, 352, 352, max_batch=9, plan={})
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    for b, fmt in enumerate(FORMATS):
        _same(got[b], eng.resize_frames_yuv([frames[b]])[0], "%s alone" % ym.NAMES[fmt])
        _same(got[b], want[b], "%s against the model" % ym.NAMES[fmt])
    only420 = eng.resize_frames_yuv(frames[:3])                      # the 4:2:0-only launch
    for b in range(3):
        _same(got[b], only420[b], "%s in a 4:2:0-only call" % ym.NAMES[FORMATS[b]])
    # the order of the frames does not matter either: the general frame last, first, in the middle
    back = eng.resize_frames_yuv(frames[::-1])
    for b in range(9):
        _same(back[8 - b], got[b], "reversed, frame %d" % b)


# ---- 4. the widest frame, and the limits ----------------------------------------------------------------------------------------------
def test_widest_frame_and_the_limits(yfv2, dev, engine):
    from yolo_fastestv2_amd import _lib
    limit, limit420 = rows_model.max_width(rows_model.U8, rows_model.YUV8_ANY, 352), rows_model.max_width(rows_model.U8, rows_model.YUV8, 352)
    assert limit == yfv2.yuv.max_width(352, general=True) == 27125 < limit420 == yfv2.yuv.max_width(352) == 40689
    assert limit <= rows_model.max_width(rows_model.U8, rows_model.BGR, 352)          # the B, G, R reference call admits the converted frame
    rng = np.random.default_rng(400)
    z = lambda r, c: torch.zeros((r, c), dtype=torch.uint8, device=dev)
    wide444 = yfv2.YuvFrame((z(2, limit + 1), z(2, limit + 1), z(2, limit + 1)), "i444")
    wide_yuyv = yfv2.YuvFrame(z(2, 2 * (limit + 1)), "yuyv")
    assert wide_yuyv.width == limit + 1
    eng, frames, dst, out = check_widest_frame_and_limit(yfv2, dev, engine, rng, (ym.I444, ym.YUYV), limit, [wide444, wide_yuyv])
    # an NV12 frame wider than the general limit and inside the 4:2:0 one: accepted alone, refused beside an I444 frame
    nv12_w = limit + 1001
    assert limit < nv12_w <= limit420
    nv12 = _frame(yfv2, dev, ym.random_planes(rng, 2, nv12_w, ym.NV12), ym.NV12, ym.BT601_FULL)
    alone = eng.resize_frames_yuv([nv12])
    # (the B, G, R resize does not admit a frame that wide; the claim here is acceptance - the bytes of NV12 frames are tests/test_gpu_yuv.py's)
    assert tuple(alone.shape) == (1, 352, 352, 3)
    for call in (lambda: eng.resize_frames_yuv([frames[0], nv12], out=dst), lambda: engine.detect_frames_yuv([frames[0], nv12], 0.3, 0.4, out=out)):
        with pytest.raises(_lib.Yfv2Error) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and "frame 1" in str(e.value) and "wider than %d" % limit in str(e.value), str(e.value)
    with pytest.raises(_lib.Yfv2Error) as e:
        eng.resize_frames_yuv([nv12, frames[0]], out=dst)               # the batch's kind is not frame 0's: the NV12 frame comes first here
    assert "frame 0" in str(e.value) and "wider than %d" % limit in str(e.value) and "4:2:0" in str(e.value) and str(limit420) in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((dst == 77).all()) and bool((out[0] == SENTINEL).all()) and bool((out[2] == -9).all()), "a failed call wrote its output"


# ---- 5. detection ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def picture_batch(yfv2, dev, images_u8):
    """a mixed-size, mixed-format batch made from the reference pictures, and the same frames converted by the model: computed once"""
    frames, bgr = [], []
    for k, (fmt, (w, h)) in enumerate([(ym.I444, (352, 352)), (ym.YUYV, (480, 360)), (ym.NV12, (640, 480)), (ym.I422, (353, 301)), (ym.GREY, (400, 300)), (ym.I440, (500, 420))]):
        planes = ym.from_i444(ym.bgr_to_i444(_picture(images_u8, k, h, w, 500 + k)), fmt)
        frames.append(_frame(yfv2, dev, planes, fmt, "jpeg", 0, 0, w, h))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, fmt, ym.BT601_FULL, 0, 0, w, h)))
    return frames, bgr


@pytest.mark.parametrize("conf", [0.3, 0.01])
def test_detect_frames_yuv_is_detect_frames_on_the_converted_frames(engine, picture_batch, conf):
    check_detect_frames(engine, *picture_batch, conf)


def test_detect_tiled_yuv_is_detect_tiled_on_the_converted_frames(yfv2, engine, dev, images_u8):
    """a YUYV and an I440 frame: the odd origins lie in the middle of a macropixel"""
    frames, bgr = [], []
    for f, fmt in enumerate((ym.YUYV, ym.I440)):
        planes = ym.from_i444(ym.bgr_to_i444(_picture(images_u8, 1 + f, 420, 500, 600 + f)), fmt)
        frames.append(_frame(yfv2, dev, planes, fmt, "jpeg", 0, 0, 500, 420))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, fmt, ym.BT601_FULL, 0, 0, 500, 420)))
    check_detect_tiled(yfv2, engine, frames, bgr)


def test_pipeline_submit_frames_yuv(yfv2, dev, cfg, coco_weights, engine, picture_batch):
    frames, bgr = (x[:4] for x in picture_batch)
    check_pipeline(yfv2, dev, cfg, coco_weights, engine, [(frames, bgr)], 4)


# ---- 6. training batches and second-stage crops --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(yfv2, dev):
    """4 small frames - YUYV at an odd origin, I440 whole, UYVY at an even origin, NV12 at an odd one - and their model conversions"""
    rng = np.random.default_rng(41)
    pairs = [_pair(yfv2, dev, ym.random_planes(rng, rows, cols, fmt), fmt, colour, *rect)
             for fmt, colour, (rows, cols), rect in ((ym.YUYV, ym.BT709_LIMITED, (45, 84), (3, 1, 77, 41)), (ym.I440, ym.BT601_FULL, (64, 96), (0, 0, 96, 64)),
                                                     (ym.UYVY, ym.BT601_LIMITED, (33, 40), (2, 3, 37, 29)), (ym.NV12, ym.BT709_FULL, (40, 50), (1, 1, 49, 39)))]
    return [f for f, _ in pairs], [b for _, b in pairs]


def test_train_batch_frames_yuv(yfv2, dev, small):
    check_train_batch(yfv2, dev, *small, [1.0, 0.5, 1.75, 0.25], [0.0, 0.25, -7.25, 31.5])


def _rows(w, h):
    """with pad 0.25 a box 8 wide from x1 starts its rectangle at x1 - 2 - odd and even origins on every frame, the packed ones too,
    folded into the plane pointers ON THE DEVICE; then inside, touching the far corner, one outside (skipped), the whole frame"""
    return [(9.0, 6.0, 17.0, 14.0, 0.9, 0), (10.0, 7.0, 18.0, 15.0, 0.8, 1), (0.31 * w, 0.22 * h, 0.74 * w, 0.81 * h, 0.7, 2), (w - 9.0, h - 7.0, w + 4.0, h + 4.0, 0.6, 3),
            (0.0, 0.0, 1.0, 1.0, 0.5, 0), (w + 5.0, 2.0, w + 9.0, 8.0, 0.4, 0), (0.0, 0.0, float(w), float(h), 0.3, 4)]


def test_crop_detections_yuv(yfv2, dev, small):
    """rectangles at odd and even x (and y) on each of the packed frames, 0 and 2"""
    check_crop_detections(yfv2, dev, *small, _rows, 0.25, 20, [{0}, {2}])


@pytest.mark.parametrize("dtype,letterbox", [(torch.float32, False), (torch.float16, True)], ids=["fp32", "fp16_letterboxed"])
def test_crop_tensors_yuv(yfv2, dev, small, dtype, letterbox):
    check_crop_tensors(yfv2, dev, *small, _rows, 0.25, 20, [{0}, {2}], dtype, letterbox)


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(yfv2, dev, engine, picture_batch):
    from yolo_fastestv2_amd import _lib
    frames, bgr = picture_batch
    limit = yfv2.yuv.max_width(352, general=True)
    y = torch.zeros((480, 1280), dtype=torch.uint8, device=dev)        # 640 pixels of a packed plane, or a luma plane with room
    u = torch.zeros((480, 640), dtype=torch.uint8, device=dev)
    p10 = torch.zeros((480, 640), dtype=torch.int16, device=dev)
    # what the Python layer refuses itself: plane counts, short planes, a 10-bit frame among 8-bit ones
    for bad in (yfv2.YuvFrame((y, u), "i444"), yfv2.YuvFrame((y, u, u), "yuyv"), yfv2.YuvFrame((y[:, :1279],), "yuyv", width=640), yfv2.YuvFrame((y, u, u[:, :639]), "i444", width=640),
                yfv2.YuvFrame((y, u, u), "i422", width=1282), yfv2.YuvFrame((p10, p10), "p010")):
        with pytest.raises(ValueError, match="frame 1"):
            engine.resize_frames_yuv([frames[0], bad])
    out = _out(engine, 4)
    dst = torch.full((4, 352, 352, 3), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L, h = _lib.lib(), engine._h
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    i444 = dict(y=y.data_ptr(), u=u.data_ptr(), v=u.data_ptr(), pitch_y=1280, pitch_c=640, x0=0, y0=0, width=640, height=480, format=ym.I444, colour=2)
    i422, i440 = dict(i444, format=ym.I422, pitch_c=320), dict(i444, format=ym.I440)
    yuyv = dict(i444, u=None, v=None, pitch_c=-5, format=ym.YUYV)
    uyvy, grey = dict(yuyv, format=ym.UYVY), dict(yuyv, format=ym.GREY)
    nv12 = dict(i444, v=None, format=ym.NV12)
    p010 = dict(i444, y=p10.data_ptr(), u=p10.data_ptr(), v=None, pitch_c=1280, format=16, colour=0)

    def table(*fs):
        arr = (_lib.FrameYuv * len(fs))()
        for i, f in enumerate(fs):
            for k, v in f.items():
                setattr(arr[i], k, v)
        return arr

    cases = [   # (frames, words of the message)
        (table(i444, dict(i444, v=None)), ["frame 1", "null v", "I444"]),
        (table(dict(i422, v=None)), ["frame 0", "null v", "I422"]),
        (table(nv12, dict(i440, v=None)), ["frame 1", "null v", "I440"]),
        (table(dict(i444, u=None)), ["frame 0", "null u"]),
        (table(yuyv, dict(grey, y=None)), ["frame 1", "null y"]),
        (table(dict(i444, pitch_y=639)), ["frame 0", "pitch_y 639 < x0 + width"]),
        (table(dict(i422, x0=1, pitch_y=640)), ["frame 0", "pitch_y 640 < x0 + width"]),
        (table(dict(grey, pitch_y=639)), ["frame 0", "pitch_y 639 < x0 + width"]),
        (table(dict(yuyv, pitch_y=1279)), ["frame 0", "pitch_y 1279 < 1280", "macropixel"]),
        (table(yuyv, dict(uyvy, width=639, pitch_y=1279)), ["frame 1", "pitch_y 1279 < 1280", "macropixel"]),       # an odd last pixel reads its whole macropixel
        (table(dict(uyvy, x0=1, width=638, pitch_y=1279)), ["frame 0", "pitch_y 1279 < 1280"]),
        (table(dict(i444, pitch_c=639)), ["frame 0", "pitch_c 639 < 640"]),
        (table(dict(i440, x0=1, width=639, pitch_c=639)), ["frame 0", "pitch_c 639 < 640"]),
        (table(dict(i422, pitch_c=319)), ["frame 0", "pitch_c 319 < 320"]),
        (table(dict(i422, x0=1, width=639, pitch_c=319)), ["frame 0", "pitch_c 319 < 320"]),
        (table(dict(i444, pitch_c=(1 << 40) + 1)), ["frame 0", "pitch_c out of range"]),
        (table(dict(i422, height=(1 << 13) + 1, pitch_c=1 << 40)), ["frame 0", "pitch_c out of range"]),      # 4:2:2 has a chroma row per luma row: no vertical shift
        (table(dict(yuyv, pitch_y=(1 << 40) + 1)), ["frame 0", "pitch_y out of range"]),
        (table(dict(i444, colour=4)), ["frame 0", "unknown colour 4"]),
        (table(dict(i444, format=9)), ["frame 0", "unknown format 9"]),
        (table(i444, dict(i444, format=15)), ["frame 1", "unknown format 15"]),
        (table(i444, p010), ["frame 1", "sample width"]),
        (table(p010, yuyv), ["frame 1", "sample width"]),
        (table(dict(i444, width=limit + 1, pitch_y=limit + 1, pitch_c=limit + 1)), ["frame 0", "wider than %d" % limit]),
        (table(dict(yuyv, width=limit + 1, pitch_y=2 * limit + 2)), ["frame 0", "wider than %d" % limit]),
        (table(dict(nv12, width=limit + 1, pitch_y=limit + 1, pitch_c=limit + 1), grey), ["frame 0", "wider than %d" % limit, "4:2:0", "40689"]),
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
    # u and v NULL and any pitch_c are fine for the packed formats and grey: these calls succeed (a black picture: nothing to detect)
    ok = table(yuyv, uyvy, grey, dict(yuyv, x0=1, width=639))
    assert L.yfv2_resize_frames_yuv(h, ok, 4, _ptr(dst), st) == _lib.OK, _lib.last_error(h)
    torch.cuda.synchronize()
    assert not bool((dst == 77).any())
    # the engine is intact
    got = engine.detect_frames_yuv(frames[:2], 0.3, 0.4, out=_out(engine, 2))
    want = engine.detect_frames(bgr[:2], 0.3, 0.4, out=_out(engine, 2))
    assert torch.equal(got[2], want[2]) and torch.equal(got[1], want[1])
    _same(got[0], want[0], "after the errors")
