"""GPU tests of the YUV 4:2:0 front door: Engine.resize_frames_yuv / detect_frames_yuv / detect_tiled_yuv and
DetectPipeline.submit_frames_yuv (include/yfv2.h yfv2_resize_frames_yuv, yfv2_detect_frames_yuv, yfv2_detect_tiled_yuv).
Run with ``-m gpu`` on an MI355X.

One claim, everywhere: the result for a YUV frame is bit-identical to converting that frame to B, G, R with the integer rule of
include/yfv2.h (tests/yuv_model.py states it in numpy) and passing it to the existing B, G, R entry point ON THE DEVICE.  Every
comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rows_model
import yuv_model as ym
from yuv_frames import (SENTINEL, _bgr, _out, _picture, _plane_set, _ptr, _same, _to, check_detect_frames, check_detect_tiled, check_pipeline,
                        check_widest_frame_and_limit, dev, engine, new_engine, yfv2)  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu
FORMATS = ym.FORMATS420


# ---- 1. resize equals convert-then-resize ------------------------------------------------------------------------------------
SIZES_WH = [(1, 1), (2, 2), (3, 5), (5, 3), (7, 9), (33, 47), (351, 353), (352, 352), (640, 480), (1279, 721)]


@pytest.mark.parametrize("fmt", FORMATS, ids=["nv12", "nv21", "i420"])
def test_resize_yuv_is_convert_then_resize(yfv2, dev, fmt):
    """One ragged batch: every size of the list (1 x 1 up to 1279 x 721, 352 x 352 being the identity resize - the pure conversion),
    each with the colour standard k % 4, and the 7 x 9 and 640 x 480 frames once more under each of the other three standards.
    Random planes, U and V over the full range: the clamps fire."""
    rng = np.random.default_rng(100 + fmt)
    items = [(w, h, k % 4) for k, (w, h) in enumerate(SIZES_WH)]
    for k in (4, 8):
        items += [(SIZES_WH[k][0], SIZES_WH[k][1], c) for c in ym.COLOURS if c != k % 4]
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(items), plan={})
    frames, bgr = [], []
    for w, h, colour in items:
        planes = ym.random_planes(rng, h, w, fmt)
        frames.append(yfv2.YuvFrame(_to(dev, planes), fmt, colour))
        bgr.append(torch.from_numpy(ym.yuv_to_bgr(planes, fmt, colour, 0, 0, w, h)).to(dev))
    assert {c for w, h, c in items if (w, h) == (7, 9)} == set(ym.COLOURS) == {c for w, h, c in items if (w, h) == (640, 480)}
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(items), 352, 352, 3)
    for b, (w, h, colour) in enumerate(items):
        _same(got[b], want[b], "frame %d (%d x %d, colour %d)" % (b, w, h, colour))
    k = SIZES_WH.index((352, 352))
    assert torch.equal(got[k], bgr[k]), "the identity resize is the pure conversion"
    assert bool((got == 0).any()) and bool((got == 255).any())


# ---- 2. crops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=["nv12", "nv21", "i420"])
def test_crops_of_padded_planes_at_odd_addresses(yfv2, dev, fmt):
    """One 97 x 131 plane set in ONE byte tensor that ends with the last plane's last byte: the luma plane at byte offset 1, the
    chroma plane(s) at offsets that are 3 (and 2) mod 4, each allocated exactly ((rows - 1) * pitch + width bytes), odd pitches, the
    padding between rows poisoned.  Frames: every (x0, y0) parity, ending on the planes' last row and column and inside them."""
    rng = np.random.default_rng(200 + fmt)
    rows, cols = 97, 131
    planes = ym.random_planes(rng, rows, cols, fmt)
    pitches = [137] + [planes[1].shape[1] + 5] * (len(planes) - 1)
    flat, host, views, offs = _plane_set(dev, planes, pitches, [(1, 4), (3, 4), (2, 4)])
    assert [q % 4 for q in offs] == [1, 3, 2][:len(offs)]
    rects = []
    for x0, y0 in ((0, 0), (1, 0), (0, 1), (1, 1)):
        rects.append((x0, y0, cols - x0, rows - y0))                   # ends on the last row and column
        rects.append((10 + x0, 20 + y0, 50 + x0, 40 + y0))            # inside: poison on both sides of every row
        rects.append((cols - 3 - x0, rows - 4 - y0, 3 + x0, 4 + y0))  # the bottom-right corner
    rects += [(cols - 1, rows - 1, 1, 1), (0, 0, 1, 1), (cols - 2, 0, 2, rows), (0, rows - 1, cols, 1)]
    frames = [yfv2.YuvFrame(views, fmt, k % 4, x0, y0, w, h) for k, (x0, y0, w, h) in enumerate(rects)]
    bgr = [torch.from_numpy(ym.yuv_to_bgr(planes, fmt, k % 4, x0, y0, w, h)).to(dev) for k, (x0, y0, w, h) in enumerate(rects)]
    eng = yfv2.Engine(dev, 352, 352, max_batch=len(rects), plan={})
    got = eng.resize_frames_yuv(frames)
    want = eng.resize_frames(bgr)
    for b, r in enumerate(rects):
        _same(got[b], want[b], "crop %d %s" % (b, r))
    # a frame made with crop() is the same descriptor
    again = eng.resize_frames_yuv([yfv2.YuvFrame(views, fmt, 1).crop(*rects[4])])
    _same(again[0], eng.resize_frames([torch.from_numpy(ym.yuv_to_bgr(planes, fmt, 1, *rects[4])).to(dev)])[0], "crop()")
    assert np.array_equal(flat.cpu().numpy(), host)


# ---- 3. the widest frame, and one pixel more -----------------------------------------------------------------------------------
def test_widest_frame_and_the_limit(yfv2, dev, engine):
    limit = rows_model.max_width(rows_model.U8, rows_model.YUV8, 352)
    assert limit == yfv2.yuv.max_width(352) == 40689
    wide = yfv2.YuvFrame((torch.zeros((2, limit + 1), dtype=torch.uint8, device=dev), torch.zeros((1, limit + 2), dtype=torch.uint8, device=dev)), "nv12")
    check_widest_frame_and_limit(yfv2, dev, engine, np.random.default_rng(300), FORMATS, limit, [wide], by_oracle=True)


# ---- 4. detection ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nv12_batch(yfv2, dev, images_u8):
    """a mixed-size batch of NV12 frames made from the reference pictures, and the same frames converted by the model: computed once"""
    sizes = [(480, 640), (1080, 1920), (720, 1280), (352, 352), (300, 500), (201, 261), (353, 351)]
    frames, bgr = [], []
    for k, (h, w) in enumerate(sizes):
        planes = ym.bgr_to_nv12(_picture(images_u8, k, h, w, 500 + k))
        frames.append(yfv2.YuvFrame(_to(dev, planes), "nv12", "bt601"))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, ym.NV12, ym.BT601_LIMITED, 0, 0, w, h)))
    return frames, bgr


@pytest.mark.parametrize("conf", [0.3, 0.01])
def test_detect_frames_yuv_is_detect_frames_on_the_converted_frames(engine, nv12_batch, conf):
    want = check_detect_frames(engine, *nv12_batch, conf)
    assert int((want[2] > 0).sum()) >= 4, want[2].tolist()
    # frame coordinates: a box of the 1920-wide frame reaches beyond the network's 352 columns
    assert float(want[0][1, :int(want[2][1]), 2].max()) > 352.0


def _tiled_pair(yfv2, dev, images_u8):
    frames, bgr = [], []
    for f in range(2):
        planes = ym.bgr_to_nv12(_picture(images_u8, 1 + f, 420, 500, 600 + f))
        frames.append(yfv2.YuvFrame(_to(dev, planes), "nv12", "bt601"))
        bgr.append(_bgr(dev, ym.yuv_to_bgr(planes, ym.NV12, ym.BT601_LIMITED, 0, 0, 500, 420)))
    return frames, bgr


def test_detect_tiled_yuv_is_detect_tiled_on_the_converted_frames(yfv2, engine, dev, images_u8):
    check_detect_tiled(yfv2, engine, *_tiled_pair(yfv2, dev, images_u8), planned_by_the_call=True)


def test_pipeline_submit_frames_yuv(yfv2, dev, cfg, coco_weights, engine, nv12_batch):
    frames, _ = nv12_batch
    check_pipeline(yfv2, dev, cfg, coco_weights, engine, [(frames[:3], None), (frames, None), (frames[2:6], None)], 8)


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------------
def test_yuv_argument_errors_launch_nothing(yfv2, dev, cfg, coco_weights, nv12_batch):
    from yolo_fastestv2_amd import _lib
    eng = new_engine(yfv2, dev, cfg, coco_weights, 4)
    frames, bgr = nv12_batch
    y, uv = frames[0].planes           # 480 x 640
    u = torch.zeros((240, 320), dtype=torch.uint8, device=dev)
    # what the Python layer refuses itself: planes that do not hold the frame, wrong plane counts, types and devices
    for bad in (yfv2.YuvFrame((y, uv), "nv12", width=641), yfv2.YuvFrame((y, uv), "nv12", y0=1, height=480), yfv2.YuvFrame((y, uv[:, :638]), "nv12"),
                yfv2.YuvFrame((y, uv), "i420"), yfv2.YuvFrame((y, u, u[:, :319]), "i420"), yfv2.YuvFrame((y, uv.cpu()), "nv12"),
                yfv2.YuvFrame((y, uv.float()), "nv12"), yfv2.YuvFrame((y, uv), "nv12", x0=-1, width=10), yfv2.YuvFrame((y[:, ::2], uv), "nv12")):
        with pytest.raises(ValueError):
            eng.resize_frames_yuv([frames[0], bad])
        with pytest.raises(ValueError):
            eng.detect_frames_yuv([bad], 0.3, 0.4)
    for bad in ([], (), y, [y]):
        with pytest.raises(ValueError):
            eng.resize_frames_yuv(bad)
    with pytest.raises(ValueError):
        yfv2.YuvFrame((y, uv), "p010")
    with pytest.raises(ValueError):
        yfv2.YuvFrame((y, uv), "nv12", "bt2020")

    out = _out(eng, 4)
    dst = torch.full((4, 352, 352, 3), 77, dtype=torch.uint8, device=dev)
    tout = eng.new_tiled_buffers(1)
    tout[0].fill_(SENTINEL)
    tout[2].fill_(-9)
    torch.cuda.synchronize()
    L = _lib.lib()
    h = eng._h
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    good = dict(y=y.data_ptr(), u=uv.data_ptr(), v=None, pitch_y=640, pitch_c=640, x0=0, y0=0, width=640, height=480, format=ym.NV12, colour=0)
    planar = dict(good, u=u.data_ptr(), v=u.data_ptr(), pitch_c=320, format=ym.I420)

    def table(*fs):
        arr = (_lib.FrameYuv * len(fs))()
        for i, f in enumerate(fs):
            for k, v in f.items():
                setattr(arr[i], k, v)
        return arr

    d0 = dst.data_ptr()
    cases = [   # (frames, B, dst, code, words of the message)
        (None, 1, d0, _lib.ERR_ARG, ["null pointer"]),
        (table(good), 0, d0, _lib.ERR_ARG, ["B < 1"]),
        (table(good), 1, None, _lib.ERR_ARG, ["null pointer"]),
        (table(good), 1, d0 + 2, _lib.ERR_ARG, ["4-byte aligned"]),
        (table(good, dict(good, y=None)), 2, d0, _lib.ERR_ARG, ["frame 1", "null y"]),
        (table(good, dict(good, u=None)), 2, d0, _lib.ERR_ARG, ["frame 1", "null u"]),
        (table(good, dict(planar, v=None)), 2, d0, _lib.ERR_ARG, ["frame 1", "null v"]),
        (table(dict(good, width=0)), 1, d0, _lib.ERR_ARG, ["frame 0", "height and width"]),
        (table(good, good, dict(good, height=-2)), 3, d0, _lib.ERR_ARG, ["frame 2", "height and width"]),
        (table(dict(good, x0=-1)), 1, d0, _lib.ERR_ARG, ["frame 0", "x0 and y0"]),
        (table(dict(good, y0=-1)), 1, d0, _lib.ERR_ARG, ["frame 0", "x0 and y0"]),
        (table(dict(good, pitch_y=639)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_y 639 < x0 + width"]),
        (table(dict(good, x0=1, width=640, pitch_y=640)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_y 640 < x0 + width"]),
        (table(dict(good, pitch_c=639)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_c 639 < 640"]),
        (table(dict(good, x0=1, width=639, pitch_c=639)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_c 639 < 640"]),
        (table(dict(planar, pitch_c=319)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_c 319 < 320"]),
        (table(dict(good, format=3)), 1, d0, _lib.ERR_ARG, ["frame 0", "unknown format 3"]),
        (table(dict(good, format=-1)), 1, d0, _lib.ERR_ARG, ["frame 0", "unknown format -1"]),
        (table(dict(good, colour=4)), 1, d0, _lib.ERR_ARG, ["frame 0", "unknown colour 4"]),
        (table(dict(good, width=40690, pitch_y=40690, pitch_c=40690)), 1, d0, _lib.ERR_ARG, ["frame 0", "wider than 40689"]),
        (table(dict(good, pitch_y=(1 << 40) + 1)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_y out of range"]),
        (table(dict(good, pitch_c=(1 << 40) + 1)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_c out of range"]),
        (table(dict(good, pitch_y=1 << 40, height=1 << 20)), 1, d0, _lib.ERR_ARG, ["frame 0", "pitch_y out of range"]),
        (table(dict(good, x0=0x7fffffff, pitch_y=1 << 33)), 1, d0, _lib.ERR_ARG, ["frame 0", "below 2^31"]),
        (table(*([good] * 5)), 5, d0, _lib.ERR_BATCH, ["max_batch=4"]),
    ]
    for arr, B, dptr, code, words in cases:
        rc = L.yfv2_resize_frames_yuv(h, arr, B, C.c_void_p(dptr) if dptr else None, st)
        msg = _lib.last_error(h)
        assert rc == code and all(w in msg for w in words) and "yfv2_resize_frames_yuv" in msg, (words, rc, msg)
        if dptr == d0:
            rc = L.yfv2_detect_frames_yuv(h, arr, B, 0.3, 0.4, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), st)
            msg = _lib.last_error(h)
            want_rc = _lib.ERR_BATCH if B < 1 else code      # check_call reports B outside [1, max_batch] as a batch error
            assert rc == want_rc and msg, (words, rc, msg)
            if B >= 1 and code == _lib.ERR_ARG:
                assert all(w in msg for w in words) and "yfv2_detect_frames_yuv" in msg, (words, rc, msg)
    assert L.yfv2_detect_frames_yuv(h, table(good), 1, 0.3, 0.4, None, _ptr(out[1]), _ptr(out[2]), st) == _lib.ERR_ARG
    assert L.yfv2_resize_frames_yuv(None, table(good), 1, C.c_void_p(d0), st) == _lib.ERR_ARG
    # the tiled entry point: its frames, its rectangles, and what a rectangle turns into
    tiles = lambda *ts: yfv2.tiling.tile_table(ts)
    tiled_cases = [
        (table(good), tiles((0, 0, 0, 352, 352)), 1, 300, None, ["null pointer"]),
        (table(dict(good, u=None)), tiles((0, 0, 0, 352, 352)), 1, 300, tout[0], ["frame 0", "null u"]),
        (table(dict(good, colour=9)), tiles((0, 0, 0, 352, 352)), 1, 300, tout[0], ["frame 0", "unknown colour"]),
        (table(good), tiles((0, 300, 0, 352, 352)), 1, 300, tout[0], ["tile 0", "inside its 640 x 480 frame"]),
        (table(good), tiles((0, 1, 1, 352, 0)), 1, 300, tout[0], ["tile 0", "at least one pixel"]),
        (table(good), tiles((1, 0, 0, 352, 352)), 1, 300, tout[0], ["frame 1 outside"]),
        (table(good), tiles((0, 0, 0, 352, 352)), 1, 0, tout[0], ["max_out"]),
    ]
    for farr, tarr, F, max_out, dets, words in tiled_cases:
        rc = L.yfv2_detect_tiled_yuv(h, farr, F, tarr, len(tarr), 0.3, 0.4, 0.4, 0, max_out, _ptr(dets) if dets is not None else None, _ptr(tout[1]), _ptr(tout[2]), st)
        msg = _lib.last_error(h)
        assert rc == _lib.ERR_ARG and all(w in msg for w in words) and "yfv2_detect_tiled_yuv" in msg, (words, rc, msg)
    five = tiles(*[(0, k, k, 352, 352) for k in range(5)])
    assert L.yfv2_detect_tiled_yuv(h, table(good), 1, five, 5, 0.3, 0.4, 0.4, 0, 300, _ptr(tout[0]), _ptr(tout[1]), _ptr(tout[2]), st) == _lib.ERR_BATCH
    torch.cuda.synchronize()
    assert bool((dst == 77).all()), "a failed call wrote its output"
    assert bool((out[0] == SENTINEL).all()) and bool((out[1] == -7).all()) and bool((out[2] == -9).all()), "a failed call wrote its output"
    assert bool((tout[0] == SENTINEL).all()) and bool((tout[2] == -9).all()), "a failed call wrote its output"
    # the engine is intact
    got = eng.detect_frames_yuv(frames[:2], 0.3, 0.4, out=_out(eng, 2))
    want = eng.detect_frames(bgr[:2], 0.3, 0.4, out=_out(eng, 2))
    assert torch.equal(got[2], want[2]) and torch.equal(got[1], want[1])
    _same(got[0], want[0], "after the errors")
