"""GPU tests of crops as network input: Engine.crop_tensors / Engine.crop_tensors_yuv (include/yfv2.h yfv2_crop_tensors_u8 / _yuv;
DESIGN.md 4.21).  Run with ``-m gpu`` on an MI355X.

The claims: the tensor equals the rule's numpy statement (tests/crop_tensors_model.py) bit for bit - fp32 and fp16, both plane
orders, stretch and letterbox; crop_src, crop_rect, crop_offset and crop_skipped equal what crop_detections returns; with
letterbox off the tensor is crop_detections' bytes put through the value rule; nothing beyond slot min(total, cap) is written; a YUV
frame's tensors equal those of the converted frame; bad arguments fail before anything is launched.  No tolerance appears
anywhere: every comparison is of raw bits.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import crop_tensors_model as model
import crops_model
import rows_model
import yuv_model

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
S_VAL, S_SRC, S_RECT, S_OFF, S_SKIP = -123.25, -7, -8, -9, -10      # the outputs are pre-filled with these (-123.25 is exact in fp16)
MEAN, STD, FILL = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), (114, 7, 201)      # one non-trivial triple of each
PLAIN = dict(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), fill=(0, 0, 0))
R_HAND = 32


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
def eng(yfv2, dev):
    """crops need no weights: an engine of the usual size with room for four frames"""
    return yfv2.Engine(dev, 352, 352, max_batch=4, plan={})


def _rows(h, w):
    """the adversarial rows of a h x w frame: x1, y1, x2, y2, conf, cls - conf-descending like a detector's"""
    boxes = [
        (0.31 * w, 0.22 * h, 0.74 * w, 0.81 * h, 0),             # inside
        (-0.2 * w, 0.1 * h, 0.4 * w, 0.5 * h, 1),                # crossing the left edge
        (0.7 * w, 0.1 * h, 1.3 * w, 0.5 * h, 2),                 # ... right
        (0.2 * w, -0.3 * h, 0.6 * w, 0.4 * h, 3),                # ... top
        (0.2 * w, 0.6 * h, 0.6 * w, 1.4 * h, 254),               # ... bottom
        (-0.5 * w - 3, 0.1 * h, -1.0, 0.5 * h, 0),               # outside, left
        (w + 0.5, 0.1 * h, 2.0 * w + 2, 0.5 * h, 0),             # ... right
        (0.1 * w, -0.5 * h - 3, 0.5 * w, -0.25, 0),              # ... above
        (0.1 * w, h + 1.0, 0.5 * w, 2.0 * h + 2, 0),             # ... below
        (0.5 * w, 0.1 * h, 0.5 * w, 0.9 * h, 1),                 # x1 == x2
        (0.6 * w, 0.1 * h, 0.4 * w, 0.9 * h, 1),                 # inverted
        (NAN, 0.1 * h, 0.5 * w, 0.9 * h, 1),
        (0.1 * w, 0.1 * h, INF, 0.9 * h, 1),
        (-INF, -INF, INF, INF, 1),
        (-1e30, -1e30, 1e30, 1e30, 2),                           # finite: the whole frame
        (0.25, 0.25, 0.5, 0.5, 2),                               # a sub-pixel box: a 1 x 1 rectangle
        (0.0, 0.0, float(min(w, 2)), float(min(h, 2)), 3),       # integer corners: 2 x 2 where the frame has them
        (0.0, 0.0, float(w), float(h), 3),                       # the whole frame
        (0.3 * w, 0.3 * h, 0.6 * w, 0.6 * h, 255),               # 255 is no class
        (0.3 * w, 0.3 * h, 0.6 * w, 0.6 * h, 1.5),               # ... nor is 1.5
        (0.3 * w, 0.3 * h, 0.6 * w, 0.6 * h, NAN),
        (0.45 * w, 0.4 * h, 0.9 * w, 0.95 * h, 7),
        (0.05 * w, 0.5 * h, 0.95 * w, 0.5 * h + 0.5, 7),         # a sliver: wide, one or two rows tall
        (0.5 * w, 0.05 * h, 0.5 * w + 0.5, 0.95 * h, 7),         # ... and its transpose
    ]
    return np.array([[x1, y1, x2, y2, 0.99 - 0.01 * i, c] for i, (x1, y1, x2, y2, c) in enumerate(boxes)], np.float32)


@pytest.fixture(scope="module")
def scene(dev):
    """four frames - 240 x 320, 1 x 1, a view with an odd pitch at an odd address, 57 x 91 - their rows and counts"""
    rng = np.random.default_rng(21)
    host = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8), rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)]
    base = rng.integers(0, 256, (100, 151, 3), dtype=np.uint8)           # pitch 453
    host.append(np.ascontiguousarray(base[7:90, 6:141]))
    host.append(rng.integers(0, 256, (57, 91, 3), dtype=np.uint8))
    base_t = torch.from_numpy(base).to(dev)
    frames = [torch.from_numpy(host[0]).to(dev), torch.from_numpy(host[1]).to(dev), base_t[7:90, 6:141], torch.from_numpy(host[3]).to(dev)]
    assert frames[2].stride(0) == 453 and frames[2].data_ptr() % 2 == 1
    dets = np.full((4, R_HAND, 6), -3.0, np.float32)
    count = np.zeros(4, np.int32)
    for b, f in enumerate(host):
        rows = _rows(f.shape[0], f.shape[1])
        dets[b, :len(rows)] = rows
        count[b] = len(rows)
    count[3] = 40                                                        # count > R: every row of the frame, the filler included
    dets[3, len(rows):] = [5.0, 5.0, 20.5, 30.5, 0.1, 9.0]
    sizes = [f.shape[:2] for f in host]
    return {"host": host, "frames": frames, "dets": dets, "count": count, "sizes": sizes, "plan": crops_model.plan(dets, count, sizes), "bytes": {}}


def _byte_images(scene, out_size, lb, fill):
    """the scene's byte images at (out_size, letterbox, fill): computed once, shared by the dtype and plane-order cases"""
    key = (out_size, lb, fill)
    if key not in scene["bytes"]:
        want = scene["plan"]
        imgs = [model.byte_image(scene["host"][b][y0:y0 + h, x0:x0 + w], out_size[0], out_size[1], lb, fill)
                for b, (x0, y0, w, h) in zip(want["frame"].tolist(), want["rect"].tolist())]
        scene["bytes"][key] = np.stack(imgs)
        scene["bytes"][key].setflags(write=False)
    return scene["bytes"][key]


def _buffers(dev, B, cap, out_size, dtype=torch.float32):
    oh, ow = out_size
    return (torch.full((cap, 3, oh, ow), S_VAL, device=dev, dtype=dtype), torch.full((cap,), S_SRC, device=dev, dtype=torch.int32),
            torch.full((cap, 4), S_RECT, device=dev, dtype=torch.int32), torch.full((B + 1,), S_OFF, device=dev, dtype=torch.int32),
            torch.full((B,), S_SKIP, device=dev, dtype=torch.int32))


def _dev(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev) if isinstance(a, np.ndarray) else a


def _run(eng, frames, dets, count, out_size, cap=None, yuv=False, dtype=torch.float32, **kw):
    """-> the five outputs as numpy arrays, written into sentinel-filled buffers of capacity cap"""
    dev = eng.device
    B, R = dets.shape[0], dets.shape[1]
    if cap is None:
        cap = B * min(R, kw.get("max_per_frame", 300))
    fn = eng.crop_tensors_yuv if yuv else eng.crop_tensors
    out = fn(frames, _dev(dets, dev), _dev(count, dev, np.int32), out_size, dtype=dtype, cap=cap, out=_buffers(dev, B, cap, out_size, dtype), **kw)
    torch.cuda.synchronize(dev)
    return [t.cpu().numpy() for t in out]


def _run_u8(eng, frames, dets, count, out_size, cap=None, **kw):
    """crop_detections on the same arguments"""
    dev = eng.device
    B, R = dets.shape[0], dets.shape[1]
    if cap is None:
        cap = B * min(R, kw.get("max_per_frame", 300))
    out = eng.crop_detections(frames, _dev(dets, dev), _dev(count, dev, np.int32), out_size, cap=cap, **kw)
    torch.cuda.synchronize(dev)
    return [t.cpu().numpy() for t in out]


def _same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = model.bits(got), model.bits(want)
    assert np.array_equal(g, w), "%s: %d of %d values differ in their bits" % (what, int((g != w).sum()), g.size)


def _untouched(got, live):
    t, src, rect, _off, _skip = got
    sentinel = model.bits(np.full((), S_VAL, t.dtype))
    assert (model.bits(t[live:]) == sentinel).all() and (src[live:] == S_SRC).all() and (rect[live:] == S_RECT).all(), "written beyond slot %d" % live


def _check_plan(got, want, cap):
    _t, src, rect, off, skip = got
    live = min(int(want["offset"][-1]), cap)
    assert off.tolist() == want["offset"].tolist()
    assert skip.tolist() == want["skipped"].tolist()
    assert src[:live].tolist() == want["src"].tolist()[:live] and rect[:live].tolist() == want["rect"].tolist()[:live]
    _untouched(got, live)
    return live


@pytest.mark.parametrize("lb", [False, True])
@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("out_size", [(32, 32), (20, 12), (1, 4), (64, 64)])
def test_values_equal_the_model(eng, scene, out_size, dtype, rgb, lb):
    want = scene["plan"]
    rects = [r[2:] for r in want["rect"].tolist()]
    assert [2, 2] in rects and [1, 1] in rects                       # the up-scales from a 2 x 2 and a 1 x 1 rectangle are among them
    half = dtype == torch.float16
    got = _run(eng, scene["frames"], scene["dets"], scene["count"], out_size, dtype=dtype, mean=MEAN, std=STD, rgb=rgb, letterbox=lb, fill=FILL)
    live = _check_plan(got, want, got[1].shape[0])
    assert live == len(rects) > 20
    ref = model.from_bytes(_byte_images(scene, out_size, lb, FILL), MEAN, STD, rgb, half)
    _same_bits(got[0][:live], ref, "%s %s rgb=%d letterbox=%d" % (out_size, dtype, rgb, lb))


def test_plan_outputs_equal_crop_detections(eng, scene):
    for kw in ({}, {"pad": 0.1}, {"pad": (16.0, 0.25)}, {"max_per_frame": 3}, {"classes": [0, 2, 3, 254]}, {"classes": []}):
        ref = _run_u8(eng, scene["frames"], scene["dets"], scene["count"], (8, 8), **kw)
        for lb, dtype in ((False, torch.float32), (True, torch.float16)):
            got = _run(eng, scene["frames"], scene["dets"], scene["count"], (8, 8), dtype=dtype, letterbox=lb, **kw)
            live = min(int(ref[3][-1]), got[1].shape[0])
            assert (live > 0) == (kw.get("classes") != [])
            assert np.array_equal(got[3], ref[3]) and np.array_equal(got[4], ref[4]), kw
            assert np.array_equal(got[1][:live], ref[1][:live]) and np.array_equal(got[2][:live], ref[2][:live]), kw
            _untouched(got, live)
        py, px = kw["pad"] if isinstance(kw.get("pad"), tuple) else (kw.get("pad", 0.0),) * 2
        want = crops_model.plan(scene["dets"], scene["count"], scene["sizes"], px, py, kw.get("max_per_frame", 300), kw.get("classes"))
        _check_plan(got, want, got[1].shape[0])


@pytest.mark.parametrize("out_size", [(32, 32), (20, 12)])
def test_stretch_is_crop_detections_put_through_the_value_rule(eng, scene, out_size):
    """ties the new launch to the existing one, not only to the oracle"""
    u8 = _run_u8(eng, scene["frames"], scene["dets"], scene["count"], out_size, pad=0.1)
    live = int(u8[3][-1])
    assert 0 < live <= u8[1].shape[0]
    got = _run(eng, scene["frames"], scene["dets"], scene["count"], out_size, pad=0.1)
    assert np.array_equal(got[1][:live], u8[1][:live]) and np.array_equal(got[2][:live], u8[2][:live])
    _same_bits(got[0][:live], model.from_bytes(u8[0][:live], (0, 0, 0), (1, 1, 1), False, False), "plain / 255")
    got = _run(eng, scene["frames"], scene["dets"], scene["count"], out_size, pad=0.1, mean=MEAN, std=STD)
    _same_bits(got[0][:live], model.from_bytes(u8[0][:live], MEAN, STD, False, False), "normalised")
    _untouched(got, live)


# boxes of a 100 x 120 frame and the (ox0, oy0, iw, ih) each must get in a (32, 32) letterbox
LETTERBOX_CASES = [
    ((10.0, 20.0, 90.0, 30.0), (0, 14, 32, 4)),          # 80 x 10: wider than the output's aspect, margins above and below
    ((20.0, 10.0, 30.0, 90.0), (14, 0, 4, 32)),          # 10 x 80: taller, margins left and right
    ((30.0, 30.0, 70.0, 70.0), (0, 0, 32, 32)),          # 40 x 40: the output's aspect, no margin
    ((5.2, 5.2, 5.6, 5.6), (0, 0, 32, 32)),              # a 1 x 1 rectangle
    ((0.0, 40.0, 120.0, 41.0), (0, 15, 32, 1)),          # 120 x 1: the inner height is 1 (0.27 rounds to 0, the rule's max(1, .))
    ((40.0, 0.0, 41.0, 100.0), (15, 0, 1, 32)),          # ... and the inner width
    ((10.0, 10.0, 31.0, 42.0), (5, 0, 21, 32)),          # 21 x 32: an odd margin, 5 on the left and 6 on the right
    ((10.0, 10.0, 42.0, 31.0), (0, 5, 32, 21)),
]


@pytest.mark.parametrize("dtype,out_size", [(torch.float32, (32, 32)), (torch.float16, (32, 32)), (torch.float16, (20, 12)), (torch.float32, (20, 12))])
def test_letterbox_shapes_and_fill(eng, dev, dtype, out_size):
    rng = np.random.default_rng(8)
    host = rng.integers(0, 256, (100, 120, 3), dtype=np.uint8)
    dets = np.zeros((1, 16, 6), np.float32)
    for i, (box, _inner) in enumerate(LETTERBOX_CASES):
        dets[0, i] = list(box) + [0.9 - 0.01 * i, 0.0]
    count = np.array([len(LETTERBOX_CASES)], np.int32)
    want = crops_model.plan(dets, count, [(100, 120)])
    assert len(want["rect"]) == len(LETTERBOX_CASES)
    half = dtype == torch.float16
    H, W = out_size
    for rgb in (False, True):
        got = _run(eng, [torch.from_numpy(host).to(dev)], dets, count, out_size, dtype=dtype, mean=MEAN, std=STD, rgb=rgb, letterbox=True, fill=FILL)
        live = _check_plan(got, want, got[1].shape[0])
        ref = model.tensors([host], want, out_size, MEAN, STD, rgb, True, FILL, half)
        _same_bits(got[0][:live], ref, "letterbox %s %s rgb=%d" % (out_size, dtype, rgb))
        # what lies outside the inner rectangle holds exactly the rule's value of fill, plane by plane
        fill_planes = model.from_bytes(np.asarray(FILL, np.uint8).reshape(1, 1, 3), MEAN, STD, rgb, half).reshape(3)
        margins = 0
        for k, ((x0, y0, w, h), (_box, inner32)) in enumerate(zip(want["rect"].tolist(), LETTERBOX_CASES)):
            ox0, oy0, iw, ih = model.letterbox(w, h, H, W, True)
            if out_size == (32, 32):
                assert (ox0, oy0, iw, ih) == inner32, (k, (w, h))
            outside = np.ones((H, W), bool)
            outside[oy0:oy0 + ih, ox0:ox0 + iw] = False
            margins += int(outside.sum())
            for c in range(3):
                assert (model.bits(got[0][k, c][outside]) == model.bits(fill_planes[c:c + 1])).all(), (k, c)
        assert margins > 0


@pytest.mark.parametrize("colour", ["bt601", "bt709_full"])
def test_yuv_equals_tensors_of_the_converted_frame(yfv2, eng, dev, colour):
    fmt = "i420"
    code, ccode = yfv2.yuv.FORMATS[fmt], yfv2.yuv.COLOURS[colour]
    rng = np.random.default_rng(3 + ccode)
    rects = [(0, 0, 96, 64), (13, 7, 75, 51), (1, 1, 1, 1)]              # x0, y0, width, height: whole planes; odd origin, odd size; one pixel
    yframes, host = [], []
    for x0, y0, w, h in rects:
        planes = yuv_model.random_planes(rng, 64, 96, code)
        host.append(np.ascontiguousarray(yuv_model.yuv_to_bgr(planes, code, ccode, x0, y0, w, h)))
        yframes.append(yfv2.yuv.YuvFrame([torch.from_numpy(p).to(dev) for p in planes], fmt, colour, x0, y0, w, h))
    dets = np.full((3, R_HAND, 6), -3.0, np.float32)
    count = np.zeros(3, np.int32)
    for b, (_x0, _y0, w, h) in enumerate(rects):
        rows = _rows(h, w)
        dets[b, :len(rows)], count[b] = rows, len(rows)
    dets[1, :4, :4] += [0.5, 1.0, 1.5, 1.0]                              # odd and even crop origins inside the odd-origin frame
    want = crops_model.plan(dets, count, [(h, w) for _x, _y, w, h in rects], 0.1, 0.1)
    bgr = [torch.from_numpy(f).to(dev) for f in host]
    for dtype, rgb, lb in ((torch.float32, True, True), (torch.float16, False, False), (torch.float16, True, True)):
        kw = dict(dtype=dtype, pad=0.1, mean=MEAN, std=STD, rgb=rgb, letterbox=lb, fill=FILL)
        got = _run(eng, yframes, dets, count, (20, 12), yuv=True, **kw)
        live = _check_plan(got, want, got[1].shape[0])
        assert live > 10 and {r[0] & 1 for r in want["rect"].tolist()} == {0, 1} and {r[1] & 1 for r in want["rect"].tolist()} == {0, 1}
        ref = _run(eng, bgr, dets, count, (20, 12), **kw)
        for g, r in zip(got[1:], ref[1:]):
            assert np.array_equal(g, r)
        _same_bits(got[0], ref[0], "yuv against converted, %s" % dtype)
        _same_bits(got[0][:live], model.tensors(host, want, (20, 12), MEAN, STD, rgb, lb, FILL, dtype == torch.float16), "yuv against the model")


def test_capacity_truncates_and_reports_the_total(eng, scene):
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD, letterbox=True, fill=FILL)
    full = _run(eng, scene["frames"], scene["dets"], scene["count"], (20, 12), **kw)
    total = int(full[3][-1])
    assert total > 3
    got = _run(eng, scene["frames"], scene["dets"], scene["count"], (20, 12), cap=3, **kw)
    assert got[3].tolist() == full[3].tolist() and got[4].tolist() == full[4].tolist()      # crop_offset[B] is still the total
    _same_bits(got[0], full[0][:3])
    assert np.array_equal(got[1], full[1][:3]) and np.array_equal(got[2], full[2][:3])
    # slot 3 onward does not exist in these buffers; larger buffers with the same cap show that they stay untouched
    from yolo_fastestv2_amd import _lib
    dev = eng.device
    big = _buffers(dev, 4, 8, (20, 12), torch.float16)
    d, c = torch.from_numpy(scene["dets"]).to(dev), torch.from_numpy(scene["count"]).to(dev)
    arr, keep = eng._frame_table(scene["frames"])
    tz, _dt = eng._crop_tensor("test", MEAN, STD, False, True, FILL, torch.float16)
    _lib.check(_lib.lib().yfv2_crop_tensors_u8(eng._h, arr, 4, d.data_ptr(), c.data_ptr(), R_HAND, C.byref(_rule(20, 12)), C.byref(tz),
                                               *[t.data_ptr() for t in big], 3, None), eng._h)
    torch.cuda.synchronize(dev)
    host = [t.cpu().numpy() for t in big]
    _same_bits(host[0][:3], full[0][:3])
    _untouched(host, 3)


def _rule(out_h, out_w, pad_x=0.0, pad_y=0.0, max_per_frame=300):
    from yolo_fastestv2_amd import _lib
    r = _lib.CropRule()
    r.out_h, r.out_w, r.pad_x, r.pad_y, r.max_per_frame = out_h, out_w, pad_x, pad_y, max_per_frame
    return r


def test_nothing_to_crop(eng, scene):
    for count in (np.zeros(4, np.int32), np.array([-1, 0, -300, 0], np.int32)):
        got = _run(eng, scene["frames"], scene["dets"], count, (32, 32), letterbox=True, fill=FILL)
        assert got[3].tolist() == [0] * 5 and got[4].tolist() == [0] * 4
        _untouched(got, 0)


def test_batch_independence(eng, scene):
    kw = dict(pad=0.1, mean=MEAN, std=STD, rgb=True, letterbox=True, fill=FILL)
    full = _run(eng, scene["frames"], scene["dets"], scene["count"], (20, 12), **kw)
    off = full[3]
    for b in range(4):
        one = _run(eng, [scene["frames"][b]], scene["dets"][b:b + 1], scene["count"][b:b + 1], (20, 12), **kw)
        n = int(one[3][1])
        assert n == off[b + 1] - off[b] and one[4][0] == full[4][b]
        _same_bits(one[0][:n], full[0][off[b]:off[b + 1]], "frame %d" % b)
        assert np.array_equal(one[2][:n], full[2][off[b]:off[b + 1]]) and np.array_equal(one[1][:n], full[1][off[b]:off[b + 1]] - b * R_HAND)
        _untouched(one, n)


def _limit(out_w, half):
    """the width limit of the B, G, R entry point (include/yfv2.h)"""
    return rows_model.max_width(rows_model.TENSOR_F16 if half else rows_model.TENSOR_F32, rows_model.BGR, out_w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_widest_frame(eng, dev, dtype):
    """one frame at the width limit, two rows tall, one crop that spans it: the most LDS a workgroup of these launches takes"""
    half = dtype == torch.float16
    wmax = _limit(64, half)
    assert wmax == (27172 if not half else 27236)
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, (2, wmax, 3), dtype=np.uint8)
    dets = np.zeros((1, 4, 6), np.float32)
    dets[0, 0] = [0.0, 0.0, float(wmax), 2.0, 0.9, 0.0]
    count = np.array([1], np.int32)
    want = crops_model.plan(dets, count, [(2, wmax)])
    assert want["rect"].tolist() == [[0, 0, wmax, 2]]
    got = _run(eng, [torch.from_numpy(host).to(dev)], dets, count, (4, 64), dtype=dtype, mean=MEAN, std=STD)
    _check_plan(got, want, 4)
    _same_bits(got[0][:1], model.tensors([host], want, (4, 64), MEAN, STD, False, False, (0, 0, 0), half))


def _picture(images_u8, k, h, w, seed):
    from oracle import yfv2_oracle as oracle
    hwc = np.ascontiguousarray(images_u8[k % len(images_u8)].transpose(1, 2, 0))
    rng = np.random.default_rng(seed)
    f = oracle.resize_linear_u8(hwc, w, h)
    return np.clip(f.astype(np.int16) + rng.integers(-3, 4, f.shape), 0, 255).astype(np.uint8)


def test_cascade_end_to_end(yfv2, dev, cfg, coco_weights, images_u8):
    """detect_frames, track_update(fresh=True) until the tracks are confirmed, crop_tensors of the fresh rows: the tensor equals
    the model on the rows copied to the host"""
    det = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=4, plan={})
    det.load_state_dict(coco_weights)
    host = [_picture(images_u8, k, h, w, 60 + k) for k, (h, w) in enumerate(((240, 320), (200, 150)))]
    frames = [torch.from_numpy(f).to(dev) for f in host]
    confirm = 2
    tracker = yfv2.Tracker(det, len(frames), max_tracks=64, confirm_hits=confirm)
    for _ in range(confirm):                                             # the same frames again: every track is confirmed in the last pass
        dets, _idx, cnt = det.detect_frames(frames, 0.3, 0.4)
        _id, _hits, fresh_dets, _fresh_src, fresh_count = tracker.update(dets, cnt, fresh=True)
    kw = dict(pad=0.1, mean=MEAN, std=STD, rgb=True, letterbox=True, fill=FILL)
    got = _run(det, frames, fresh_dets, fresh_count, (64, 64), dtype=torch.float16, **kw)
    want = crops_model.plan(fresh_dets.cpu().numpy(), fresh_count.cpu().numpy(), [f.shape[:2] for f in host], 0.1, 0.1)
    live = _check_plan(got, want, got[1].shape[0])
    assert live > 0 and int(fresh_count.sum()) > 0 and fresh_dets.shape[1] == 300
    _same_bits(got[0][:live], model.tensors(host, want, (64, 64), MEAN, STD, True, True, FILL, True), "cascade")
    det.close()


def test_argument_errors_launch_nothing(yfv2, eng, scene):
    from yolo_fastestv2_amd import _lib
    L, dev = _lib.lib(), eng.device
    d, c = torch.from_numpy(scene["dets"]).to(dev), torch.from_numpy(scene["count"]).to(dev)
    cap = 16
    bufs = _buffers(dev, 4, cap, (8, 8))
    arr, keep = eng._frame_table(scene["frames"])
    good = dict(h=eng._h, frames=arr, B=4, dets=d.data_ptr(), count=c.data_ptr(), R=R_HAND, rule=None, tensor=None, out=bufs[0].data_ptr(),
                src=bufs[1].data_ptr(), rect=bufs[2].data_ptr(), offset=bufs[3].data_ptr(), skipped=bufs[4].data_ptr(), cap=cap)

    def call(rule_kw=None, tensor_kw=None, native=L.yfv2_crop_tensors_u8, **over):
        a = dict(good, **over)
        r = _rule(8, 8)
        for k, v in (rule_kw or {}).items():
            setattr(r, k, v)
        t, _dt = eng._crop_tensor("test", MEAN, STD, False, True, FILL, torch.float32)
        for k, v in (tensor_kw or {}).items():
            if isinstance(v, tuple):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        rule = C.byref(r) if a["rule"] is None else None
        tensor = C.byref(t) if a["tensor"] is None else None
        return native(a["h"], a["frames"], a["B"], a["dets"], a["count"], a["R"], rule, tensor, a["out"], a["src"], a["rect"], a["offset"], a["skipped"],
                      a["cap"], None)

    def frames_with(**kw):
        bad = (_lib.Frame * 4)()
        for i in range(4):
            bad[i].data, bad[i].height, bad[i].width, bad[i].row_pitch = arr[i].data, arr[i].height, arr[i].width, arr[i].row_pitch
        for k, v in kw.items():
            setattr(bad[0], k, v)
        return bad

    E = _lib.ERR_ARG
    cases = [
        ("null frames", dict(frames=None), E), ("null dets", dict(dets=None), E), ("null count", dict(count=None), E), ("null rule", dict(rule=False), E),
        ("null tensor", dict(tensor=False), E), ("null out", dict(out=None), E), ("null src", dict(src=None), E), ("null rect", dict(rect=None), E),
        ("null offset", dict(offset=None), E), ("B < 1", dict(B=0), E), ("R < 1", dict(R=0), E), ("R > 4096", dict(R=4097), E), ("cap < 1", dict(cap=0), E),
        ("out_h < 1", dict(rule_kw={"out_h": 0}), E), ("out_w < 4", dict(rule_kw={"out_w": 0}), E), ("out_w % 4", dict(rule_kw={"out_w": 10}), E),
        ("pad NaN", dict(rule_kw={"pad_x": NAN}), E), ("max_per_frame < 1", dict(rule_kw={"max_per_frame": 0}), E),
        ("dtype 2", dict(tensor_kw={"dtype": 2}), E), ("dtype -1", dict(tensor_kw={"dtype": -1}), E),
        ("rgb 2", dict(tensor_kw={"rgb": 2}), E), ("letterbox -1", dict(tensor_kw={"letterbox": -1}), E),
        ("std 0", dict(tensor_kw={"std": (1, 0.0)}), E), ("std < 0", dict(tensor_kw={"std": (0, -0.25)}), E), ("std NaN", dict(tensor_kw={"std": (2, NAN)}), E),
        ("std inf", dict(tensor_kw={"std": (2, INF)}), E), ("mean inf", dict(tensor_kw={"mean": (0, INF)}), E), ("mean NaN", dict(tensor_kw={"mean": (1, NAN)}), E),
        ("out misaligned by 4", dict(out=bufs[0].data_ptr() + 4), E), ("out misaligned by 8", dict(out=bufs[0].data_ptr() + 8), E),
        ("frame height", dict(frames=frames_with(height=0)), E), ("frame data", dict(frames=frames_with(data=None)), E),
        ("frame too wide, fp32", dict(frames=frames_with(width=_limit(8, False) + 1, row_pitch=10 ** 6)), E),
        ("frame too wide, fp16", dict(frames=frames_with(width=_limit(8, True) + 1, row_pitch=10 ** 6), tensor_kw={"dtype": 1}), E),
        ("B > max_batch", dict(B=eng.max_batch + 1), _lib.ERR_BATCH),
    ]
    for what, kw, code in cases:
        rule_kw, tensor_kw = kw.pop("rule_kw", None), kw.pop("tensor_kw", None)
        assert call(rule_kw, tensor_kw, **kw) == code, what
        assert "yfv2_crop_tensors_u8" in _lib.last_error(eng._h), what
    assert call(h=None) == E
    # the YUV entry point: the same checks of the call, its own of the frame
    yarr = (_lib.FrameYuv * 1)()
    assert call(native=L.yfv2_crop_tensors_yuv, frames=yarr, B=1) == E and "yfv2_crop_tensors_yuv: frame 0" in _lib.last_error(eng._h)
    assert call(native=L.yfv2_crop_tensors_yuv, frames=yarr, B=1, tensor_kw={"std": (0, 0.0)}) == E and "std" in _lib.last_error(eng._h)
    torch.cuda.synchronize(dev)
    host = [t.cpu().numpy() for t in bufs]
    _untouched(host, 0)
    assert (host[3] == S_OFF).all() and (host[4] == S_SKIP).all()
    # the widest frame that is allowed at out_w = 8 passes the check, in fp16 a little wider than in fp32
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    assert _limit(8, True) > _limit(8, False)
    assert call(frames=frames_with(width=_limit(8, False), height=1, row_pitch=10 ** 6), B=1, count=zero.data_ptr()) == 0
    assert call(frames=frames_with(width=_limit(8, True), height=1, row_pitch=10 ** 6), B=1, count=zero.data_ptr(), tensor_kw={"dtype": 1}) == 0
    torch.cuda.synchronize(dev)
    # Engine-level validation
    with pytest.raises(ValueError):
        eng.crop_tensors(scene["frames"], d, c, (8, 8), dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        eng.crop_tensors(scene["frames"], d, c, (8, 8), mean=(0.5, 0.5))
    with pytest.raises(ValueError):
        eng.crop_tensors(scene["frames"], d, c, (8, 8), fill=(0, 0, 256))
    with pytest.raises(ValueError):
        eng.crop_tensors(scene["frames"], d, c, (8, 8), dtype=torch.float16, out=bufs)       # fp32 buffers for an fp16 call
    with pytest.raises(yfv2.Yfv2Error):
        eng.crop_tensors(scene["frames"], d, c, (8, 10))
    with pytest.raises(yfv2.Yfv2Error):
        eng.crop_tensors(scene["frames"], d, c, (8, 8), std=(1.0, 0.0, 1.0))
