"""GPU tests of second-stage crops: Engine.crop_detections / Engine.crop_detections_yuv (include/yfv2.h yfv2_crop_detections_u8 /
_yuv).  Run with ``-m gpu`` on an MI355X.

The claims: crop_src, crop_rect, crop_offset and crop_skipped equal the rule's Python statement (tests/crops_model.py); every crop
equals the oracle's resize of its rectangle of the host frame, and resize_frames of the same views; nothing beyond slot
min(total, cap) is written; a YUV frame's crops equal those of the converted frame; bad arguments fail before anything is launched.
No tolerance appears anywhere: every comparison is exact.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import crops_model
import yuv_model
from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
S_PIX, S_SRC, S_RECT, S_OFF, S_SKIP = 0xA5, -7, -8, -9, -10      # the outputs are pre-filled with these


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
        (0.25, 0.25, 0.5, 0.5, 2),                               # a sub-pixel box
        (0.0, 0.0, float(min(w, 2)), float(min(h, 2)), 3),       # integer corners: 2 x 2 where the frame has them
        (0.0, 0.0, float(w), float(h), 3),                       # the whole frame
        (0.3 * w, 0.3 * h, 0.6 * w, 0.6 * h, 255),               # 255 is no class
        (0.3 * w, 0.3 * h, 0.6 * w, 0.6 * h, 1.5),               # ... nor is 1.5
        (0.3 * w, 0.3 * h, 0.6 * w, 0.6 * h, NAN),
        (0.45 * w, 0.4 * h, 0.9 * w, 0.95 * h, 7),
    ]
    return np.array([[x1, y1, x2, y2, 0.99 - 0.01 * i, c] for i, (x1, y1, x2, y2, c) in enumerate(boxes)], np.float32)


R_HAND = 32


@pytest.fixture(scope="module")
def scene(dev):
    """four frames - 240 x 320, 1 x 1, a crop view with an odd pitch at an odd address, 57 x 91 - their rows and counts"""
    rng = np.random.default_rng(11)
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
    return {"host": host, "frames": frames, "dets": dets, "count": count, "sizes": [f.shape[:2] for f in host]}


def _buffers(dev, B, cap, out_size):
    oh, ow = out_size
    return (torch.full((cap, oh, ow, 3), S_PIX, device=dev, dtype=torch.uint8), torch.full((cap,), S_SRC, device=dev, dtype=torch.int32),
            torch.full((cap, 4), S_RECT, device=dev, dtype=torch.int32), torch.full((B + 1,), S_OFF, device=dev, dtype=torch.int32),
            torch.full((B,), S_SKIP, device=dev, dtype=torch.int32))


def _run(eng, frames, dets, count, out_size, cap=None, yuv=False, **kw):
    """-> the five outputs as numpy arrays, written into sentinel-filled buffers of capacity cap"""
    dev = eng.device
    B, R = dets.shape[0], dets.shape[1]
    if cap is None:
        cap = B * min(R, kw.get("max_per_frame", 300))
    d = torch.from_numpy(np.ascontiguousarray(dets)).to(dev) if isinstance(dets, np.ndarray) else dets
    c = torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).to(dev) if isinstance(count, np.ndarray) else count
    fn = eng.crop_detections_yuv if yuv else eng.crop_detections
    out = fn(frames, d, c, out_size, cap=cap, out=_buffers(dev, B, cap, out_size), **kw)
    torch.cuda.synchronize(dev)
    return [t.cpu().numpy() for t in out]


def _untouched(got, live):
    crops, src, rect, _off, _skip = got
    assert (crops[live:] == S_PIX).all() and (src[live:] == S_SRC).all() and (rect[live:] == S_RECT).all(), "written beyond slot %d" % live


def _check_plan(got, want, cap):
    crops, src, rect, off, skip = got
    live = min(int(want["offset"][-1]), cap)
    assert off.tolist() == want["offset"].tolist()
    assert skip.tolist() == want["skipped"].tolist()
    assert src[:live].tolist() == want["src"].tolist() and rect[:live].tolist() == want["rect"].tolist()
    _untouched(got, live)
    return live


def _check_pixels(got, want, host, out_size):
    oh, ow = out_size
    for k, (b, (x0, y0, w, h)) in enumerate(zip(want["frame"].tolist(), want["rect"].tolist())):
        ref = oracle.resize_linear_u8(np.ascontiguousarray(host[b][y0:y0 + h, x0:x0 + w]), ow, oh)
        assert np.array_equal(got[0][k], ref), "crop %d (frame %d, rect %s) differs from the oracle's resize in %d bytes" % (
            k, b, (x0, y0, w, h), int((got[0][k] != ref).sum()))


def _views(frames, want):
    return [frames[b][y0:y0 + h, x0:x0 + w] for b, (x0, y0, w, h) in zip(want["frame"].tolist(), want["rect"].tolist())]


def test_plan_outputs_match_the_model(eng, scene):
    for kw in ({}, {"pad": 0.1}, {"pad": (16.0, 0.25)}, {"max_per_frame": 3}, {"classes": [0, 2, 3, 254]}, {"classes": []}):
        py, px = kw["pad"] if isinstance(kw.get("pad"), tuple) else (kw.get("pad", 0.0),) * 2
        want = crops_model.plan(scene["dets"], scene["count"], scene["sizes"], px, py, kw.get("max_per_frame", 300), kw.get("classes"))
        got = _run(eng, scene["frames"], scene["dets"], scene["count"], (8, 8), **kw)
        live = _check_plan(got, want, got[1].shape[0])
        assert (live > 0) == (kw.get("classes") != [])
        _check_pixels(got, want, scene["host"], (8, 8))
    want = crops_model.plan(scene["dets"], scene["count"], scene["sizes"])
    assert 0 in want["frame"] and 1 in want["frame"] and 2 in want["frame"] and 3 in want["frame"] and (want["skipped"] > 0).all()


@pytest.mark.parametrize("out_size", [(32, 32), (20, 12), (1, 4), (64, 64)])
def test_pixels_equal_the_oracle(eng, scene, out_size):
    want = crops_model.plan(scene["dets"], scene["count"], scene["sizes"])
    assert [2, 2] in [r[2:] for r in want["rect"].tolist()]                 # the up-scale from a 2 x 2 rectangle is among them
    got = _run(eng, scene["frames"], scene["dets"], scene["count"], out_size)
    _check_plan(got, want, got[1].shape[0])
    _check_pixels(got, want, scene["host"], out_size)


def test_pixels_equal_resize_frames_of_the_views(yfv2, dev, eng, scene):
    want = crops_model.plan(scene["dets"], scene["count"], scene["sizes"], 0.1, 0.1)
    views = _views(scene["frames"], want)
    for out_size, other in (((96, 64), yfv2.Engine(dev, 96, 64, max_batch=len(views), plan={})),
                            ((352, 352), yfv2.Engine(dev, 352, 352, max_batch=len(views), plan={}))):
        got = _run(eng, scene["frames"], scene["dets"], scene["count"], out_size, pad=0.1)
        live = _check_plan(got, want, got[1].shape[0])
        ref = other.resize_frames(views).cpu().numpy()
        assert live == len(views) and np.array_equal(got[0][:live], ref), out_size
        other.close()


def test_capacity_truncates_and_reports_the_total(eng, scene):
    full = _run(eng, scene["frames"], scene["dets"], scene["count"], (20, 12))
    total = int(full[3][-1])
    assert total > 3
    got = _run(eng, scene["frames"], scene["dets"], scene["count"], (20, 12), cap=3)
    assert got[3].tolist() == full[3].tolist() and got[4].tolist() == full[4].tolist()      # crop_offset[B] is still the total
    assert np.array_equal(got[0], full[0][:3]) and np.array_equal(got[1], full[1][:3]) and np.array_equal(got[2], full[2][:3])
    # slot 3 onward does not exist in these buffers; a larger buffer with the same cap shows they stay untouched
    dev = eng.device
    big = _buffers(dev, 4, 8, (20, 12))
    d, c = torch.from_numpy(scene["dets"]).to(dev), torch.from_numpy(scene["count"]).to(dev)
    rule = yfv2_rule(20, 12)
    arr, keep = eng._frame_table(scene["frames"])
    from yolo_fastestv2_amd import _lib
    _lib.check(_lib.lib().yfv2_crop_detections_u8(eng._h, arr, 4, d.data_ptr(), c.data_ptr(), R_HAND, C.byref(rule), *[t.data_ptr() for t in big], 3, None), eng._h)
    torch.cuda.synchronize(dev)
    host = [t.cpu().numpy() for t in big]
    assert np.array_equal(host[0][:3], full[0][:3])
    _untouched(host, 3)


def yfv2_rule(out_h, out_w, pad_x=0.0, pad_y=0.0, max_per_frame=300):
    from yolo_fastestv2_amd import _lib
    r = _lib.CropRule()
    r.out_h, r.out_w, r.pad_x, r.pad_y, r.max_per_frame = out_h, out_w, pad_x, pad_y, max_per_frame
    return r


def test_nothing_to_crop(eng, scene):
    got = _run(eng, scene["frames"], scene["dets"], np.zeros(4, np.int32), (32, 32))
    assert got[3].tolist() == [0] * 5 and got[4].tolist() == [0] * 4
    _untouched(got, 0)
    got = _run(eng, scene["frames"], scene["dets"], np.array([-1, 0, -300, 0], np.int32), (32, 32))
    assert got[3].tolist() == [0] * 5
    _untouched(got, 0)


def test_batch_independence(eng, scene):
    full = _run(eng, scene["frames"], scene["dets"], scene["count"], (20, 12), pad=0.1)
    off = full[3]
    for b in range(4):
        one = _run(eng, [scene["frames"][b]], scene["dets"][b:b + 1], scene["count"][b:b + 1], (20, 12), pad=0.1)
        n = int(one[3][1])
        assert n == off[b + 1] - off[b] and one[4][0] == full[4][b]
        assert np.array_equal(one[0][:n], full[0][off[b]:off[b + 1]]) and np.array_equal(one[2][:n], full[2][off[b]:off[b + 1]])
        assert np.array_equal(one[1][:n], full[1][off[b]:off[b + 1]] - b * R_HAND)
        _untouched(one, n)


def test_wide_frame(eng, dev):
    """a (2, 20000) frame: 120 KB of LDS for its two staged rows, the most of this file"""
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, (2, 20000, 3), dtype=np.uint8)
    dets = np.zeros((1, 4, 6), np.float32)
    dets[0, 0] = [0.0, 0.0, 20000.0, 2.0, 0.9, 0.0]          # spans the frame
    dets[0, 1] = [19990.5, 0.5, 20010.0, 1.5, 0.8, 0.0]      # its last columns
    count = np.array([2], np.int32)
    want = crops_model.plan(dets, count, [(2, 20000)])
    assert want["rect"].tolist() == [[0, 0, 20000, 2], [19990, 0, 10, 2]]
    got = _run(eng, [torch.from_numpy(host).to(dev)], dets, count, (4, 64))
    _check_plan(got, want, 4)
    _check_pixels(got, want, [host], (4, 64))


def _picture(images_u8, k, h, w, seed):
    hwc = np.ascontiguousarray(images_u8[k % len(images_u8)].transpose(1, 2, 0))
    rng = np.random.default_rng(seed)
    f = oracle.resize_linear_u8(hwc, w, h)
    return np.clip(f.astype(np.int16) + rng.integers(-3, 4, f.shape), 0, 255).astype(np.uint8)


def test_both_row_layouts_end_to_end(yfv2, dev, cfg, coco_weights, images_u8):
    """R = 300: detect_frames output on four pictures equals the host round trip it replaces (rows to the host, the rule in
    Python, torch views, a second engine's resize_frames); R = 50: detect_tiled(max_out=50) output"""
    det = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=8, plan={})
    det.load_state_dict(coco_weights)
    host = [_picture(images_u8, k, h, w, 40 + k) for k, (h, w) in enumerate(((240, 320), (200, 150), (352, 352), (123, 301)))]
    frames = [torch.from_numpy(f).to(dev) for f in host]
    dets, _idx, cnt = det.detect_frames(frames, 0.3, 0.4)
    got = _run(det, frames, dets, cnt, (64, 64), pad=0.1)
    want = crops_model.plan(dets.cpu().numpy(), cnt.cpu().numpy(), [f.shape[:2] for f in host], 0.1, 0.1)       # the round trip
    live = _check_plan(got, want, got[1].shape[0])
    assert live > 0 and dets.shape[1] == 300
    second = yfv2.Engine(dev, 64, 64, max_batch=live, plan={})
    assert np.array_equal(got[0][:live], second.resize_frames(_views(frames, want)).cpu().numpy())
    second.close()
    # R = 50: the tiled call's (F, max_out, 6) layout, boxes already in frame coordinates
    big = _picture(images_u8, 1, 500, 700, 77)
    tframes = [torch.from_numpy(big).to(dev)]
    tdets, _src, tcnt = det.detect_tiled(tframes, max_out=50)
    got = _run(det, tframes, tdets, tcnt, (32, 32))
    want = crops_model.plan(tdets.cpu().numpy(), tcnt.cpu().numpy(), [(500, 700)])
    live = _check_plan(got, want, got[1].shape[0])
    assert live > 0 and tdets.shape[1] == 50
    _check_pixels(got, want, [big], (32, 32))
    det.close()


@pytest.mark.parametrize("fmt,colour", [("nv12", "bt601"), ("nv21", "bt709_full"), ("i420", "bt601"), ("i420", "bt709_full")])
def test_yuv_equals_crops_of_the_converted_frame(yfv2, eng, dev, fmt, colour):
    code, ccode = yfv2.yuv.FORMATS[fmt], yfv2.yuv.COLOURS[colour]
    rng = np.random.default_rng(3 + code)
    rects = [(0, 0, 96, 64), (13, 7, 75, 51), (1, 1, 1, 1)]              # x0, y0, width, height: whole planes; odd origin, odd size; one pixel
    yframes, host = [], []
    for x0, y0, w, h in rects:
        planes = yuv_model.random_planes(rng, 64, 96, code)
        host.append(yuv_model.yuv_to_bgr(planes, code, ccode, x0, y0, w, h))
        yframes.append(yfv2.yuv.YuvFrame([torch.from_numpy(p).to(dev) for p in planes], fmt, colour, x0, y0, w, h))
    dets = np.full((3, R_HAND, 6), -3.0, np.float32)
    count = np.zeros(3, np.int32)
    for b, (_x0, _y0, w, h) in enumerate(rects):
        rows = _rows(h, w)
        dets[b, :len(rows)], count[b] = rows, len(rows)
    dets[1, :4, :4] += [0.5, 1.0, 1.5, 1.0]                              # odd and even crop origins inside the odd-origin frame
    want = crops_model.plan(dets, count, [(h, w) for _x, _y, w, h in rects], 0.1, 0.1)
    got = _run(eng, yframes, dets, count, (20, 12), yuv=True, pad=0.1)
    live = _check_plan(got, want, got[1].shape[0])
    assert live > 10 and {r[0] & 1 for r in want["rect"].tolist()} == {0, 1} and {r[1] & 1 for r in want["rect"].tolist()} == {0, 1}
    ref = _run(eng, [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in host], dets, count, (20, 12), pad=0.1)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    _check_pixels(got, want, host, (20, 12))


def test_argument_errors_launch_nothing(yfv2, eng, scene):
    from yolo_fastestv2_amd import _lib
    L, dev = _lib.lib(), eng.device
    d, c = torch.from_numpy(scene["dets"]).to(dev), torch.from_numpy(scene["count"]).to(dev)
    cap = 16
    bufs = _buffers(dev, 4, cap, (8, 8))
    arr, keep = eng._frame_table(scene["frames"])
    good = dict(h=eng._h, frames=arr, B=4, dets=d.data_ptr(), count=c.data_ptr(), R=R_HAND, rule=None, crops=bufs[0].data_ptr(), src=bufs[1].data_ptr(),
                rect=bufs[2].data_ptr(), offset=bufs[3].data_ptr(), skipped=bufs[4].data_ptr(), cap=cap)

    def call(rule_kw=None, classes=None, native=L.yfv2_crop_detections_u8, **over):
        a = dict(good, **over)
        r = yfv2_rule(8, 8)
        for k, v in (rule_kw or {}).items():
            setattr(r, k, v)
        if classes is not None:
            carr = (C.c_int32 * len(classes))(*classes)
            r.classes, r.n_classes = C.cast(carr, C.POINTER(C.c_int32)), len(classes)
        rule = C.byref(r) if a["rule"] is None else None
        return native(a["h"], a["frames"], a["B"], a["dets"], a["count"], a["R"], rule, a["crops"], a["src"], a["rect"], a["offset"], a["skipped"], a["cap"], None)

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
        ("null crops", dict(crops=None), E), ("null src", dict(src=None), E), ("null rect", dict(rect=None), E), ("null offset", dict(offset=None), E),
        ("B < 1", dict(B=0), E), ("R < 1", dict(R=0), E), ("R > 4096", dict(R=4097), E), ("cap < 1", dict(cap=0), E),
        ("cap * out_h", dict(cap=2 ** 28, rule_kw={"out_h": 8}), E), ("out_h < 1", dict(rule_kw={"out_h": 0}), E),
        ("out_w < 4", dict(rule_kw={"out_w": 0}), E), ("out_w % 4", dict(rule_kw={"out_w": 10}), E),
        ("crops misaligned", dict(crops=bufs[0].data_ptr() + 1), E),
        ("pad NaN", dict(rule_kw={"pad_x": NAN}), E), ("pad inf", dict(rule_kw={"pad_y": INF}), E), ("pad < 0", dict(rule_kw={"pad_x": -0.5}), E),
        ("pad > 16", dict(rule_kw={"pad_y": 16.5}), E), ("max_per_frame < 1", dict(rule_kw={"max_per_frame": 0}), E),
        ("class 255", dict(classes=[3, 255]), E), ("class -1", dict(classes=[-1]), E),
        ("frame height", dict(frames=frames_with(height=0)), E), ("frame data", dict(frames=frames_with(data=None)), E),
        ("frame pitch", dict(frames=frames_with(row_pitch=3)), E),
        ("frame too wide", dict(frames=frames_with(width=(160 * 1024 - 3 * 8) // 6 - 1, row_pitch=10 ** 6)), E),
        ("B > max_batch", dict(B=eng.max_batch + 1), _lib.ERR_BATCH),
    ]
    for what, kw, code in cases:
        rule_kw, classes = kw.pop("rule_kw", None), kw.pop("classes", None)
        assert call(rule_kw, classes, **kw) == code, what
        assert "yfv2_crop_detections_u8" in _lib.last_error(eng._h), what
    assert call(h=None) == E
    # the YUV entry point: the same checks of the call, its own of the frame
    yarr = (_lib.FrameYuv * 1)()
    assert call(native=L.yfv2_crop_detections_yuv, frames=yarr, B=1) == E and "yfv2_crop_detections_yuv: frame 0" in _lib.last_error(eng._h)
    assert call(native=L.yfv2_crop_detections_yuv, frames=yarr, B=1, rule_kw={"out_w": 6}) == E
    torch.cuda.synchronize(dev)
    host = [t.cpu().numpy() for t in bufs]
    _untouched(host, 0)
    assert (host[3] == S_OFF).all() and (host[4] == S_SKIP).all()
    # the widest frame that is allowed at out_w = 8 passes the check (27 300 pixels: (160 KiB - 24) / 6 - 2)
    assert call(frames=frames_with(width=(160 * 1024 - 3 * 8) // 6 - 2, height=1, row_pitch=10 ** 6), B=1, count=torch.zeros(1, dtype=torch.int32, device=dev).data_ptr()) == 0
    torch.cuda.synchronize(dev)
    # Engine-level validation, the way _tiled_out does it
    with pytest.raises(ValueError):
        eng.crop_detections(scene["frames"], d[:3], c, (8, 8))
    with pytest.raises(ValueError):
        eng.crop_detections(scene["frames"], d, c.to(torch.int64), (8, 8))
    with pytest.raises(ValueError):
        eng.crop_detections(scene["frames"], d, c, (8, 8), out=bufs[:4])
    with pytest.raises(yfv2.Yfv2Error):
        eng.crop_detections(scene["frames"], d, c, (8, 10))
