"""CPU-only checks of second-stage crops (include/yfv2.h yfv2_crop_rect, yfv2_crop_detections_u8 / _yuv):
  * yfv2_crop_rect - the host entry point that calls the very function the plan kernel calls - equals the rule restated in
    tests/crops_model.py bit for bit, on seeded boxes and on the hand-written cases, and every rectangle has the properties a
    caller relies on
  * the model's selection, offsets and src numbering on a hand-computed case
  * argument errors of yfv2_crop_rect, which needs no device
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import crops_model

INF, NAN = float("inf"), float("nan")


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _c_rect(m, box, h, w, px=0.0, py=0.0):
    """-> (X0, Y0, width, height), None when skipped; rect is pre-filled so that an untouched one shows"""
    b = (C.c_float * 4)(*[float(v) for v in box])
    r = (C.c_int32 * 4)(-77, -77, -77, -77)
    rc = m.lib().yfv2_crop_rect(b, h, w, px, py, r)
    assert rc in (0, 1), (rc, m.last_error())
    if rc == 0:
        assert list(r) == [-77] * 4          # a skipped box writes nothing
        return None
    return tuple(r)


# (box, frame (h, w), expected rect at pad 0 or None)
HAND = [
    ((10.5, 20.25, 50.5, 60.75), (100, 200), (10, 20, 41, 41)),          # inside the frame
    ((-5.0, 10.0, 20.0, 30.0), (100, 200), (0, 10, 20, 20)),             # crossing the left edge
    ((190.0, 10.0, 230.0, 30.0), (100, 200), (190, 10, 10, 20)),         # ... the right edge
    ((10.0, -8.5, 20.0, 30.0), (100, 200), (10, 0, 10, 30)),             # ... the top edge
    ((10.0, 90.0, 20.0, 130.5), (100, 200), (10, 90, 10, 10)),           # ... the bottom edge
    ((-30.0, 10.0, -1.0, 30.0), (100, 200), None),                       # fully outside, left
    ((-30.0, 10.0, 0.0, 30.0), (100, 200), None),                        # ... touching the left edge from outside: cx2 > cx1 fails
    ((200.0, 10.0, 230.0, 30.0), (100, 200), None),                      # ... right (starts on the edge)
    ((10.0, -30.0, 20.0, -0.5), (100, 200), None),                       # ... above
    ((10.0, 100.0, 20.0, 130.0), (100, 200), None),                      # ... below
    ((10.0, 10.0, 10.0, 30.0), (100, 200), None),                        # x1 == x2
    ((20.0, 10.0, 10.0, 30.0), (100, 200), None),                        # inverted in x
    ((10.0, 30.0, 20.0, 10.0), (100, 200), None),                        # inverted in y
    ((NAN, 10.0, 20.0, 30.0), (100, 200), None),
    ((10.0, NAN, 20.0, 30.0), (100, 200), None),
    ((10.0, 10.0, INF, 30.0), (100, 200), None),
    ((-INF, 10.0, 20.0, 30.0), (100, 200), None),
    ((10.0, -INF, 20.0, INF), (100, 200), None),
    ((-1e30, -1e30, 1e30, 1e30), (100, 200), (0, 0, 200, 100)),          # 1e30: finite, clipped to the whole frame
    ((1e30, 10.0, 2e30, 30.0), (100, 200), None),
    ((10.25, 10.25, 10.5, 10.5), (100, 200), (10, 10, 1, 1)),            # a sub-pixel box: one pixel
    ((10.75, 10.75, 11.25, 11.25), (100, 200), (10, 10, 2, 2)),          # a sub-pixel box across a pixel boundary: two
    ((10.0, 20.0, 30.0, 40.0), (100, 200), (10, 20, 20, 20)),            # integer corners: floor and ceil move nothing
    ((0.0, 0.0, 200.0, 100.0), (100, 200), (0, 0, 200, 100)),            # the whole frame
    ((0.0, 0.0, 1.0, 1.0), (1, 1), (0, 0, 1, 1)),                        # a 1x1 frame
    ((-3.0, -3.0, 0.5, 0.25), (1, 1), (0, 0, 1, 1)),
    ((1.0, 0.0, 2.0, 1.0), (1, 1), None),
]


def test_crop_rect_hand_written_cases():
    m = _lib()
    for box, (h, w), want in HAND:
        assert crops_model.crop_rect(box, h, w) == want, ("model", box, h, w)
        assert _c_rect(m, box, h, w) == want, ("library", box, h, w)
        for pad in (0.0, 0.1, 16.0):
            assert _c_rect(m, box, h, w, pad, pad) == crops_model.crop_rect(box, h, w, pad, pad), (box, h, w, pad)


def test_crop_rect_pads_by_hand():
    """pad 0.1 in fp32 is 0.100000001490116...: 10 - 0.1f * 20 = 7.99999997 -> floor 7; 30 + 0.1f * 20 = 32.00000003 -> ceil 33"""
    m = _lib()
    assert _c_rect(m, (10.0, 10.0, 30.0, 30.0), 100, 200, 0.1, 0.0) == (7, 10, 26, 20)
    assert _c_rect(m, (10.0, 10.0, 30.0, 30.0), 100, 200, 0.0, 0.5) == (10, 0, 20, 40)
    assert _c_rect(m, (10.0, 10.0, 30.0, 30.0), 100, 200, 16.0, 16.0) == (0, 0, 200, 100)
    # a pad can bring a box that lies outside back in: [-30, -1] grows by 16 * 29 on each side
    assert _c_rect(m, (-30.0, 10.0, -1.0, 30.0), 100, 200, 16.0, 0.0) == (0, 10, 200, 20)


def _seeded_boxes(n, seed):
    """boxes around and across a frame: fractional, integer-cornered, degenerate, far away"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        h, w = (int(v) for v in rng.choice([1, 2, 3, 17, 240, 1080, 4000], 2))
        kind = rng.integers(0, 5)
        if kind == 0:
            c = rng.uniform(-0.5, 1.5, 4) * [w, h, w, h]
        elif kind == 1:
            c = np.floor(rng.uniform(-0.2, 1.2, 4) * [w, h, w, h])
        elif kind == 2:
            x, y = rng.uniform(0, w), rng.uniform(0, h)
            c = np.array([x, y, x + rng.uniform(0, 1.5), y + rng.uniform(0, 1.5)])
        elif kind == 3:
            c = rng.uniform(-3, 3, 4) * [w, h, w, h]
        else:
            c = rng.uniform(-0.5, 1.5, 4) * [w, h, w, h]
            c[rng.integers(0, 4)] = rng.choice([0.0, -0.0, w, h, NAN, INF, -INF, 1e30, -1e30, 1e-30])
        out.append((tuple(np.float32(c).tolist()), h, w))
    return out


def test_crop_rect_matches_the_model_and_keeps_its_promises():
    m = _lib()
    n_rect = 0
    for i, (box, h, w) in enumerate(_seeded_boxes(4000, 2024)):
        px, py = ((0.0, 0.0), (0.1, 0.1), (16.0, 16.0), (0.25, 1.5))[i % 4]
        got = _c_rect(m, box, h, w, px, py)
        assert got == crops_model.crop_rect(box, h, w, px, py), (box, h, w, px, py)
        if got is None:
            continue
        n_rect += 1
        X0, Y0, cw, ch = got
        assert cw >= 1 and ch >= 1 and 0 <= X0 and X0 + cw <= w and 0 <= Y0 and Y0 + ch <= h, (box, h, w, got)
        # the rectangle contains the clipped padded box (exact: every term is a double of few bits or the rule's own value)
        x1, y1, x2, y2 = (float(np.float32(v)) for v in box)
        fx, fy = float(np.float32(px)), float(np.float32(py))
        cx1, cx2 = max(x1 - fx * (x2 - x1), 0.0), min(x2 + fx * (x2 - x1), float(w))
        cy1, cy2 = max(y1 - fy * (y2 - y1), 0.0), min(y2 + fy * (y2 - y1), float(h))
        assert X0 <= cx1 and cx2 <= X0 + cw and Y0 <= cy1 and cy2 <= Y0 + ch, (box, h, w, got)
        # ... and not a pixel more than floor / ceil demand
        assert X0 == math.floor(cx1) and X0 + cw == math.ceil(cx2) and Y0 == math.floor(cy1) and Y0 + ch == math.ceil(cy2)
    assert n_rect > 1000        # the seeded set exercises both outcomes


def test_crop_rect_argument_errors():
    m = _lib()
    L = m.lib()
    box, rect = (C.c_float * 4)(1, 1, 5, 5), (C.c_int32 * 4)(-77, -77, -77, -77)
    for args in ((None, 10, 10, 0.0, 0.0, rect), (box, 10, 10, 0.0, 0.0, None), (box, 0, 10, 0.0, 0.0, rect), (box, 10, 0, 0.0, 0.0, rect),
                 (box, 10, 10, -0.1, 0.0, rect), (box, 10, 10, 0.0, 16.5, rect), (box, 10, 10, NAN, 0.0, rect), (box, 10, 10, 0.0, INF, rect)):
        assert L.yfv2_crop_rect(*args) == m.ERR_ARG, args
        assert "yfv2_crop_rect" in m.last_error()
    assert list(rect) == [-77] * 4
    assert L.yfv2_crop_rect(box, 10, 10, 16.0, 0.0, rect) == 1      # the bound itself is allowed


def test_class_filter_of_the_model():
    ok = crops_model.class_passes
    assert ok(0.0, None) and ok(254.0, None) and ok(-0.0, None)
    assert not ok(255.0, None) and not ok(-1.0, None) and not ok(1.5, None) and not ok(NAN, None) and not ok(INF, None)
    assert ok(3.0, [1, 3]) and not ok(2.0, [1, 3]) and not ok(3.0, [])


def test_model_selection_offsets_and_src_on_a_hand_computed_case():
    """five frames of 100 x 200, R = 4: count 0; count > R; a negative count; max_per_frame cutting a frame; a class filter and a
    skipped row that takes no slot"""
    good = lambda x, cls: [x, 10.0, x + 10.0, 30.0, 0.9, cls]
    bad = lambda cls: [50.0, 10.0, 50.0, 30.0, 0.9, cls]                 # x1 == x2: skipped
    R = 4
    dets = np.zeros((5, R, 6), np.float32)
    dets[0] = [good(0, 0), good(10, 0), good(20, 0), good(30, 0)]        # count 0: nothing
    dets[1] = [good(0, 1), good(10, 1), good(20, 1), good(30, 1)]        # count 9 > R: all four rows, cut to 3 by max_per_frame
    dets[2] = [good(0, 1), good(10, 1), good(20, 1), good(30, 1)]        # count -2: nothing
    dets[3] = [bad(1), good(10, 1), bad(1), good(30, 1)]                 # two skipped rows: the two others take slots 0, 1
    dets[4] = [good(0, 2), good(10, 1), bad(2), good(30, 1.5)]           # class 2 filtered out (skipped or not), 1.5 is no class
    count = [0, 9, -2, 4, 4]
    sizes = [(100, 200)] * 5
    p = crops_model.plan(dets, count, sizes, max_per_frame=3, classes=[0, 1])
    assert p["offset"].tolist() == [0, 0, 3, 3, 5, 6]
    assert p["skipped"].tolist() == [0, 0, 0, 2, 0]                      # frame 4's degenerate row is class 2: no candidate, not counted
    assert p["src"].tolist() == [1 * R + 0, 1 * R + 1, 1 * R + 2, 3 * R + 1, 3 * R + 3, 4 * R + 1]
    assert p["frame"].tolist() == [1, 1, 1, 3, 3, 4]
    assert p["rect"].tolist() == [[0, 10, 10, 20], [10, 10, 10, 20], [20, 10, 10, 20], [10, 10, 10, 20], [30, 10, 10, 20], [10, 10, 10, 20]]
    # a cap below the total truncates what is written and nothing else
    q = crops_model.plan(dets, count, sizes, max_per_frame=3, classes=[0, 1], cap=4)
    assert q["offset"].tolist() == p["offset"].tolist() and q["skipped"].tolist() == p["skipped"].tolist()
    assert q["src"].tolist() == p["src"].tolist()[:4] and q["rect"].tolist() == p["rect"].tolist()[:4]
    # without the filter frame 4 contributes its class-2 row, skips the degenerate one and still drops class 1.5
    a = crops_model.plan(dets, count, sizes, max_per_frame=300)
    assert a["offset"].tolist() == [0, 0, 4, 4, 6, 8] and a["skipped"].tolist() == [0, 0, 0, 2, 1]
    assert a["src"].tolist()[-2:] == [4 * R + 0, 4 * R + 1]


def test_entry_points_are_bound():
    m = _lib()
    for name in ("yfv2_crop_rect", "yfv2_crop_detections_u8", "yfv2_crop_detections_yuv"):
        assert name in m._PROTOTYPES and hasattr(m.lib(), name)
    assert C.sizeof(m.CropRule) == 40       # int32 x2, float x2, int32, (pad), pointer, int32, (pad): the C layout on LP64
