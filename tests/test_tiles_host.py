"""CPU-only checks of tiled detection (include/yfv2.h yfv2_tile_plan, yfv2_merge_tiles, yfv2_detect_tiled_u8):
  * yfv2_tile_plan (host code of the library) equals the rule restated in tests/tiles_ref.py, and every plan has the
    properties a caller relies on
  * the numpy model of the merge, which the GPU tests compare the device with bit for bit, is itself pinned against the
    oracle's torchvision NMS where the two rules coincide
  * the new entry points are exported and bound, and argument errors that need no device are reported
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import yfv2_oracle as oracle
from tiles_ref import MAX_DET, merge_model, plan_axis, plan_tiles


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _c_plan(m, fh, fw, th, tw, oh, ow, full):
    L = m.lib()
    n = L.yfv2_tile_plan(fh, fw, th, tw, oh, ow, full, None, 0)
    assert n >= 1, m.last_error()
    arr = (m.Tile * n)()
    assert L.yfv2_tile_plan(fh, fw, th, tw, oh, ow, full, arr, n) == n       # the count asked for with NULL agrees with the filled one
    return [(t.frame, t.x0, t.y0, t.width, t.height) for t in arr]


LENGTHS = (1, 351, 352, 353, 640, 352 + 288, 352 + 288 + 1, 4000)


def _check_axis(L, t, o, ivals):
    assert ivals == plan_axis(L, t, o)
    assert ivals[0][0] == 0 and ivals[-1][0] + ivals[-1][1] == L                 # starts at 0, the last one ends on the edge
    covered = np.zeros(L, bool)
    for s, n in ivals:
        assert 0 <= s and s + n <= L and n == min(t, L)                           # inside the axis, full length
        covered[s:s + n] = True
    assert covered.all()
    for (s0, n0), (s1, _n1) in zip(ivals, ivals[1:]):
        assert s1 > s0 and s0 + n0 - s1 >= o, (L, t, o, ivals)                    # neighbours overlap by at least o
    if L > t:
        assert len(ivals) == -(-(L - t) // (t - o)) + 1


@pytest.mark.parametrize("o", [64, 0, 351])
def test_tile_plan_matches_the_rule_and_has_its_properties(o):
    m = _lib()
    t = 352
    for L in LENGTHS:
        for full in (0, 1):
            # this length on the y axis against a fixed x axis, and on the x axis against a fixed y axis
            # (both axes at once only where that is not millions of tiles: 4000 at overlap 351 is 3649 per axis)
            for fh, fw, th, tw, oh, ow in ((L, 500, t, 200, o, 30), (700, L, 300, t, 17, o)) + (((L, L, t, t, o, o),) if L < 1000 else ()):
                got = _c_plan(m, fh, fw, th, tw, oh, ow, full)
                want = plan_tiles(fh, fw, (th, tw), (oh, ow), bool(full))
                assert got == want, (fh, fw, th, tw, oh, ow, full)
                ys, xs = plan_axis(fh, th, oh), plan_axis(fw, tw, ow)
                grid = got[:len(ys) * len(xs)]
                assert grid == [(0, x0, y0, w, h) for y0, h in ys for x0, w in xs]      # row-major, y outer
                _check_axis(fh, th, oh, sorted({(y0, h) for _, _, y0, _, h in grid}))
                _check_axis(fw, tw, ow, sorted({(x0, w) for _, x0, _, w, _ in grid}))
                # include_full appends exactly one whole-frame tile, and only when the grid has more than one
                extra = got[len(grid):]
                assert extra == ([(0, 0, 0, fw, fh)] if full and len(grid) > 1 else [])
                for _, x0, y0, w, h in got:
                    assert x0 >= 0 and y0 >= 0 and w >= 1 and h >= 1 and x0 + w <= fw and y0 + h <= fh


def test_tile_plan_python_wrapper_and_errors():
    m = _lib()
    from yolo_fastestv2_amd import tiling
    assert tiling.plan_tiles(1080, 1920) == plan_tiles(1080, 1920) and len(tiling.plan_tiles(1080, 1920)) == 28
    assert len(tiling.plan_tiles(2160, 3840)) == 112
    assert tiling.plan_tiles(700, 1000, tile=(300, 500), overlap=(0, 17), include_full=True, frame=3) == plan_tiles(700, 1000, (300, 500), (0, 17), True, 3)
    assert tiling.plan_tiles(100, 100, tile=352, overlap=64, include_full=True) == [(0, 0, 0, 100, 100)]
    L = m.lib()
    arr = (m.Tile * 28)()
    assert L.yfv2_tile_plan(1080, 1920, 352, 352, 64, 64, 0, arr, 27) == m.ERR_ARG and "cap 27 < 28" in m.last_error()
    assert L.yfv2_tile_plan(1080, 1920, 352, 352, 64, 64, 1, arr, 28) == m.ERR_ARG        # the whole-frame tile needs a 29th entry
    for bad in ((0, 10, 4, 4, 0, 0), (10, 0, 4, 4, 0, 0), (10, 10, 0, 4, 0, 0), (10, 10, 4, -1, 0, 0), (10, 10, 4, 4, 4, 0), (10, 10, 4, 4, 0, 4),
                (10, 10, 4, 4, -1, 0), (10, 10, 4, 4, 0, -1)):
        assert L.yfv2_tile_plan(*bad, 0, None, 0) == m.ERR_ARG, bad
        assert L.yfv2_tile_plan(*bad, 0, arr, 28) == m.ERR_ARG, bad
    assert L.yfv2_tile_plan(2**31 - 1, 2**31 - 1, 2, 2, 1, 1, 0, None, 0) == m.ERR_ARG    # more tiles than an int32 counts
    for bad in (dict(tile=(1, 2, 3)), dict(overlap=352), dict(tile=0)):
        with pytest.raises(ValueError):
            tiling.plan_tiles(100, 100, **bad)


def test_tile_entry_points_are_exported_and_refuse_a_null_handle():
    m = _lib()
    L = m.lib()
    raw = C.CDLL(m.LIB_PATH)
    for name in ("yfv2_tile_plan", "yfv2_merge_tiles", "yfv2_detect_tiled_u8"):
        assert name in m._PROTOTYPES and hasattr(raw, name)
    assert C.sizeof(m.Tile) == 20
    assert L.yfv2_abi_version() == 7                     # additive: the number stays
    t = (m.Tile * 1)()
    t[0].width = t[0].height = 4
    p = C.c_void_p(64)
    assert L.yfv2_merge_tiles(None, p, p, t, 1, 1, 0.5, 0, 300, p, p, p, None) == m.ERR_ARG and "null handle" in m.last_error()
    fr = (m.Frame * 1)()
    fr[0].data, fr[0].height, fr[0].width, fr[0].row_pitch = 64, 4, 4, 12
    assert L.yfv2_detect_tiled_u8(None, fr, 1, t, 1, 0.3, 0.4, 0.4, 0, 300, p, p, p, None) == m.ERR_ARG and "null handle" in m.last_error()


def _random_case(rng, n, tiles, n_scores, n_cls, span):
    """n boxes with integer coordinates in [0, span) and a few distinct scores, dealt to the tiles in consecutive groups; inside a
    group the rows are ordered by score (stable), so that the flat (tile, row) order is an index order the oracle can be given"""
    T = len(tiles)
    x1 = rng.integers(0, span - 40, n)
    y1 = rng.integers(0, span - 40, n)
    w = rng.integers(0, 40, n)             # zero-width boxes included
    h = rng.integers(0, 40, n)
    boxes = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    # a third of the boxes repeat an earlier box, some of them under another class
    rep = rng.random(n) < 0.33
    boxes[rep] = boxes[rng.integers(0, n, rep.sum())]
    conf = (rng.integers(1, n_scores + 1, n) / np.float32(n_scores + 1)).astype(np.float32)
    cls = rng.integers(0, n_cls, n).astype(np.float32)
    assert T == 5 and n == 700
    sizes = rng.integers(134, 201, 3).tolist()
    sizes = [sizes[0], sizes[1], 0, sizes[2], n - sum(sizes)]      # a tile without rows in the middle of the range; every size <= 300
    bounds = np.concatenate(([0], np.cumsum(sizes)))
    tile_dets = np.zeros((T, MAX_DET, 6), np.float32)
    tile_count = np.zeros(T, np.int32)
    flat = []
    for k in range(T):
        lo, hi = int(bounds[k]), int(bounds[k + 1])
        assert hi - lo <= MAX_DET
        ids = np.arange(lo, hi)
        ids = ids[np.argsort(-conf[ids], kind="stable")]
        _, x0, y0, _, _ = tiles[k]
        tile_dets[k, :len(ids), :4] = boxes[ids] - np.float32([x0, y0, x0, y0])      # integers: exact
        tile_dets[k, :len(ids), 4], tile_dets[k, :len(ids), 5] = conf[ids], cls[ids]
        tile_count[k] = len(ids)
        flat.extend(ids.tolist())
    flat = np.asarray(flat, np.int64)
    origin = np.concatenate([k * MAX_DET + np.arange(tile_count[k]) for k in range(T)]).astype(np.int32)
    return tile_dets, tile_count, boxes[flat], conf[flat], cls[flat], origin


@pytest.mark.parametrize("seed", range(6))
def test_merge_model_is_torchvision_nms_where_the_class_offset_is_exact(seed):
    """Integer coordinates below 4096 and classes below 80: x + 4096 cls is exact in fp32, boxes of different classes cannot
    meet, so non_max_suppression's class-offset NMS and the merge rule (metric 0) are the same function.  Every case is
    decided by the oracle alone: several hundred boxes, few distinct scores (ties within and across tiles), repeated boxes,
    zero-area boxes, thresholds that the exact ratios hit (0.5, 0.25, 0)."""
    rng = np.random.default_rng(seed)
    tiles = [(0, 0, 0, 352, 352), (0, 288, 0, 352, 352), (0, 0, 17, 400, 300), (0, 0, 0, 640, 640), (0, 31, 5, 352, 352)]
    n = 700
    tile_dets, tile_count, boxes, conf, cls, origin = _random_case(rng, n, tiles, n_scores=7, n_cls=3 if seed % 2 else 80, span=(300, 4055)[seed % 2])
    assert tile_count[2] == 0 and tile_count.sum() >= 300
    assert boxes.max() < 4096 and (boxes == np.round(boxes)).all()
    for thres in (0.5, 0.25, 0.0, 0.4):
        for max_out in (300, 7, 4096):
            keep = oracle.nms_greedy(boxes + cls[:, None] * np.float32(4096), conf, thres)[:max_out]
            dets, src, count = merge_model(tile_dets, tile_count, tiles, 1, thres, 0, max_out, fill=-1.0, fill_src=-1)
            assert count[0] == len(keep), (thres, max_out, count[0], len(keep))
            assert np.array_equal(src[0, :len(keep)], origin[keep])
            want = np.concatenate([boxes[keep], conf[keep, None], cls[keep, None]], 1)
            assert np.array_equal(dets[0, :len(keep)].view(np.uint32), want.view(np.uint32))
            assert (dets[0, len(keep):] == -1.0).all() and (src[0, len(keep):] == -1).all()
    if seed % 2:
        assert 7 < count[0] < tile_count.sum()          # the dense case: many kept, many dropped


def test_merge_model_frames_and_metric_1():
    """what the oracle cannot say: frames are independent, a frame without tiles has count 0, and metric 1 merges a half box
    with its whole box where metric 0 keeps both"""
    td = np.zeros((3, MAX_DET, 6), np.float32)
    td[0, 0] = [0, 0, 10, 10, 0.9, 1]
    td[1, 0] = [0, 0, 5, 10, 0.8, 1]        # tile 1 starts at x0 = 5: the right half of the box above
    td[2, 0] = [0, 0, 10, 10, 0.7, 1]       # another frame: not compared with frame 0's boxes
    tc = np.asarray([1, 1, 1], np.int32)
    tiles = [(0, 0, 0, 20, 20), (0, 5, 0, 15, 20), (2, 0, 0, 20, 20)]
    d0, s0, c0 = merge_model(td, tc, tiles, 3, 0.6, 0, 300)
    d1, s1, c1 = merge_model(td, tc, tiles, 3, 0.6, 1, 300)
    assert c0.tolist() == [2, 0, 1] and c1.tolist() == [1, 0, 1]
    assert s0[0, :2].tolist() == [0, 300] and d0[0, 1, :4].tolist() == [5, 0, 10, 10] and s0[2, 0] == 600


def test_detect_tiled_argument_errors_that_need_no_device():
    _lib()
    from yolo_fastestv2_amd import tiling
    from yolo_fastestv2_amd.engine import Engine
    eng = Engine.__new__(Engine)              # no handle: everything below is refused before one is needed
    eng._anchors_set, eng._h = True, None
    for kw in (dict(metric="giou"), dict(metric=2), dict(metric=True), dict(max_out=0), dict(max_out=4097)):
        with pytest.raises(ValueError):
            eng.detect_tiled([], conf_thres=0.3, iou_thres=0.4, **kw)
    eng._anchors_set = False
    with pytest.raises(RuntimeError):
        eng.detect_tiled([], conf_thres=0.3, iou_thres=0.4)
    with pytest.raises(ValueError):
        eng.merge_tiles(None, None, [(0, 0, 0, 4, 4)], 1, 0.5, metric="union")
    with pytest.raises(ValueError):
        tiling.tile_table([])
    with pytest.raises(ValueError):
        tiling.tile_table([(0, 0, 0, 4)])
    assert tiling.metric_code("iou") == 0 and tiling.metric_code("ios") == 1
