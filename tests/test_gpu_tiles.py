"""GPU tests of tiled detection: Engine.detect_tiled / Engine.merge_tiles / DetectPipeline.submit_tiled (include/yfv2.h
yfv2_detect_tiled_u8, yfv2_merge_tiles).  Run with ``-m gpu`` on an MI355X.

The claims: detect_tiled equals the composition it replaces - detect_frames on the crop views, then the merge rule as
tests/tiles_ref.py restates it in numpy - bit for bit (counts, src, the uint32 views of dets), on every plan; the merge alone
equals the model on crafted rows (ties, NaN matches, thresholds hit exactly, offsets beyond 4096, 64 x 300 candidates);
bad arguments fail before anything is launched.  No tolerances anywhere.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import yfv2_oracle as oracle
from tiles_ref import MAX_DET, merge_model, plan_tiles

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0    # output buffers are pre-filled with it: rows beyond count must come back untouched
SRC_FILL, CNT_FILL = -7, -9


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
    return _engine(yfv2, dev, cfg, coco_weights, max_batch=16)


def _out(eng, F, max_out=MAX_DET):
    dets, src, cnt = eng.new_tiled_buffers(F, max_out)
    dets.fill_(SENTINEL)
    src.fill_(SRC_FILL)
    cnt.fill_(CNT_FILL)
    return dets, src, cnt


def _picture(images_u8, k, h, w, seed):
    """a plausible (h, w, 3) frame: reference image k resized by the oracle, plus a little seeded noise"""
    hwc = np.ascontiguousarray(images_u8[k % len(images_u8)].transpose(1, 2, 0))
    rng = np.random.default_rng(seed)
    f = oracle.resize_linear_u8(hwc, w, h)
    return np.clip(f.astype(np.int16) + rng.integers(-3, 4, f.shape), 0, 255).astype(np.uint8)


def _mosaic(images_u8, h, w, seed):
    """a large frame made of several reference pictures side by side: objects in every tile"""
    out = np.zeros((h, w, 3), np.uint8)
    hh, hw = (h + 1) // 2, (w + 1) // 2
    for k, (y, x) in enumerate(((0, 0), (0, hw), (hh, 0), (hh, hw))):
        p = _picture(images_u8, seed + k, min(hh, h - y), min(hw, w - x), seed + k)
        out[y:y + p.shape[0], x:x + p.shape[1]] = p
    return out


def _assert_same(got, want, what):
    gd, gs, gc = (t.cpu().numpy() for t in got)
    wd, ws, wc = want
    assert np.array_equal(gc, wc), "%s: counts %s vs %s" % (what, gc.tolist(), wc.tolist())
    assert np.array_equal(gs, ws), "%s: src differs" % what
    bad = np.argwhere(gd.view(np.uint32) != wd.view(np.uint32))
    assert bad.size == 0, "%s: %d dets words differ, first at %s: %r vs %r" % (what, len(bad), bad[0].tolist(), gd[tuple(bad[0])], wd[tuple(bad[0])])


def _model(td, tc, tiles, F, thres, metric, max_out):
    return merge_model(td, tc, tiles, F, thres, metric, max_out, fill=SENTINEL, fill_src=SRC_FILL)


def _tile_detections(eng, frames, tiles, conf, iou):
    """the first half of the composition: detect_frames on the crop views -> host (tile_dets, tile_count)"""
    from yolo_fastestv2_amd import tiling
    d, _, c = eng.detect_frames(tiling.crop_views(frames, tiles), conf, iou)
    return d.cpu().numpy(), c.cpu().numpy()


# ---- 1. one tile that is the whole frame ------------------------------------------------------------------------------------
def test_one_whole_frame_tile_is_detect_frames(yfv2, dev, engine, images_u8):
    frame = torch.from_numpy(_picture(images_u8, 0, 480, 640, 5)).to(dev)
    got = engine.detect_tiled([frame], tiles=[(0, 0, 0, 640, 480)], conf_thres=0.3, iou_thres=0.4, out=_out(engine, 1))
    rd, _, rc = engine.detect_frames([frame], 0.3, 0.4)
    n = int(rc[0])
    assert n > 0 and int(got[2][0]) == n
    gd, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gd[0, :n].view(np.uint32), rd.cpu().numpy()[0, :n].view(np.uint32))
    assert gs[0, :n].tolist() == list(range(n))
    assert (gd[0, n:] == SENTINEL).all() and (gs[0, n:] == SRC_FILL).all()
    # the same through the planner: a frame no larger than the tile is one tile
    again = engine.detect_tiled([frame], conf_thres=0.3, iou_thres=0.4, tile=(480, 640), overlap=0, include_full=True, out=_out(engine, 1))
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ---- 2. composition -----------------------------------------------------------------------------------------------------------
PLANS = {"t352_o64_full": dict(tile=(352, 352), overlap=(64, 64), include_full=True), "t300x500_o0x17": dict(tile=(300, 500), overlap=(0, 17), include_full=False)}


def _three_frames(dev, images_u8, views):
    """700x1000, a frame that gets no tiles, 352x352; views=True: each a non-contiguous crop of a larger tensor at an odd byte offset"""
    host = [_mosaic(images_u8, 700, 1000, 1), _picture(images_u8, 2, 90, 120, 9), _picture(images_u8, 3, 352, 352, 10)]
    if not views:
        return [torch.from_numpy(h).to(dev) for h in host]
    frames = []
    for h in host:
        parent = torch.zeros((h.shape[0] + 5, h.shape[1] + 11, 3), dtype=torch.uint8, device=dev)
        parent[3:3 + h.shape[0], 8:8 + h.shape[1]] = torch.from_numpy(h).to(dev)
        v = parent[3:3 + h.shape[0], 8:8 + h.shape[1]]
        assert not v.is_contiguous() and v.stride(0) % 2 == 1 and (v.data_ptr() - parent.data_ptr()) % 2 == 1      # odd pitch, odd byte offset
        frames.append(v)
    return frames


@pytest.mark.parametrize("views", [False, True], ids=["contiguous", "crop_views"])
@pytest.mark.parametrize("conf", [0.3, 0.01])
@pytest.mark.parametrize("plan", list(PLANS))
def test_detect_tiled_is_detect_frames_then_the_merge_model(yfv2, dev, engine, images_u8, plan, conf, views):
    frames = _three_frames(dev, images_u8, views)
    kw = PLANS[plan]
    tiles = plan_tiles(700, 1000, kw["tile"], kw["overlap"], kw["include_full"], frame=0) + plan_tiles(352, 352, kw["tile"], kw["overlap"], kw["include_full"], frame=2)
    assert len(tiles) == {"t352_o64_full": 14, "t300x500_o0x17": 11}[plan]
    td, tc = _tile_detections(engine, frames, tiles, conf, 0.4)
    assert tc.sum() > 0, tc
    kept = {}
    for metric, code in (("iou", 0), ("ios", 1)):
        for max_out in (300, 7):
            got = engine.detect_tiled(frames, tiles=tiles, conf_thres=conf, iou_thres=0.4, metric=metric, max_out=max_out, out=_out(engine, 3, max_out))
            want = _model(td, tc, tiles, 3, 0.4, code, max_out)
            _assert_same(got, want, "%s conf %g %s max_out %d" % (plan, conf, metric, max_out))
            assert want[2][1] == 0 and want[2][0] > 0                              # the frame without tiles; the mosaic of four pictures
            kept[metric, max_out] = want[2].copy()
    assert kept["iou", 7][0] == min(7, kept["iou", 300][0])                        # max_out cuts the list
    # a merge threshold of its own
    got = engine.detect_tiled(frames, tiles=tiles, conf_thres=conf, iou_thres=0.4, merge_thres=0.15, out=_out(engine, 3))
    _assert_same(got, _model(td, tc, tiles, 3, 0.15, 0, 300), "%s merge_thres 0.15" % plan)
    if not views:
        # tiles=None plans every frame (here the small middle frame gets its one tile too)
        got = engine.detect_tiled(frames, conf_thres=conf, iou_thres=0.4, out=_out(engine, 3), **kw)
        tiles_all = [t for f, fr in enumerate(frames) for t in plan_tiles(int(fr.shape[0]), int(fr.shape[1]), kw["tile"], kw["overlap"], kw["include_full"], frame=f)]
        td2, tc2 = _tile_detections(engine, frames, tiles_all, conf, 0.4)
        _assert_same(got, _model(td2, tc2, tiles_all, 3, 0.4, 0, 300), "%s planned" % plan)


# ---- 3. the merge alone, on crafted rows ------------------------------------------------------------------------------------------
def _rows(*rows):
    a = np.zeros((MAX_DET, 6), np.float32)
    for i, r in enumerate(rows):
        a[i] = r
    return a, len(rows)


def _run_merge(eng, dev, tds, tiles, F, thres, metric, max_out, what):
    td = np.stack([t for t, _ in tds]).astype(np.float32)
    tc = np.asarray([n for _, n in tds], np.int32)
    got = eng.merge_tiles(torch.from_numpy(td).to(dev), torch.from_numpy(tc).to(dev), tiles, F, thres, metric=("iou", "ios")[metric], max_out=max_out,
                          out=_out(eng, F, max_out))
    want = _model(td, tc, tiles, F, thres, metric, max_out)
    _assert_same(got, want, what)
    return want


def test_merge_tiles_on_crafted_rows(yfv2, dev, engine):
    eng = engine
    T0 = (0, 0, 0, 352, 352)
    # identical boxes of different classes: both kept; of the same class: one
    w = _run_merge(eng, dev, [_rows([10, 10, 50, 50, .9, 3]), _rows([10, 10, 50, 50, .8, 4]), _rows([10, 10, 50, 50, .7, 3])], [T0, T0, T0], 1, 0.4, 0, 300, "classes")
    assert w[2][0] == 2 and w[1][0, :2].tolist() == [0, 300]
    # zero-area boxes: 0 / 0 is a NaN match, which suppresses nothing - not even under a negative threshold
    for thres in (0.4, -1.0):
        w = _run_merge(eng, dev, [_rows([5, 5, 5, 9, .9, 1], [5, 5, 5, 9, .9, 1]), _rows([5, 5, 5, 9, .9, 1])], [T0, T0], 1, thres, 0, 300, "zero area %g" % thres)
        assert w[2][0] == 3
    # touching boxes: a match of 0, kept at threshold 0 because the test is >
    for metric in (0, 1):
        w = _run_merge(eng, dev, [_rows([0, 0, 10, 10, .9, 1]), _rows([0, 0, 10, 10, .8, 1])], [T0, (0, 10, 0, 352, 352)], 1, 0.0, metric, 300, "touching")
        assert w[2][0] == 2
    # a match exactly equal to the threshold is kept; one ulp below it, dropped
    pair = [_rows([0, 0, 2, 2, .9, 1], [0, 0, 2, 1, .8, 1])]
    assert _run_merge(eng, dev, pair, [T0], 1, 0.5, 0, 300, "match == threshold")[2][0] == 2
    assert _run_merge(eng, dev, pair, [T0], 1, float(np.nextafter(0.5, 0.0)), 0, 300, "match just above")[2][0] == 1
    # metric 1 merges a half box with its whole box where metric 0 keeps both
    half = [_rows([0, 0, 10, 10, .9, 1]), _rows([0, 0, 5, 10, .8, 1])]
    ht = [(0, 0, 0, 20, 20), (0, 5, 0, 15, 20)]
    assert _run_merge(eng, dev, half, ht, 1, 0.6, 0, 300, "half box, IoU")[2][0] == 2
    assert _run_merge(eng, dev, half, ht, 1, 0.6, 1, 300, "half box, smaller")[2][0] == 1
    # offsets above 4096 with fractional coordinates: the sum rounds in fp32, classes are compared, not offset
    rng = np.random.default_rng(3)

    def random_tile(n, lo=0.0, hi=352.0, size=60.0, n_cls=3, n_scores=0):
        xy = rng.random((n, 2)) * (hi - lo - size) + lo
        wh = rng.random((n, 2)) * size
        conf = np.sort(rng.random(n) if not n_scores else rng.integers(1, n_scores + 1, n) / (n_scores + 1.0))[::-1]
        a = np.zeros((MAX_DET, 6), np.float32)
        a[:n] = np.concatenate([xy, xy + wh, conf[:, None], rng.integers(0, n_cls, (n, 1))], 1)
        return a, n
    far = [(0, 5000, 70001, 352, 352), (0, 5100, 70001, 352, 352), (0, 5000, 70123, 352, 352), (1, 4097, 0, 352, 352), (1, 4197, 0, 352, 352)]
    w = _run_merge(eng, dev, [random_tile(n) for n in (300, 250, 300, 120, 300)], far, 2, 0.3, 0, 300, "offsets above 4096")
    assert w[2][0] > 0 and w[2][1] > 0 and w[0][0, 0, 1] > 70000 and w[0][1, 0, 0] > 4096
    # equal scores within and across tiles (the order is stable over tile, row), a tile with count 0 in the middle of a range
    tied = [random_tile(n, n_scores=5) for n in (200, 300, 0, 300, 64, 65)]
    tt = [(0, 0, 0, 352, 352), (0, 100, 0, 352, 352), (0, 200, 0, 352, 352), (0, 0, 100, 352, 352), (1, 0, 0, 352, 352), (1, 30, 30, 352, 352)]
    for metric in (0, 1):
        for max_out in (1, 300, 4096):
            w = _run_merge(eng, dev, tied, tt, 3, 0.45, metric, max_out, "ties metric %d max_out %d" % (metric, max_out))
            assert w[2][2] == 0 and w[2][0] == (1 if max_out == 1 else w[2][0])
    # truncation: 5400 disjoint boxes in 18 tiles -> exactly max_out of them, in order
    grid = []
    for k in range(18):
        a = np.zeros((MAX_DET, 6), np.float32)
        i = np.arange(MAX_DET)
        a[:, 0], a[:, 1] = (i % 20) * 10, (i // 20) * 10
        a[:, 2], a[:, 3] = a[:, 0] + 9, a[:, 1] + 9
        a[:, 4], a[:, 5] = np.linspace(0.99, 0.01, MAX_DET).astype(np.float32), k % 2
        grid.append((a, MAX_DET))
    gt = [(0, 200 * (k % 6), 150 * (k // 6), 200, 150) for k in range(18)]
    for max_out in (1, 300, 4096):
        w = _run_merge(eng, dev, grid, gt, 1, 0.4, 0, max_out, "truncation at %d" % max_out)
        assert w[2][0] == max_out


def test_merge_tiles_64_full_tiles_next_to_a_single_row(yfv2, dev, engine):
    """the worst case the workspace is sized for: 64 tiles x 300 rows on one frame (19 200 candidates), next to a frame with one
    row; the same call twice gives identical bits"""
    rng = np.random.default_rng(8)
    tiles, tds = [], []
    for k in range(64):
        x0, y0 = 220 * (k % 8), 110 * (k // 8)
        xy = rng.random((MAX_DET, 2)) * 300
        wh = rng.random((MAX_DET, 2)) * 50 + 2
        conf = np.sort(rng.integers(1, 2000, MAX_DET) / 2000.0)[::-1]      # ties across tiles, some within
        a = np.concatenate([xy, xy + wh, conf[:, None], rng.integers(0, 4, (MAX_DET, 1))], 1).astype(np.float32)
        tds.append((a, MAX_DET))
        tiles.append((0, x0, y0, 352, 352))
    tds.append(_rows([1, 2, 30, 40, .5, 7]))
    tiles.append((1, 3, 4, 352, 352))
    td = torch.from_numpy(np.stack([t for t, _ in tds])).to(dev)
    tc = torch.from_numpy(np.asarray([n for _, n in tds], np.int32)).to(dev)
    for metric, max_out in ((0, 300), (1, 4096)):
        got = engine.merge_tiles(td, tc, tiles, 2, 0.4, metric=metric, max_out=max_out, out=_out(engine, 2, max_out))
        again = engine.merge_tiles(td, tc, tiles, 2, 0.4, metric=metric, max_out=max_out, out=_out(engine, 2, max_out))
        for a, b in zip(got, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        want = _model(td.cpu().numpy(), tc.cpu().numpy(), tiles, 2, 0.4, metric, max_out)
        _assert_same(got, want, "64 x 300, metric %d, max_out %d" % (metric, max_out))
        assert want[2][1] == 1 and want[1][1, 0] == 64 * 300 and want[0][1, 0].tolist() == [4, 6, 33, 44, .5, 7]
        assert want[2][0] == 300 if max_out == 300 else want[2][0] > 300


# ---- 4. other plans, the pipeline -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [{"fp32_matrix": 1}, {"lanes": 2}], ids=["fp32_matrix", "lanes2"])
def test_detect_tiled_on_other_plans(yfv2, dev, cfg, coco_weights, images_u8, plan):
    frames = _three_frames(dev, images_u8, False)
    kw = PLANS["t352_o64_full"]
    tiles = plan_tiles(700, 1000, frame=0, **kw) + plan_tiles(352, 352, frame=2, **kw)
    eng = _engine(yfv2, dev, cfg, coco_weights, max_batch=1, plan=plan)
    got = eng.detect_tiled(frames, tiles=tiles, conf_thres=0.3, iou_thres=0.4, out=_out(eng, 3))
    assert eng.max_batch >= len(tiles)                     # the tiles are the batch: max_batch grew
    td, tc = _tile_detections(eng, frames, tiles, 0.3, 0.4)
    want = _model(td, tc, tiles, 3, 0.4, 0, 300)
    _assert_same(got, want, str(plan))
    assert want[2][0] > 0


def test_pipeline_submit_tiled(yfv2, dev, cfg, coco_weights, images_u8):
    pipe = yfv2.DetectPipeline(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=16, depth=2, plan={})
    pipe.load_state_dict(coco_weights)
    ref = _engine(yfv2, dev, cfg, coco_weights, max_batch=16)
    frames = _three_frames(dev, images_u8, False)
    calls = [dict(include_full=True), dict(metric="ios", max_out=7, tile=(300, 500), overlap=(0, 17)), dict(merge_thres=0.2)]
    tickets = [pipe.submit_tiled(frames, 0.3, 0.4, **kw) for kw in calls]
    for t, kw in list(zip(tickets, calls))[1:]:            # depth 2: the first ticket's slot was reused by the third submit
        got = pipe.result(t)
        want = ref.detect_tiled(frames, conf_thres=0.3, iou_thres=0.4, **kw)
        assert tuple(got[0].shape) == (3, kw.get("max_out", 300), 6)
        assert torch.equal(got[2], want[2]) and int(got[2].sum()) > 0
        for f in range(3):
            n = int(got[2][f])
            assert torch.equal(got[1][f, :n], want[1][f, :n])
            assert torch.equal(got[0][f, :n].view(torch.int32), want[0][f, :n].view(torch.int32))
    with pytest.raises(RuntimeError):
        pipe.result(tickets[0])
    with pytest.raises(ValueError):
        pipe.submit_tiled(frames, 0.3, 0.4, tile=64, overlap=0)       # 11 x 16 + ... tiles: more than max_batch
    pipe.synchronize()


# ---- 5. errors before launch ------------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_tiled_argument_errors_launch_nothing(yfv2, dev, cfg, coco_weights, images_u8):
    from yolo_fastestv2_amd import _lib, tiling
    eng = _engine(yfv2, dev, cfg, coco_weights, max_batch=4)
    frame = torch.from_numpy(_picture(images_u8, 0, 480, 640, 3)).to(dev)
    small = torch.from_numpy(_picture(images_u8, 1, 200, 260, 4)).to(dev)
    frames = [frame, small]
    good = [(0, 0, 0, 352, 352), (0, 288, 128, 352, 352), (1, 0, 0, 260, 200)]
    out = _out(eng, 2)
    ref = eng.detect_tiled(frames, tiles=good, conf_thres=0.3, iou_thres=0.4)          # also allocates the workspaces
    ref = tuple(t.clone() for t in ref)
    torch.cuda.synchronize()
    L, h = _lib.lib(), eng._h
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    farr, keep = eng._frame_table(frames)

    def call(tiles, F=2, T=None, thres=0.4, metric=0, max_out=300, fr=farr, o=out):
        arr = tiling.tile_table(tiles)
        return L.yfv2_detect_tiled_u8(h, fr, F, arr, len(arr) if T is None else T, 0.3, 0.4, thres, metric, max_out, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), st)

    cases = [
        (dict(tiles=[(0, 289, 0, 352, 352)]), _lib.ERR_ARG, "inside"),                   # sticks out of the 640-wide frame by one pixel
        (dict(tiles=[(0, 0, 129, 352, 352)]), _lib.ERR_ARG, "inside"),                   # ... of the 480 rows by one
        (dict(tiles=[(0, -1, 0, 352, 352)]), _lib.ERR_ARG, "inside"),
        (dict(tiles=[(0, 0, 0, 0, 352)]), _lib.ERR_ARG, "inside"),
        (dict(tiles=[(1, 0, 0, 260, 200), (0, 0, 0, 352, 352)]), _lib.ERR_ARG, "decreases"),
        (dict(tiles=[(2, 0, 0, 100, 100)]), _lib.ERR_ARG, "outside [0, F)"),
        (dict(tiles=[(-1, 0, 0, 100, 100)]), _lib.ERR_ARG, "outside [0, F)"),
        (dict(tiles=good + [good[-1]] * 2), _lib.ERR_BATCH, "above max_batch=4"),        # five tiles on a handle for four
        (dict(tiles=good, max_out=0), _lib.ERR_ARG, "max_out"),
        (dict(tiles=good, max_out=4097), _lib.ERR_ARG, "max_out"),
        (dict(tiles=good, metric=2), _lib.ERR_ARG, "merge_metric"),
        (dict(tiles=good, metric=-1), _lib.ERR_ARG, "merge_metric"),
        (dict(tiles=good, thres=float("nan")), _lib.ERR_ARG, "finite"),
        (dict(tiles=good, thres=float("inf")), _lib.ERR_ARG, "finite"),
        (dict(tiles=good, T=0), _lib.ERR_ARG, "T must be"),
        (dict(tiles=good, F=0), _lib.ERR_ARG, "F must be"),
    ]
    for kw, code, msg in cases:
        rc = call(**kw)
        assert rc == code and msg in _lib.last_error(h), (kw, rc, _lib.last_error(h))
    bad_frames = (_lib.Frame * 2)()
    for i in range(2):
        bad_frames[i].data, bad_frames[i].height, bad_frames[i].width, bad_frames[i].row_pitch = farr[i].data, farr[i].height, farr[i].width, farr[i].row_pitch
    bad_frames[1].row_pitch = 3 * 260 - 1
    assert call(good, fr=bad_frames) == _lib.ERR_ARG and "row_pitch" in _lib.last_error(h)
    assert L.yfv2_detect_tiled_u8(h, farr, 2, tiling.tile_table(good), 3, 0.3, 0.4, 0.4, 0, 300, None, _ptr(out[1]), _ptr(out[2]), st) == _lib.ERR_ARG
    # the merge alone: the same checks
    td = torch.zeros((3, MAX_DET, 6), device=dev)
    tc = torch.zeros(3, dtype=torch.int32, device=dev)

    def merge(tiles=good, F=2, thres=0.4, metric=0, max_out=300, tdp=td):
        arr = tiling.tile_table(tiles)
        return L.yfv2_merge_tiles(h, _ptr(tdp) if tdp is not None else None, _ptr(tc), arr, len(arr), F, thres, metric, max_out, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), st)
    for kw, msg in ((dict(tiles=good[::-1]), "decreases"), (dict(F=1), "outside [0, F)"), (dict(max_out=0), "max_out"), (dict(max_out=4097), "max_out"),
                    (dict(metric=2), "merge_metric"), (dict(thres=float("nan")), "finite"), (dict(tdp=None), "null pointer")):
        assert merge(**kw) == _lib.ERR_ARG and msg in _lib.last_error(h), (kw, _lib.last_error(h))
    # ... and through the Python surface
    with pytest.raises(_lib.Yfv2Error) as e:
        eng.detect_tiled(frames, tiles=[(0, 289, 0, 352, 352)], conf_thres=0.3, iou_thres=0.4, out=out)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.Yfv2Error):
        eng.detect_tiled(frames, tiles=good, conf_thres=0.3, iou_thres=0.4, merge_thres=float("nan"), out=out)
    with pytest.raises(ValueError):
        eng.detect_tiled(frames, tiles=good, conf_thres=0.3, iou_thres=0.4, metric="giou", out=out)
    torch.cuda.synchronize()
    assert bool((out[0] == SENTINEL).all()) and bool((out[1] == SRC_FILL).all()) and bool((out[2] == CNT_FILL).all()), "a failed call wrote its output"
    # the engine is intact: the next valid call succeeds and repeats the first one's bits
    got = eng.detect_tiled(frames, tiles=good, conf_thres=0.3, iou_thres=0.4, out=out)
    assert torch.equal(got[2], ref[2]) and int(got[2].sum()) > 0
    for f in range(2):
        n = int(ref[2][f])
        assert torch.equal(got[1][f, :n], ref[1][f, :n]) and torch.equal(got[0][f, :n].view(torch.int32), ref[0][f, :n].view(torch.int32))
    assert bool((got[0][0, int(ref[2][0]):] == SENTINEL).all())
