"""GPU tests of the per-stream IoU tracker: Engine.track_update / tracking.Tracker (include/yfv2.h yfv2_track_update; DESIGN.md
4.18).  Run with ``-m gpu`` on an MI355X.

The claim: after every call the int32 state and every output equal the rule's numpy statement (tests/track_model.py, whose walk is
the rule as written) bit for bit - torch.equal, no tolerance anywhere; rows of the fresh outputs beyond fresh_count are not written;
bad arguments fail before anything is launched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import track_model as tm
from track_pair import F32, S_CNT, S_DETS, S_HITS, S_ID, S_SRC, Pair, _box, _frame, dev, eng, yfv2  # noqa: F401  (dev, eng, yfv2: the fixtures)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def test_lifecycle(yfv2, eng):
    """S = 1, M = 4, R = 8, max_misses 2, confirm_hits 3, by hand: birth; match; a miss kept for max_misses frames, then death; the
    freed slot reused in the same frame; ids never reused; confirm_hits reached exactly once"""
    p = Pair(yfv2, eng, 1, max_tracks=4, match_thres=0.3, max_misses=2, confirm_hits=3)
    R = 8
    o = p.step(*_frame([_box(0), _box(100), _box(200)], R))                       # three births
    assert o["track_id"][0].tolist() == [1, 2, 3, 0, 0, 0, 0, 0] and p.header() == [3, 3, 1, 3, 0, 0]
    o = p.step(*_frame([_box(201), _box(1), _box(300)], R))                       # tracks 3 and 1 matched in another row order, 2 misses, 4 born
    assert o["track_id"][0].tolist() == [3, 1, 4, 0, 0, 0, 0, 0] and o["track_hits"][0].tolist() == [2, 2, 1, 0, 0, 0, 0, 0]
    assert p.header() == [4, 4, 2, 4, 0, 0] and o["fresh_count"][0] == 0
    o = p.step(*_frame([_box(2), _box(202), _box(301), _box(400)], R))            # 1 and 3 confirmed; the table is full: a dropped birth
    assert o["track_id"][0].tolist() == [1, 3, 4, 0, 0, 0, 0, 0] and o["fresh_count"][0] == 2 and o["fresh_src"][0, :2].tolist() == [0, 1]
    assert p.header() == [4, 4, 3, 4, 0, 1]
    o = p.step(*_frame([_box(3), _box(203), _box(302), _box(400)], R))            # track 2's third miss: it dies, and (400) takes its slot at once
    assert o["track_id"][0].tolist() == [1, 3, 4, 5, 0, 0, 0, 0] and o["track_hits"][0].tolist() == [4, 4, 3, 1, 0, 0, 0, 0]
    assert p.header() == [5, 4, 4, 5, 1, 1]
    assert o["fresh_count"][0] == 1 and o["fresh_src"][0, 0] == 2                 # track 4 is fresh now; 1 and 3 were, once
    slots = p.model.state[0, tm.HEADER:].reshape(4, tm.SLOT)
    assert slots[:, 6].tolist() == [1, 5, 3, 4]                                   # id 5 sits in the slot id 2 left
    o = p.step(*_frame([], R))                                                    # an empty frame: everyone misses
    assert p.header() == [5, 4, 5, 5, 1, 1] and not o["track_id"].any()
    o = p.step(*_frame([_box(4)], R))                                             # a track comes back after a miss: hits go on, misses restart
    assert o["track_id"][0, 0] == 1 and o["track_hits"][0, 0] == 5
    p.step(*_frame([_box(5)], R))
    o = p.step(*_frame([_box(6), _box(204)], R))                                  # 3, 4 and 5 have died of three misses; (204) is a NEW track
    assert o["track_id"][0].tolist()[:2] == [1, 6] and p.header() == [6, 2, 8, 6, 4, 1]
    # the Tracker's views of the same state
    tr = p.tracker
    assert tr.header(0) == dict(issued=6, live=2, frames=8, births=6, deaths=4, dropped=1)
    t = tr.tracks(0)
    assert t["id"].tolist() == [1, 6] and t["hits"].tolist() == [7, 1] and t["box"].cpu().tolist() == [[6, 0, 16, 10], [204, 0, 214, 10]]
    tr.reset(0)
    assert not tr.state.any() and tr.header(0)["issued"] == 0


def test_max_misses_zero(yfv2, eng):
    """a track that is not seen dies in that very frame, and its slot is free for that frame's births"""
    p = Pair(yfv2, eng, 1, max_tracks=2, match_thres=0.3, max_misses=0, confirm_hits=1)
    o = p.step(*_frame([_box(0), _box(100)], 4))
    assert o["fresh_count"][0] == 2                                               # confirm_hits 1: fresh at birth
    o = p.step(*_frame([_box(1), _box(200), _box(300)], 4))
    assert o["track_id"][0].tolist() == [1, 3, 0, 0] and p.header() == [3, 2, 2, 3, 1, 1]
    p.step(*_frame([], 4))
    assert p.header() == [3, 0, 3, 3, 3, 1] and not p.model.state[0, tm.HEADER:].any()


def test_ties(yfv2, eng):
    """equal IoUs are decided by the order: the lower row, then the lower slot"""
    # two rows with equal IoU to one track: the first row takes it, the second starts a track
    p = Pair(yfv2, eng, 1, max_tracks=4, match_thres=0.3, confirm_hits=2)
    p.step(*_frame([_box(10)], 4))
    o = p.step(*_frame([_box(12), _box(8)], 4))
    assert o["track_id"][0].tolist()[:2] == [1, 2]
    # two tracks with equal IoU to one row: the lower slot takes it
    p = Pair(yfv2, eng, 1, max_tracks=4, match_thres=0.3, confirm_hits=2)
    p.step(*_frame([_box(8), _box(12)], 4))
    o = p.step(*_frame([_box(10)], 4))
    assert o["track_id"][0, 0] == 1 and p.model.state[0, tm.HEADER:].reshape(4, tm.SLOT)[:, 8].tolist() == [0, 1, 0, 0]
    # both: rows at 10 and 14, tracks at 8, 12, 16.  Every edge has IoU 2/3; (row 0, slot 0), then (row 1, slot 1); track 3 misses
    p = Pair(yfv2, eng, 1, max_tracks=4, match_thres=0.3, confirm_hits=2)
    p.step(*_frame([_box(8), _box(12), _box(16)], 4))
    o = p.step(*_frame([_box(10), _box(14)], 4))
    assert o["track_id"][0].tolist()[:2] == [1, 2] and o["fresh_count"][0] == 2
    # the case that tells a slot's best row over all rows from its best among the rows that named it (tests/test_track_host.py)
    p = Pair(yfv2, eng, 1, max_tracks=2, match_thres=0.2, confirm_hits=2)
    p.step(*_frame([_box(0), _box(6)], 4))
    o = p.step(*_frame([_box(1), _box(2), _box(12)], 4))
    assert o["track_id"][0].tolist()[:3] == [1, 2, 0] and p.header()[5] == 1


def test_class_awareness(yfv2, eng):
    """a class flicker breaks a track with class_aware, and without it the track's class follows the row's"""
    p = Pair(yfv2, eng, 1, max_tracks=4, match_thres=0.3, class_aware=True)
    p.step(*_frame([_box(0, cls=3.0)], 4))
    o = p.step(*_frame([_box(1, cls=5.0)], 4))
    assert o["track_id"][0, 0] == 2 and p.header()[:2] == [2, 2]
    p = Pair(yfv2, eng, 1, max_tracks=4, match_thres=0.3, class_aware=False)
    p.step(*_frame([_box(0, cls=3.0)], 4))
    o = p.step(*_frame([_box(1, cls=5.0)], 4))
    assert o["track_id"][0, 0] == 1 and p.header()[:2] == [1, 1]
    assert p.tracker.tracks(0)["cls"].tolist() == [5.0]


def _sequence(calls=20, S=5, R=32, objects=20, seed=3):
    """random walks of `objects` boxes per stream; every call a changing subset of the streams, rows in a random order with random
    confs, some rows broken, some counts 0, negative or beyond R"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 300, (S, objects, 2))
    size = rng.uniform(20, 60, (S, objects, 2))
    cls = rng.integers(0, 3, (S, objects)).astype(F32)
    out = []
    for t in range(calls):
        streams = sorted(rng.choice(S, int(rng.integers(1, S + 1)), replace=False).tolist(), key=lambda s: (s * 7 + t) % S)
        dets = np.zeros((len(streams), R, 6), F32)
        count = np.zeros(len(streams), np.int32)
        for b, s in enumerate(streams):
            pos[s] += rng.uniform(-4, 4, (objects, 2))
            seen = rng.permutation(objects)[:int(rng.integers(objects // 2, objects + 1))]
            rows = np.concatenate([pos[s, seen], pos[s, seen] + size[s, seen], rng.uniform(0.2, 1.0, (len(seen), 1)), cls[s, seen, None]], axis=1).astype(F32)
            flick = rng.random(len(seen)) < 0.05
            rows[flick, 5] += 1.0                                   # a class flicker
            for r in np.nonzero(rng.random(len(seen)) < 0.12)[0]:   # broken rows
                kind = int(rng.integers(0, 5))
                if kind == 0: rows[r, rng.integers(0, 4)] = NAN
                elif kind == 1: rows[r, rng.integers(0, 4)] = rng.choice([INF, -INF])
                elif kind == 2: rows[r, 4] = NAN
                elif kind == 3: rows[r, 2] = rows[r, 0]             # x2 == x1
                else: rows[r, 2] = rows[r, 0] - 5.0                 # x2 < x1
            dets[b] = np.array([700.0, 700.0, 730.0, 730.0, 0.95, 1.0], F32)   # beyond the count: valid rows that must not be read
            dets[b, :len(rows)] = rows
            count[b] = len(rows)
            odd = rng.random()
            if odd < 0.08: count[b] = 0
            elif odd < 0.16: count[b] = -3
            elif odd < 0.24: count[b] = R + 9                       # every row of the frame, the filler included
        out.append((dets, count, streams))
    return out


def test_sequence_of_batches(yfv2, eng):
    """S = 5, M = 16 (the table fills and `dropped` counts), R = 32, 20 calls; compared after every call; the same sequence one frame
    per call leaves the same bits"""
    rule = dict(max_tracks=16, match_thres=0.3, class_aware=True, init_conf=0.4, max_misses=2, confirm_hits=3)
    seq = _sequence()
    p = Pair(yfv2, eng, 5, **rule)
    fresh_total = 0
    for dets, count, streams in seq:
        fresh_total += int(p.step(dets, count, streams)["fresh_count"].sum())
    head = p.model.state[:, :6]
    assert (head[:, 5] > 0).all() and (head[:, 4] > 0).all() and (head[:, 1] == 16).any() and fresh_total > 20, head      # dropped, deaths, a full table
    assert {int(c) for _d, cnt, _s in seq for c in cnt} >= {0, -3, 41}
    q = Pair(yfv2, eng, 5, **rule)
    for dets, count, streams in seq:
        for b, s in enumerate(streams):
            q.step(dets[b:b + 1], count[b:b + 1], [s], fresh=b % 2 == 0)
    assert torch.equal(q.tracker.state, p.tracker.state)


def test_chain_needs_a_round_per_pair(yfv2, eng):
    """the adversarial input of the rounds (tests/track_model.py chain_case): 40 pairs, every edge but the last with a heavier
    neighbour, one pair per round"""
    tracks, rows = tm.chain_case(40)
    p = Pair(yfv2, eng, 1, max_tracks=64, match_thres=0.1, confirm_hits=2)
    d = np.zeros((1, 48, 6), F32)
    d[0, :40] = tracks
    p.step(d, [40])
    d[0, :40] = rows
    o = p.step(d, [40])
    assert o["track_id"][0, :40].tolist() == list(range(1, 41)) and o["fresh_count"][0] == 40 and p.header() == [40, 40, 2, 40, 0, 0]


def test_limits(yfv2, eng):
    """one stream at R = 4096, M = 1024: 400 tracks, then a full frame - the tracks drifted and in another order among 3696 other rows,
    which fill the table and are dropped beyond it"""
    rng = np.random.default_rng(9)
    R, M = 4096, 1024
    cells = rng.permutation(80 * 80)[:R]                                          # one box per cell of a grid: no two overlap
    xy = np.stack([cells % 80, cells // 80], axis=1) * 50.0
    wh = rng.uniform(20, 40, (R, 2))
    rows = np.concatenate([xy, xy + wh, rng.uniform(0.3, 1.0, (R, 1)), rng.integers(0, 4, (R, 1))], axis=1).astype(F32)
    rows[:400, 4] = np.maximum(rows[:400, 4], F32(0.5))                            # the first frame's rows all start a track
    p = Pair(yfv2, eng, 1, max_tracks=M, match_thres=0.3, init_conf=0.35, confirm_hits=2)
    first = np.zeros((1, R, 6), F32)
    first[0, :400] = rows[:400]
    o = p.step(first, [400])
    assert p.header() == [400, 400, 1, 400, 0, 0]
    moved = rows.copy()
    moved[:, :4] += np.tile(rng.uniform(-3, 3, (R, 2)), 2).astype(F32)
    perm = rng.permutation(R)
    o = p.step(moved[perm][None], [R])
    head = p.header()
    assert head[:2] == [M, M] and head[3] == M and head[5] > 2000 and head[4] == 0 and o["fresh_count"][0] == 400, head
    assert sorted(o["track_id"][0][o["track_hits"][0] == 2].tolist()) == list(range(1, 401))


def test_many_frames_in_one_call(yfv2, eng):
    """more frames than one launch carries (768): the second launch's frames and streams are addressed like the first's"""
    B, R = 800, 4
    rng = np.random.default_rng(2)
    streams = rng.permutation(B).tolist()
    d = np.zeros((B, R, 6), F32)
    d[:, 0] = np.concatenate([rng.uniform(0, 50, (B, 2)), rng.uniform(60, 90, (B, 2)), np.full((B, 1), 0.9), np.zeros((B, 1))], axis=1)
    p = Pair(yfv2, eng, B, max_tracks=2, confirm_hits=2)
    p.step(d, np.ones(B, np.int32), streams)
    o = p.step(d, np.ones(B, np.int32), streams)
    assert (o["fresh_count"] == 1).all() and (p.model.state[:, 0] == 1).all()


def test_argument_errors_launch_nothing(yfv2, eng, dev):
    from yolo_fastestv2_amd import _lib
    L = _lib.lib()
    B, R, S, M = 2, 8, 3, 4
    words = 8 + 10 * M
    state = torch.full((S, words), 0x5A5A5A5, device=dev, dtype=torch.int32)
    d = torch.zeros((B, R, 6), device=dev)
    c = torch.full((B,), 3, device=dev, dtype=torch.int32)
    outs = (torch.full((B, R), S_ID, device=dev, dtype=torch.int32), torch.full((B, R), S_HITS, device=dev, dtype=torch.int32),
            torch.full((B, R, 6), S_DETS, device=dev), torch.full((B, R), S_SRC, device=dev, dtype=torch.int32), torch.full((B,), S_CNT, device=dev, dtype=torch.int32))
    good = dict(h=eng._h, dets=d.data_ptr(), count=c.data_ptr(), R=R, B=B, streams=[0, 2], state=state.data_ptr(), S=S, rule=True,
                tid=outs[0].data_ptr(), hits=outs[1].data_ptr(), fd=outs[2].data_ptr(), fs=outs[3].data_ptr(), fc=outs[4].data_ptr())

    def call(rule_kw=None, **over):
        a = dict(good, **over)
        r = _lib.TrackRule()
        r.max_tracks, r.match_thres, r.class_aware, r.init_conf, r.max_misses, r.confirm_hits = M, 0.3, 1, 0.0, 30, 3
        for k, v in (rule_kw or {}).items():
            setattr(r, k, v)
        arr = (C.c_int32 * max(len(a["streams"]), 1))(*a["streams"]) if a["streams"] is not None else None
        return L.yfv2_track_update(a["h"], a["dets"], a["count"], a["R"], a["B"], arr, a["state"], a["S"], C.byref(r) if a["rule"] else None,
                                   a["tid"], a["hits"], a["fd"], a["fs"], a["fc"], None)

    cases = [
        ("null dets", dict(dets=None)), ("null count", dict(count=None)), ("null streams", dict(streams=None)), ("null state", dict(state=None)),
        ("null rule", dict(rule=False)), ("null track_id", dict(tid=None)),
        ("B < 1", dict(B=0)), ("S < 1", dict(S=0)), ("R < 1", dict(R=0)), ("R > 4096", dict(R=4097)),
        ("M < 1", dict(rule_kw={"max_tracks": 0})), ("M > 1024", dict(rule_kw={"max_tracks": 1025})),
        ("stream >= S", dict(streams=[0, 3])), ("stream < 0", dict(streams=[-1, 1])), ("stream twice", dict(streams=[1, 1])),
        ("thres NaN", dict(rule_kw={"match_thres": NAN})), ("thres inf", dict(rule_kw={"match_thres": INF})), ("thres < 0", dict(rule_kw={"match_thres": -0.1})),
        ("init_conf NaN", dict(rule_kw={"init_conf": NAN})), ("max_misses < 0", dict(rule_kw={"max_misses": -1})),
        ("confirm_hits < 1", dict(rule_kw={"confirm_hits": 0})),
        ("fresh: dets alone", dict(fs=None, fc=None)), ("fresh: no count", dict(fc=None)), ("fresh: no dets", dict(fd=None)), ("fresh: no src", dict(fs=None)),
    ]
    for what, kw in cases:
        rule_kw = kw.pop("rule_kw", None)
        assert call(rule_kw, **kw) == _lib.ERR_ARG, what
        assert "yfv2_track_update" in _lib.last_error(eng._h), what
    assert call(h=None) == _lib.ERR_ARG
    torch.cuda.synchronize(dev)
    assert (state == 0x5A5A5A5).all()
    for t, v in zip(outs, (S_ID, S_HITS, S_DETS, S_SRC, S_CNT)):
        assert (t == v).all()
    # what is allowed: track_hits and the fresh outputs left out, infinite init_conf, the bounds themselves
    state.zero_()
    assert call(hits=None, fd=None, fs=None, fc=None, rule_kw={"init_conf": INF, "max_misses": 0, "confirm_hits": 1, "match_thres": 0.0}) == 0
    torch.cuda.synchronize(dev)
    assert (outs[0] == 0).all() and (outs[1] == S_HITS).all() and state[[0, 2], 2].tolist() == [1, 1] and state[1].eq(0).all()
    # Engine-level validation
    tr = yfv2.Tracker(eng, S, max_tracks=M)
    with pytest.raises(ValueError):
        tr.update(d, c.to(torch.int64))
    with pytest.raises(ValueError):
        tr.update(d[:, :, :5].contiguous(), c)
    with pytest.raises(ValueError):
        tr.update(d, c, streams=[0])
    with pytest.raises(ValueError):
        eng.track_update(d, c, [0, 1], tr.state[:, :-1].contiguous(), M)
    with pytest.raises(ValueError):
        tr.update(d, c, out=outs[:1])
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, 0)
    with pytest.raises(yfv2.Yfv2Error):
        tr.update(d, c, streams=[1, 1])
    assert not tr.state.any()


def test_cascade(yfv2, dev, cfg, coco_weights, images_u8):
    """detect_frames -> Tracker.update(fresh=True) -> crop_detections, the host never learning a box: three frames per stream, each the
    picture before it moved by a few pixels; the fresh rows equal the model's, and their crops equal the crops of the model's rows"""
    det = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=8, plan={})
    det.load_state_dict(coco_weights)
    S = min(4, len(images_u8))
    base = [np.ascontiguousarray(images_u8[k].transpose(1, 2, 0)) for k in range(S)]
    rule = dict(max_tracks=64, match_thres=0.3, confirm_hits=2)
    tr, model = yfv2.Tracker(det, S, **rule), tm.Model(S, **rule)
    fresh_total = 0
    for t in range(3):
        host = [np.ascontiguousarray(np.roll(f, (2 * t, 3 * t), axis=(0, 1))) for f in base]
        frames = [torch.from_numpy(f).to(dev) for f in host]
        dets, _idx, cnt = det.detect_frames(frames, 0.3, 0.4)
        tid, hits, fdets, fsrc, fcnt = tr.update(dets, cnt, fresh=True)
        want = model.update(dets.cpu().numpy(), cnt.cpu().numpy())
        assert torch.equal(tr.state.cpu(), torch.from_numpy(model.state))
        assert torch.equal(tid.cpu(), torch.from_numpy(want["track_id"])) and torch.equal(hits.cpu(), torch.from_numpy(want["track_hits"]))
        assert torch.equal(fcnt.cpu(), torch.from_numpy(want["fresh_count"]))
        wdets = torch.from_numpy(want["fresh_dets"]).to(dev)
        for b in range(S):
            k = int(want["fresh_count"][b])
            assert torch.equal(fdets[b, :k], wdets[b, :k]) and torch.equal(fsrc[b, :k].cpu(), torch.from_numpy(want["fresh_src"][b, :k]))
        fresh_total += int(want["fresh_count"].sum())
        got = det.crop_detections(frames, fdets, fcnt, (32, 32), pad=0.1)
        ref = det.crop_detections(frames, wdets, torch.from_numpy(want["fresh_count"]).to(dev), (32, 32), pad=0.1)
        live = int(ref[3][-1])                              # at most the fresh rows: a box outside its frame has no crop
        assert 0 < live <= int(want["fresh_count"].sum()) or int(want["fresh_count"].sum()) == 0
        assert torch.equal(got[3], ref[3]) and torch.equal(got[4], ref[4])
        for g, r in zip(got[:3], ref[:3]):
            assert torch.equal(g[:live], r[:live])
    assert fresh_total > 0 and int(model.state[:, 0].sum()) >= fresh_total
    det.close()
