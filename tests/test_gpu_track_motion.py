"""GPU tests of the tracker's motion form: Engine.track_update_motion / tracking.Tracker(motion=...) (include/yfv2.h
yfv2_track_update_motion).  Run with ``-m gpu`` on an MI355X.

The claim: after every call the int32 state - the filter words included - and every output (track_box too) equal the rule's numpy
statement (tests/track_motion_model.py) bit for bit - torch.equal on int32 views, no tolerance anywhere; rows of the fresh outputs
beyond fresh_count are not written; bad arguments fail before anything is launched; and the plain form, now an instantiation of the
same kernel template, still equals tests/track_model.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import track_model as tm
import track_motion_model as mm
import track_pair
from track_pair import F32, S_BOX, S_CNT, S_DETS, S_HITS, S_ID, S_SRC, _box, _frame, dev, eng, yfv2  # noqa: F401  (dev, eng, yfv2: the fixtures)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")

Pair = functools.partial(track_pair.Pair, motion=True)          # every tracker of this file has a motion model; motion=dict(...) sets its scales


def test_lifecycle(yfv2, eng):
    """R = 4, M = 2, max_misses 1: births, matches of moving boxes, a coast, a death, the freed slot reused in the same frame"""
    p = Pair(yfv2, eng, 1, max_tracks=2, match_thres=0.3, max_misses=1, confirm_hits=2)
    o = p.step(*_frame([_box(0), _box(100)], 4))                                  # two births: the born state's corners are the rows
    assert o["track_id"][0].tolist() == [1, 2, 0, 0] and p.header() == [2, 2, 1, 2, 0, 0]
    assert o["track_box"][0, :2].tolist() == [[0, 0, 10, 10], [100, 0, 110, 10]] and not o["track_box"][0, 2:].any()
    o = p.step(*_frame([_box(103), _box(2), _box(200)], 4))                       # both matched in the other order; the table is full
    assert o["track_id"][0].tolist() == [2, 1, 0, 0] and o["fresh_count"][0] == 2 and p.header() == [2, 2, 2, 2, 0, 1]
    assert p.model.filters()[0, 0, mm.V] > 0 and 0 < o["track_box"][0, 1, 0] < 2   # the filtered box lies between prediction and row
    o = p.step(*_frame([_box(4)], 4))                                             # track 2 coasts: its filter moves on, its last row stays
    assert o["track_id"][0].tolist() == [1, 0, 0, 0] and p.slots()[1, 8] == 1
    assert p.slots()[1, :4].view(F32).tolist() == [103, 0, 113, 10] and p.model.filters()[1, 0, mm.X] > 108
    o = p.step(*_frame([_box(6), _box(300)], 4))                                  # track 2 dies of its second miss; (300) takes its slot at once
    assert o["track_id"][0].tolist() == [1, 3, 0, 0] and p.header() == [3, 2, 4, 3, 1, 1]
    assert p.slots()[:, 6].tolist() == [1, 3] and p.model.filters()[1, 0].tolist()[:2] == [305, 0]
    # the Tracker's views of the same state
    t = p.tracker.tracks(0)
    assert t["id"].tolist() == [1, 3] and t["box"].cpu().tolist() == [[6, 0, 16, 10], [300, 0, 310, 10]]
    assert torch.equal(t["pred"].cpu(), torch.from_numpy(mm.corners(p.model.filters()))) and torch.equal(t["vel"].cpu(), torch.from_numpy(p.model.filters()[:, :, mm.V].copy()))
    p.tracker.reset()
    assert not p.tracker.state.any()


def test_occlusion_keeps_the_id(yfv2, eng):
    """a 64 x 64 box moving 8 px / frame, seen for 10 frames, missing for 6, seen again: one id, fresh once - and the plain form on
    the same rows issues a second id (tests/test_track_motion_host.py has the figures)"""
    p = Pair(yfv2, eng, 1, max_tracks=4, confirm_hits=1)
    plain = yfv2.Tracker(eng, 1, max_tracks=4, confirm_hits=1)
    ids, ids_plain, fresh = [], [], 0
    for d, c in mm.occlusion_case():
        o = p.step(d, c)
        ids.append(int(o["track_id"][0, 0]))
        fresh += int(o["fresh_count"][0])
        ids_plain.append(int(plain.update(torch.from_numpy(d).to(p.dev), torch.from_numpy(c).to(p.dev))[0][0, 0]))
    assert ids == [1] * 10 + [0] * 6 + [1] and fresh == 1
    assert ids_plain == [1] * 10 + [0] * 6 + [2]


def _walks(rng, S, objects):
    pos = rng.uniform(0, 600, (S, objects, 2))
    vel = rng.uniform(-6, 6, (S, objects, 2))
    size = rng.uniform(20, 60, (S, objects, 2))
    cls = rng.integers(0, 3, (S, objects)).astype(F32)
    return pos, vel, size, cls


def _rows_of(rng, pos, size, cls, seen):
    return np.concatenate([pos[seen], pos[seen] + size[seen], rng.uniform(0.2, 1.0, (len(seen), 1)), cls[seen, None]], axis=1).astype(F32)


def test_streams_permuted_and_one_skipped(yfv2, eng):
    """3 streams given in another order every call; stream 1 is absent from the middle calls and is not advanced by them"""
    rng = np.random.default_rng(4)
    S, R, objects = 3, 16, 10
    pos, vel, size, cls = _walks(rng, S, objects)
    p = Pair(yfv2, eng, S, max_tracks=16, max_misses=2, confirm_hits=2)
    for t in range(6):
        streams = [[2, 0, 1], [1, 2, 0], [2, 0], [0, 2], [0, 1, 2], [1, 0, 2]][t]
        dets, count = np.zeros((len(streams), R, 6), F32), np.zeros(len(streams), np.int32)
        before = p.model.state[1].copy()
        for b, s in enumerate(streams):
            pos[s] += vel[s]
            seen = rng.permutation(objects)[:int(rng.integers(6, objects + 1))]
            dets[b, :len(seen)] = _rows_of(rng, pos[s], size[s], cls[s], seen)
            count[b] = len(seen)
        p.step(dets, count, streams)
        if 1 not in streams:
            assert np.array_equal(p.model.state[1], before) and p.model.state[1, 2] == 2
    assert p.model.state[:, 2].tolist() == [6, 4, 6] and (p.model.state[:, 1] > 5).all()


def test_random_walks_with_dropouts(yfv2, eng):
    """R = 300, M = 64 (the table fills: dropped births), seeded constant-velocity walks with jitter, a fifth of the objects unseen in
    each frame, rows in a new order, some rows broken, 12 frames; the same sequence with mutual_best leaves the model the same bits"""
    rng = np.random.default_rng(6)
    R, objects = 300, 90
    pos, vel, size, cls = _walks(rng, 1, objects)
    p = Pair(yfv2, eng, 1, max_tracks=64, init_conf=0.3, max_misses=3, confirm_hits=3)
    par = mm.Model(1, max_tracks=64, init_conf=0.3, max_misses=3, confirm_hits=3)
    moving = 0
    for t in range(12):
        pos[0] += vel[0] + rng.uniform(-1, 1, (objects, 2))
        seen = rng.permutation(objects)[:int(objects * 0.8)]
        rows = _rows_of(rng, pos[0], size[0], cls[0], seen)
        for r in np.nonzero(rng.random(len(seen)) < 0.06)[0]:
            rows[r, int(rng.integers(0, 4))] = (NAN, INF, -INF, 3e38)[int(rng.integers(0, 4))]
        d = np.tile(np.array([2000.0, 2000.0, 2030.0, 2030.0, 0.95, 1.0], F32), (1, R, 1))    # beyond the count: valid rows that must not be read
        d[0, :len(rows)] = rows
        o = p.step(d, [len(rows)])
        par.update(d, [len(rows)], match=tm.mutual_best)
        moving += int((o["track_hits"][0] >= 3).sum())
    assert np.array_equal(par.state, p.model.state)
    head = p.header()
    assert head[1] == 64 and head[5] > 50 and head[4] > 0 and moving > 200, (head, moving)   # a full table, dropped births, deaths, long tracks


def test_limits(yfv2, eng):
    """R = 4096, M = 1024 (the LDS maximum): 400 tracks are born, then a full frame in which they have moved, among 3696 other rows"""
    rng = np.random.default_rng(9)
    R, M = 4096, 1024
    cells = rng.permutation(80 * 80)[:R]                                          # one box per cell of a grid: no two overlap
    xy = np.stack([cells % 80, cells // 80], axis=1) * 50.0
    wh = rng.uniform(20, 40, (R, 2))
    rows = np.concatenate([xy, xy + wh, rng.uniform(0.3, 1.0, (R, 1)), rng.integers(0, 4, (R, 1))], axis=1).astype(F32)
    rows[:400, 4] = np.maximum(rows[:400, 4], F32(0.5))
    p = Pair(yfv2, eng, 1, max_tracks=M, match_thres=0.3, init_conf=0.35, confirm_hits=2)
    first = np.zeros((1, R, 6), F32)
    first[0, :400] = rows[:400]
    p.step(first, [400])
    assert p.header() == [400, 400, 1, 400, 0, 0]
    moved = rows.copy()
    moved[:, :4] += np.tile(rng.uniform(-3, 3, (R, 2)), 2).astype(F32)
    perm = rng.permutation(R)
    o = p.step(moved[perm][None], [R])
    head = p.header()
    assert head[:2] == [M, M] and head[3] == M and head[5] > 2000 and head[4] == 0 and o["fresh_count"][0] == 400, head
    assert sorted(o["track_id"][0][o["track_hits"][0] == 2].tolist()) == list(range(1, 401))
    assert p.model.filters()[:, :2, mm.V].any()                                    # the matched tracks learnt a velocity


def test_launch_split(yfv2, eng):
    """B = 769, R = 2, M = 1: one frame more than a launch carries; the second launch's frame, stream and track_box are addressed
    like the first's"""
    B, R = 769, 2
    rng = np.random.default_rng(2)
    streams = rng.permutation(B).tolist()
    d = np.zeros((B, R, 6), F32)
    d[:, 0] = np.concatenate([rng.uniform(0, 50, (B, 2)), rng.uniform(60, 90, (B, 2)), np.full((B, 1), 0.9), np.zeros((B, 1))], axis=1)
    p = Pair(yfv2, eng, B, max_tracks=1, confirm_hits=2)
    p.step(d, np.ones(B, np.int32), streams)
    d[:, 0, :4] += F32(3.0)
    o = p.step(d, np.ones(B, np.int32), streams)
    assert (o["fresh_count"] == 1).all() and (p.model.state[:, 0] == 1).all() and o["track_box"][768, 0].all()


def test_extreme_scales(yfv2, eng):
    """coordinates near 1e30 (squares overflow: infinite covariances, blind slots, NaN gains) and boxes 2^-70 wide (subnormal
    covariances) beside ordinary ones, for four frames; every bit of the state must still be the model's"""
    tiny = F32(2.0 ** -70)
    rows = [[1e30, 1e30, 1.5e30, 1.4e30, 0.9, 0.0], [-2e30, 0.0, -1e30, 3e30, 0.9, 1.0],
            [0.0, 0.0, tiny, tiny, 0.9, 2.0], [1.0, 1.0, 1.0 + 2.0 ** -20, 1.0 + 2.0 ** -20, 0.9, 2.0],
            [tiny, -tiny, 3 * tiny, tiny, 0.9, 0.0], [2.0 ** -80, 0.0, 2.0 ** -79, 2.0 ** -80, 0.9, 0.0],
            _box(50), _box(3e18, 0.0, 2e19, 2e19)]
    p = Pair(yfv2, eng, 1, max_tracks=8, max_misses=1, confirm_hits=2)
    seen_sub = seen_nonfinite = blind = False
    for t in range(4):
        f = F32(1.0 + 0.03 * t)
        d = np.array(rows, F32)
        with np.errstate(all="ignore"):
            d[:, :4] *= f
        o = p.step(d[None], [len(rows)])
        filt = p.model.filters()
        with np.errstate(all="ignore"):
            seen_sub |= bool(((np.abs(filt) > 0) & (np.abs(filt) < F32(1.17549435e-38))).any())
            seen_nonfinite |= bool((~np.isfinite(filt)).any())
        blind |= bool(p.header()[4] > 0)
    assert seen_sub and seen_nonfinite and blind, (seen_sub, seen_nonfinite, blind)


def test_nan_and_inf_rows(yfv2, eng):
    """broken rows never match and never start a track - also the rows that are finite themselves but whose measurement is not"""
    p = Pair(yfv2, eng, 1, max_tracks=8, confirm_hits=2)
    good = _box(10)
    bad = [[NAN, 0, 10, 10, 0.9, 0], [0, 0, INF, 10, 0.9, 0], [0, -INF, 10, 10, 0.9, 0], [0, 0, 10, 10, NAN, 0], [0, 0, 10, 10, 0.9, NAN],
           [-3e38, 0, 3e38, 10, 0.9, 0],                    # x2 - x1 overflows
           [3e38, 0, 3.2e38, 10, 0.9, 0],                   # x1 + x2 overflows
           [0, 2e38, 10, 3.4e38, 0.9, 0]]                   # y1 + y2 overflows
    o = p.step(*_frame([good] + bad, 12))
    assert o["track_id"][0].tolist() == [1] + [0] * 11 and p.header() == [1, 1, 1, 1, 0, 0]
    o = p.step(*_frame(bad + [_box(11)], 12))
    assert o["track_id"][0].tolist() == [0] * 8 + [1, 0, 0, 0] and p.header() == [1, 1, 2, 1, 0, 0] and o["fresh_count"][0] == 1


def test_optional_outputs_absent(yfv2, eng):
    """track_box = NULL, the fresh outputs absent, both: the state and the other outputs are the same bits"""
    seq = mm.occlusion_case(seen=4, hidden=2)
    ps = [Pair(yfv2, eng, 1, max_tracks=4, confirm_hits=2) for _ in range(4)]
    for d, c in seq:
        for p, (fresh, box) in zip(ps, ((True, True), (True, False), (False, True), (False, False))):
            p.step(d, c, fresh=fresh, box=box)
    for p in ps[1:]:
        assert torch.equal(p.tracker.state, ps[0].tracker.state)


def test_argument_errors_launch_nothing(yfv2, eng, dev):
    from yolo_fastestv2_amd import _lib
    L = _lib.lib()
    B, R, S, M = 2, 8, 3, 4
    words = 8 + 32 * M
    state = torch.full((S, words), 0x5A5A5A5, device=dev, dtype=torch.int32)
    d = torch.zeros((B, R, 6), device=dev)
    c = torch.full((B,), 3, device=dev, dtype=torch.int32)
    outs = (torch.full((B, R), S_ID, device=dev, dtype=torch.int32), torch.full((B, R), S_HITS, device=dev, dtype=torch.int32),
            torch.full((B, R, 6), S_DETS, device=dev), torch.full((B, R), S_SRC, device=dev, dtype=torch.int32), torch.full((B,), S_CNT, device=dev, dtype=torch.int32),
            torch.full((B, R, 4), S_BOX, device=dev))
    good = dict(h=eng._h, dets=d.data_ptr(), count=c.data_ptr(), R=R, B=B, streams=[0, 2], state=state.data_ptr(), S=S, rule=True, motion=(0.05, 0.00625, 0.05),
                tid=outs[0].data_ptr(), hits=outs[1].data_ptr(), fd=outs[2].data_ptr(), fs=outs[3].data_ptr(), fc=outs[4].data_ptr(), box=outs[5].data_ptr())

    def call(rule_kw=None, **over):
        a = dict(good, **over)
        r = _lib.TrackRule()
        r.max_tracks, r.match_thres, r.class_aware, r.init_conf, r.max_misses, r.confirm_hits = M, 0.3, 1, 0.0, 30, 3
        for k, v in (rule_kw or {}).items():
            setattr(r, k, v)
        arr = (C.c_int32 * max(len(a["streams"]), 1))(*a["streams"]) if a["streams"] is not None else None
        mo = C.byref(_lib.TrackMotion(*a["motion"])) if a["motion"] is not None else None
        return L.yfv2_track_update_motion(a["h"], a["dets"], a["count"], a["R"], a["B"], arr, a["state"], a["S"], C.byref(r) if a["rule"] else None, mo,
                                          a["tid"], a["hits"], a["box"], a["fd"], a["fs"], a["fc"], None)

    cases = [
        ("null dets", dict(dets=None)), ("null count", dict(count=None)), ("null streams", dict(streams=None)), ("null state", dict(state=None)),
        ("null rule", dict(rule=False)), ("null track_id", dict(tid=None)), ("null motion", dict(motion=None)),
        ("B < 1", dict(B=0)), ("S < 1", dict(S=0)), ("R < 1", dict(R=0)), ("R > 4096", dict(R=4097)),
        ("M < 1", dict(rule_kw={"max_tracks": 0})), ("M > 1024", dict(rule_kw={"max_tracks": 1025})),
        ("stream >= S", dict(streams=[0, 3])), ("stream < 0", dict(streams=[-1, 1])), ("stream twice", dict(streams=[1, 1])),
        ("thres NaN", dict(rule_kw={"match_thres": NAN})), ("thres inf", dict(rule_kw={"match_thres": INF})), ("thres < 0", dict(rule_kw={"match_thres": -0.1})),
        ("init_conf NaN", dict(rule_kw={"init_conf": NAN})), ("max_misses < 0", dict(rule_kw={"max_misses": -1})),
        ("confirm_hits < 1", dict(rule_kw={"confirm_hits": 0})),
        ("fresh: dets alone", dict(fs=None, fc=None)), ("fresh: no count", dict(fc=None)), ("fresh: no dets", dict(fd=None)), ("fresh: no src", dict(fs=None)),
        ("std_pos 0", dict(motion=(0.0, 0.1, 0.1))), ("std_vel < 0", dict(motion=(0.1, -0.1, 0.1))), ("std_meas NaN", dict(motion=(0.1, 0.1, NAN))),
        ("std_pos inf", dict(motion=(INF, 0.1, 0.1))), ("std_vel NaN", dict(motion=(0.1, NAN, 0.1))), ("std_meas 0", dict(motion=(0.1, 0.1, 0.0))),
    ]
    for what, kw in cases:
        rule_kw = kw.pop("rule_kw", None)
        assert call(rule_kw, **kw) == _lib.ERR_ARG, what
        assert "yfv2_track_update_motion" in _lib.last_error(eng._h), what
    assert call(h=None) == _lib.ERR_ARG
    torch.cuda.synchronize(dev)
    assert (state == 0x5A5A5A5).all()
    for t, v in zip(outs, (S_ID, S_HITS, S_DETS, S_SRC, S_CNT, S_BOX)):
        assert (t == v).all()
    # what is allowed: track_hits, track_box and the fresh outputs left out, infinite init_conf, the bounds themselves
    state.zero_()
    assert call(hits=None, box=None, fd=None, fs=None, fc=None, rule_kw={"init_conf": INF, "max_misses": 0, "confirm_hits": 1, "match_thres": 0.0}) == 0
    torch.cuda.synchronize(dev)
    assert (outs[0] == 0).all() and (outs[1] == S_HITS).all() and (outs[5] == S_BOX).all() and state[[0, 2], 2].tolist() == [1, 1] and state[1].eq(0).all()
    # Engine- and Tracker-level validation
    tr = yfv2.Tracker(eng, S, max_tracks=M, motion=dict(std_vel=0.01))
    assert tr.motion == dict(std_pos=0.05, std_vel=0.01, std_meas=0.05) and tuple(tr.state.shape) == (S, words)
    with pytest.raises(ValueError):
        tr.update(d, c.to(torch.int64))
    with pytest.raises(ValueError):
        eng.track_update_motion(d, c, [0, 1], tr.state[:, :-1].contiguous(), M)
    with pytest.raises(ValueError):
        eng.track_update_motion(d, c, [0, 1], torch.zeros((S, 8 + 10 * M), device=dev, dtype=torch.int32), M)     # the plain form's state
    with pytest.raises(ValueError):
        tr.update(d, c, box=True, out=outs[:2])
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, S, motion=dict(std=1.0))
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, S).update(d, c, box=True)
    with pytest.raises(yfv2.Yfv2Error):
        yfv2.Tracker(eng, S, max_tracks=M, motion=dict(std_pos=-1.0)).update(d, c)
    with pytest.raises(yfv2.Yfv2Error):
        tr.update(d, c, streams=[1, 1])
    assert not tr.state.any()


def test_plain_form_through_the_template(yfv2, eng):
    """motion=None is the plain tracker, now track_kernel<false>: a short sequence with matches, a miss, a death and a reused slot
    still equals tests/track_model.py bit for bit"""
    tr, model = yfv2.Tracker(eng, 1, max_tracks=2, max_misses=1, confirm_hits=2), tm.Model(1, max_tracks=2, max_misses=1, confirm_hits=2)
    assert tr.motion is None and tuple(tr.state.shape) == (1, 8 + 10 * 2)
    for rows in ([_box(0), _box(100)], [_box(103), _box(2), _box(200)], [_box(4)], [_box(6), _box(300)], []):
        d, c = _frame(rows, 4)
        got = tr.update(torch.from_numpy(d).to(eng.device), torch.tensor(c, dtype=torch.int32, device=eng.device), fresh=True)
        want = model.update(d, c)
        assert torch.equal(tr.state.cpu(), torch.from_numpy(model.state))
        assert torch.equal(got[0].cpu(), torch.from_numpy(want["track_id"])) and torch.equal(got[1].cpu(), torch.from_numpy(want["track_hits"]))
        assert torch.equal(got[4].cpu(), torch.from_numpy(want["fresh_count"]))
        k = int(want["fresh_count"][0])
        assert torch.equal(got[3][0, :k].cpu(), torch.from_numpy(want["fresh_src"][0, :k]))
    assert model.state[0, :6].tolist() == [3, 2, 5, 3, 1, 1]      # track 2 died in the fourth frame; the empty frame is a first miss for 1 and 3
