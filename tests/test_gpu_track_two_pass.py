"""GPU tests of the tracker's two-pass form: Engine.track_update_two_pass / tracking.Tracker(two_pass=...) (include/yfv2.h
yfv2_track_update_two_pass).  Run with ``-m gpu`` on an MI355X.

The claim: after every call the int32 state - header word 6 and, in the motion layout, the filter words included - and every output
(track_id, track_hits, track_pass, the fresh outputs, with motion track_box) equal the rule's numpy statement
(tests/track_two_pass_model.py) bit for bit - torch.equal on int32 views, no tolerance anywhere; with high_conf = -inf the form is
the shipped one-pass form of its layout on the device, bit for bit; rows of the fresh outputs beyond fresh_count are not written;
bad arguments fail before anything is launched.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import track_model as tm
import track_pair
import track_two_pass_model as tp
from track_pair import (F32, LAYOUTS, S_BOX, S_CNT, S_DETS, S_HITS, S_ID, S_PASS, S_SRC, _bits, _box, _frame, dev, eng,  # noqa: F401
                        yfv2)                                                                                           # (dev, eng, yfv2: the fixtures)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")

Pair = functools.partial(track_pair.Pair, second=True)          # every tracker of this file has two passes; second=dict(...) sets their rule


# ---- 1 equivalence with the shipped form
@pytest.mark.parametrize("motion", LAYOUTS)
def test_high_conf_minus_inf_is_the_shipped_form_on_the_device(yfv2, eng, motion):
    """8 streams, 20 frames, R = 70, M = 33: yfv2_track_update / yfv2_track_update_motion and the two-pass entry point with
    high_conf = -inf on the same rows - state, header and every output identical, track_pass == (track_id != 0)"""
    S, T, R, M = 8, 20, 70, 33
    rule = dict(max_tracks=M, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=3)
    seq = tp.walk_case(31, S, T, R, M)
    one = yfv2.Tracker(eng, S, motion=motion, **rule)
    two = yfv2.Tracker(eng, S, motion=motion, two_pass=dict(high_conf=-INF, low_conf=-INF), **rule)
    box = motion is not None
    assigned = 0
    for d, c in seq:
        d, c = torch.from_numpy(d).to(eng.device), torch.from_numpy(c).to(eng.device)
        a = one.update(d, c, fresh=True, box=box)
        b = two.update(d, c, fresh=True, box=box, passes=True)
        assert torch.equal(one.state, two.state)
        written = torch.arange(R, device=eng.device)[None, :] < a[4][:, None]      # fresh rows beyond the counts are not written
        for i, (x, y) in enumerate(zip(a, b)):
            x, y = (x[written], y[written]) if i in (2, 3) else (x, y)
            assert torch.equal(_bits(x), _bits(y)), i
        assert torch.equal(b[-1], (b[0] != 0).to(torch.int32))
        assigned += int((b[0] != 0).sum())
    head = one.state[:, :8].sum(0).tolist()
    assert assigned > 1000 and head[4] > 0 and head[5] > 0 and head[6] == 0, (assigned, head)


# ---- 2 the dip
@pytest.mark.parametrize("motion", LAYOUTS)
def test_the_dip(yfv2, eng, motion):
    """conf 0.9 for 5 frames, 0.3 for 4, 0.9 again, IoU 9 / 11 frame to frame, max_misses 2, confirm_hits 3: one id, hits 12, one
    fresh row, track_pass 2 on the dip frames; the one-pass form on the rows >= 0.5: two ids, two fresh rows"""
    rule = dict(max_tracks=4, match_thres=0.3, max_misses=2, confirm_hits=3)
    p = Pair(yfv2, eng, 1, motion=motion, **rule)
    plain = yfv2.Tracker(eng, 1, motion=motion, **rule)
    ids, passes, hits, fresh, ids_one, fresh_one = [], [], [], 0, [], 0
    for d, c in tp.dip_case():
        o = p.step(d, c)
        ids.append(int(o["track_id"][0, 0])); passes.append(int(o["track_pass"][0, 0])); hits.append(int(o["track_hits"][0, 0]))
        fresh += int(o["fresh_count"][0])
        c1 = c if d[0, 0, 4] >= 0.5 else np.zeros(1, np.int32)                   # a caller's single threshold removes the dip's rows
        got = plain.update(torch.from_numpy(d).to(p.dev), torch.from_numpy(c1).to(p.dev), fresh=True)
        ids_one.append(int(got[0][0, 0]) if c1[0] else 0)
        fresh_one += int(got[4][0])
    assert ids == [1] * 12 and hits[-1] == 12 >= 10 and fresh == 1 and passes == [1] * 5 + [2] * 4 + [1] * 3
    assert p.header() == [1, 1, 12, 1, 0, 0, 4] and p.tracker.header(0)["second"] == 4
    assert ids_one == [1] * 5 + [0] * 4 + [2] * 3 and fresh_one == 2 and "second" not in plain.header(0)


# ---- 3 no birth from LOW, 4 pass order
@pytest.mark.parametrize("motion", LAYOUTS)
def test_no_birth_from_low_and_pass_order(yfv2, eng, motion):
    p = Pair(yfv2, eng, 1, motion=motion, max_tracks=4, match_thres=0.3, init_conf=0.7, max_misses=5, confirm_hits=2)
    o = p.step(*_frame([_box(0), _box(100, conf=0.3), _box(200, conf=0.6)]))         # HIGH; LOW far from every track; HIGH below init_conf
    assert o["track_id"][0].tolist() == [1, 0, 0, 0] and o["track_pass"][0].tolist() == [1, 0, 0, 0] and p.header() == [1, 1, 1, 1, 0, 0, 0]
    o = p.step(*_frame([_box(0), _box(100, conf=0.3), _box(200, conf=0.6)]))         # again, with a live track: issued does not move
    assert o["track_id"][0].tolist() == [1, 0, 0, 0] and p.header() == [1, 1, 2, 1, 0, 0, 0]
    # the track at 0..10 (at rest: the motion form predicts the same box): a LOW row at IoU 9 / 11, a HIGH row at IoU 6 / 14 = 0.43
    o = p.step(*_frame([_box(1, conf=0.3), _box(4, conf=0.9)]))
    assert o["track_id"][0].tolist() == [0, 1, 0, 0] and o["track_pass"][0].tolist() == [0, 1, 0, 0] and p.model.stats["lost"] == 1
    assert p.header() == [1, 1, 3, 1, 0, 0, 0] and p.slots()[0, 7] == 3


# ---- 5 tracked_only
@pytest.mark.parametrize("motion", LAYOUTS)
@pytest.mark.parametrize("only", [1, 0])
def test_tracked_only(yfv2, eng, motion, only):
    """a track with misses == 1 and a LOW row on top of it: barred (the slot misses again) or matched; a HIGH row matches either way"""
    for high_row in (False, True):
        p = Pair(yfv2, eng, 1, second=dict(tracked_only=only), motion=motion, max_tracks=4, max_misses=5, confirm_hits=2)
        p.step(*_frame([_box(0)]))
        p.step(*_frame([]))
        assert p.slots()[0, 8] == 1
        o = p.step(*_frame([_box(1, conf=0.9 if high_row else 0.3)]))
        matched = high_row or not only
        assert o["track_id"][0].tolist() == [1 if matched else 0, 0, 0, 0] and o["track_pass"][0, 0] == (0 if not matched else 1 if high_row else 2)
        assert p.slots()[0, 8] == (0 if matched else 2) and p.model.stats["barred"] == (0 if matched else 1)
        assert p.header()[6] == (1 if matched and not high_row else 0)


# ---- 6 boundaries
def test_boundaries(yfv2, eng):
    high, low = F32(0.5), F32(0.25)
    below = np.nextafter(low, F32(0))
    sec = dict(high_conf=float(high), low_conf=float(low), match_thres_low=0.5)
    rule = dict(max_tracks=4, match_thres=0.3, max_misses=9, confirm_hits=2)
    p = Pair(yfv2, eng, 1, second=sec, **rule)
    o = p.step(*_frame([_box(0, conf=high), _box(100, conf=np.nextafter(high, F32(0)))]))      # exactly high_conf: HIGH, born; one ulp less: LOW
    assert o["track_id"][0].tolist() == [1, 0, 0, 0]
    o = p.step(*_frame([_box(0, conf=low)]))                                                  # exactly low_conf: LOW
    assert o["track_pass"][0].tolist() == [2, 0, 0, 0]
    o = p.step(*_frame([_box(0, conf=below)]))                                                # the next float below: OUT
    assert o["track_id"][0].tolist() == [0, 0, 0, 0] and p.slots()[0, 8] == 1
    q = Pair(yfv2, eng, 1, second=dict(high_conf=0.5, low_conf=0.5, tracked_only=0), **rule)  # low_conf == high_conf: no LOW rows
    q.step(*_frame([_box(0, conf=0.5)]))
    o = q.step(*_frame([_box(0, conf=float(np.nextafter(high, F32(0)))), _box(0, conf=0.5)]))
    assert o["track_pass"][0].tolist() == [0, 1, 0, 0] and q.header()[6] == 0
    # an IoU exactly match_thres_low is no edge.  Dyadic boxes: a 16 x 10 row inside a 32 x 10 track, 160 / (320 + 160 - 160) = 0.5
    assert float(tm.iou(np.array([0, 0, 32, 10], F32), np.array([8, 0, 24, 10], F32))) == 0.5
    for thres, want in ((0.5, 0), (float(np.nextafter(0.5, 0.0)), 2)):
        t = Pair(yfv2, eng, 1, second=dict(match_thres_low=thres), max_tracks=4, match_thres=0.1, max_misses=9, confirm_hits=2)
        t.step(*_frame([[0.0, 0.0, 32.0, 10.0, 0.9, 0.0]]))
        o = t.step(*_frame([[8.0, 0.0, 24.0, 10.0, 0.3, 0.0]]))
        assert o["track_pass"][0].tolist() == [want, 0, 0, 0], thres


# ---- 7 seeded random walks with score dips and dropouts
LEAST = dict(second=50, barred=1, lost=1, deaths=1, dropped=1)       # what the model's counters must show at least, at every shape
# R, M: the generator's objects, dip_rate and intruder.  More objects than slots wherever the table is to fill (dropped births); at
# R = 1 there is one object, so half of its frames are dips (440 stream-frames with at most one row each must give 50 second-pass
# matches) and a far HIGH row now and then is what finds the one slot taken
WALKS = {(1, 1): (1, 0.5, 0.05), (65, 64): (80, 0.2, 0.0), (300, 256): (260, 0.2, 0.0), (1030, 40): (1150, 0.2, 0.0)}


@pytest.mark.parametrize("motion", LAYOUTS)
@pytest.mark.parametrize("R,M", sorted(WALKS))
def test_random_walks_with_dips_and_dropouts(yfv2, eng, motion, R, M):
    """S = 12, 40 frames, the streams permuted per call and one skipped per call; counts of 0, negative and beyond R.  The model runs
    first and its counters are asserted at EVERY shape - at least 50 second-pass matches, a slot barred by tracked_only, a death, a
    dropped birth and a LOW row that lost a slot it had the higher IoU for (that one not at R = 1: a frame of one row has no second
    row to lose to) - then the device repeats every call against the recorded states and outputs"""
    S, T = 12, 40
    objects, dip_rate, intruder = WALKS[(R, M)]
    least = {k: v for k, v in LEAST.items() if not (k == "lost" and R == 1)}
    rule = dict(max_tracks=M, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=3)
    seq = tp.walk_case(100 + R, S, T, R, M, objects, dip_rate, intruder)
    rng = np.random.default_rng(5)
    p = Pair(yfv2, eng, S, motion=motion, **rule)
    calls, odd = [], set()
    for d, c in seq:
        perm = rng.permutation(S)[:-1]
        d, c = np.ascontiguousarray(d[perm]), np.ascontiguousarray(c[perm])
        calls.append((d, c, perm.tolist(), p.model.update(d, c, perm.tolist()), p.model.state.copy()))
        odd |= {"zero" if v == 0 else "negative" if v < 0 else "beyond" if v > R else "" for v in c.tolist()}
    shown = dict(p.model.stats, deaths=int(p.model.state[:, 4].sum()), dropped=int(p.model.state[:, 5].sum()))
    for k, v in least.items():
        assert shown[k] >= v, (k, shown[k])
    assert odd >= {"zero", "negative", "beyond"} and p.model.state[:, 6].sum() == shown["second"]
    if R > 1024:
        assert any(((c > 1024) & (c <= R)).any() for _d, c, *_ in calls)             # more rows than threads, every one a row of the walk
    for d, c, streams, want, wstate in calls:
        p.compare(d, c, streams, want, wstate)


# ---- 8 the chain in the second pass
@pytest.mark.parametrize("motion", LAYOUTS)
def test_the_chain_in_the_second_pass(yfv2, eng, motion):
    """chain_case(40), M = 40: the tracks are born HIGH, the rows come LOW: 40 rounds, every one in the second pass"""
    tracks, rows = tm.chain_case(40)
    rows = rows.copy()
    rows[:, 4] = 0.3
    p = Pair(yfv2, eng, 1, second=dict(match_thres_low=0.1), motion=motion, max_tracks=40, match_thres=0.1)
    assert p.step(tracks[None], [40])["track_id"][0].tolist() == list(range(1, 41))
    par = tp.Model(1, second=dict(match_thres_low=0.1), motion=motion, max_tracks=40, match_thres=0.1)
    par.update(tracks[None], [40])
    par.update(rows[None], [40], match=tm.mutual_best)
    o = p.step(rows[None], [40])
    assert o["track_id"][0].tolist() == list(range(1, 41)) and (o["track_pass"][0] == 2).all() and p.header()[6] == 40
    assert par.stats["rounds"][-1] == (0, 40) and np.array_equal(par.state, p.model.state)


# ---- 9 NaN / inf rows and NaN conf in each of the HIGH / LOW positions
@pytest.mark.parametrize("motion", LAYOUTS)
def test_nan_and_inf_rows(yfv2, eng, motion):
    p = Pair(yfv2, eng, 1, second=dict(tracked_only=0), motion=motion, max_tracks=8, confirm_hits=2)
    bad = []
    for conf in (0.9, 0.3):
        bad += [[NAN, 0, 10, 10, conf, 0], [0, 0, INF, 10, conf, 0], [0, -INF, 10, 10, conf, 0], [0, 0, 10, 10, conf, NAN], [0, 0, 10, 10, conf, INF]]
    bad += [[0, 0, 10, 10, NAN, 0], [0, 0, 10, 10, INF, 0], [0, 0, 10, 10, -INF, 0]]
    R = 16
    o = p.step(*_frame([_box(0)] + bad, R))
    assert o["track_id"][0].tolist() == [1] + [0] * (R - 1) and p.header() == [1, 1, 1, 1, 0, 0, 0]
    o = p.step(*_frame(bad + [_box(1, conf=0.3)], R))                                # the broken rows in front of a LOW row that matches
    assert o["track_pass"][0].tolist() == [0] * len(bad) + [2, 0, 0] and p.header() == [1, 1, 2, 1, 0, 0, 1] and o["fresh_count"][0] == 1
    o = p.step(*_frame(bad[::-1] + [_box(2, conf=0.9)], R))                          # ... and of a HIGH row
    assert o["track_pass"][0].tolist() == [0] * len(bad) + [1, 0, 0] and p.header() == [1, 1, 3, 1, 0, 0, 1]


# ---- 10 launch split
@pytest.mark.parametrize("motion", LAYOUTS)
def test_launch_split(yfv2, eng, motion):
    """B = 769, R = 4, M = 4: one frame more than a launch carries; the second launch's frame, stream, track_pass and track_box are
    addressed like the first's"""
    B, R = 769, 4
    rng = np.random.default_rng(2)
    streams = rng.permutation(B).tolist()
    d = np.zeros((B, R, 6), F32)
    d[:, 0] = np.concatenate([rng.uniform(0, 20, (B, 2)), rng.uniform(60, 90, (B, 2)), np.full((B, 1), 0.9), np.zeros((B, 1))], axis=1)
    d[:, 1] = d[:, 0] + F32(200.0)
    d[:, 1, 4:] = (0.8, 0.0)
    p = Pair(yfv2, eng, B, motion=motion, max_tracks=4, confirm_hits=2)
    p.step(d, np.full(B, 2, np.int32), streams)
    d[:, :2, :4] += F32(3.0)
    d[:, 1, 4] = 0.3
    o = p.step(d, np.full(B, 2, np.int32), streams)
    assert (o["fresh_count"] == 2).all() and (p.model.state[:, 0] == 2).all() and (p.model.state[:, 6] == 1).all()
    assert o["track_pass"][768].tolist() == [1, 2, 0, 0]


# ---- 11 optional outputs
@pytest.mark.parametrize("motion", LAYOUTS)
def test_optional_outputs(yfv2, eng, motion):
    """every optional output absent, and each one alone: the state and the other outputs are the same bits (track_hits, which the
    Python layer always passes, is left out through the C ABI below)"""
    seq = tp.dip_case(high=3, dip=2, after=1)
    combos = [(False, False, False), (True, False, False), (False, False, True)] + ([(False, True, False), (True, True, True)] if motion else [(True, False, True)])
    ps = [Pair(yfv2, eng, 1, motion=motion, max_tracks=4, confirm_hits=2) for _ in combos]
    for d, c in seq:
        for p, (fresh, box, passes) in zip(ps, combos):
            p.step(d, c, fresh=fresh, box=box, passes=passes)
    for p in ps[1:]:
        assert torch.equal(p.tracker.state, ps[0].tracker.state)
    assert ps[0].header() == [1, 1, 6, 1, 0, 0, 2]


# ---- 12 argument errors
def test_argument_errors_launch_nothing(yfv2, eng, dev):
    from yolo_fastestv2_amd import _lib
    L = _lib.lib()
    B, R, S, M = 2, 8, 3, 4
    states = {False: torch.full((S, 8 + 10 * M), 0x5A5A5A5, device=dev, dtype=torch.int32), True: torch.full((S, 8 + 32 * M), 0x5A5A5A5, device=dev, dtype=torch.int32)}
    clones = {k: v.clone() for k, v in states.items()}
    d = torch.zeros((B, R, 6), device=dev)
    c = torch.full((B,), 3, device=dev, dtype=torch.int32)
    outs = (torch.full((B, R), S_ID, device=dev, dtype=torch.int32), torch.full((B, R), S_HITS, device=dev, dtype=torch.int32),
            torch.full((B, R, 6), S_DETS, device=dev), torch.full((B, R), S_SRC, device=dev, dtype=torch.int32), torch.full((B,), S_CNT, device=dev, dtype=torch.int32),
            torch.full((B, R, 4), S_BOX, device=dev), torch.full((B, R), S_PASS, device=dev, dtype=torch.int32))
    good = dict(h=eng._h, dets=d.data_ptr(), count=c.data_ptr(), R=R, B=B, streams=[0, 2], S=S, rule=True, motion=(0.05, 0.00625, 0.05),
                second=(0.5, 0.1, 0.5, 1), tid=outs[0].data_ptr(), hits=outs[1].data_ptr(), fd=outs[2].data_ptr(), fs=outs[3].data_ptr(),
                fc=outs[4].data_ptr(), box=outs[5].data_ptr(), tpass=outs[6].data_ptr())

    def call(rule_kw=None, **over):
        a = dict(good, **over)
        r = _lib.TrackRule()
        r.max_tracks, r.match_thres, r.class_aware, r.init_conf, r.max_misses, r.confirm_hits = M, 0.3, 1, 0.0, 30, 3
        for k, v in (rule_kw or {}).items():
            setattr(r, k, v)
        arr = (C.c_int32 * max(len(a["streams"]), 1))(*a["streams"]) if a["streams"] is not None else None
        mo = C.byref(_lib.TrackMotion(*a["motion"])) if a["motion"] is not None else None
        se = C.byref(_lib.TrackSecond(*a["second"])) if a["second"] is not None else None
        state = a["state"] if "state" in a else states[a["motion"] is not None].data_ptr()
        return L.yfv2_track_update_two_pass(a["h"], a["dets"], a["count"], a["R"], a["B"], arr, state, a["S"], C.byref(r) if a["rule"] else None, mo, se,
                                            a["tid"], a["hits"], a["tpass"], a["box"], a["fd"], a["fs"], a["fc"], None)

    cases = [
        # the two-pass form's own
        ("null second", dict(second=None)), ("high_conf NaN", dict(second=(NAN, 0.1, 0.5, 1))), ("low_conf NaN", dict(second=(0.5, NAN, 0.5, 1))),
        ("low > high", dict(second=(0.3, 0.4, 0.5, 1))), ("thres_low NaN", dict(second=(0.5, 0.1, NAN, 1))), ("thres_low inf", dict(second=(0.5, 0.1, INF, 1))),
        ("thres_low < 0", dict(second=(0.5, 0.1, -0.1, 1))), ("track_box without motion", dict(motion=None)),
        # every check of the existing entry points
        ("null dets", dict(dets=None)), ("null count", dict(count=None)), ("null streams", dict(streams=None)), ("null state", dict(state=None)),
        ("null rule", dict(rule=False)), ("null track_id", dict(tid=None)),
        ("B < 1", dict(B=0)), ("S < 1", dict(S=0)), ("R < 1", dict(R=0)), ("R > 4096", dict(R=4097)),
        ("M < 1", dict(rule_kw={"max_tracks": 0})), ("M > 1024", dict(rule_kw={"max_tracks": 1025})),
        ("stream >= S", dict(streams=[0, 3])), ("stream < 0", dict(streams=[-1, 1])), ("stream twice", dict(streams=[1, 1])),
        ("thres NaN", dict(rule_kw={"match_thres": NAN})), ("thres inf", dict(rule_kw={"match_thres": INF})), ("thres < 0", dict(rule_kw={"match_thres": -0.1})),
        ("init_conf NaN", dict(rule_kw={"init_conf": NAN})), ("max_misses < 0", dict(rule_kw={"max_misses": -1})),
        ("confirm_hits < 1", dict(rule_kw={"confirm_hits": 0})),
        ("fresh: dets alone", dict(fs=None, fc=None)), ("fresh: no count", dict(fc=None)), ("fresh: no dets", dict(fd=None)), ("fresh: no src", dict(fs=None)),
        ("std_pos 0", dict(motion=(0.0, 0.1, 0.1))), ("std_vel < 0", dict(motion=(0.1, -0.1, 0.1))), ("std_meas NaN", dict(motion=(0.1, 0.1, NAN))),
        ("std_pos inf", dict(motion=(INF, 0.1, 0.1))),
    ]
    for what, kw in cases:
        rule_kw = kw.pop("rule_kw", None)
        assert call(rule_kw, **kw) == _lib.ERR_ARG, what
        assert "yfv2_track_update_two_pass" in _lib.last_error(eng._h), what
        torch.cuda.synchronize(dev)
        for k in states:
            assert torch.equal(states[k], clones[k]), what
    assert call(h=None) == _lib.ERR_ARG
    torch.cuda.synchronize(dev)
    for t, v in zip(outs, (S_ID, S_HITS, S_DETS, S_SRC, S_CNT, S_BOX, S_PASS)):
        assert (t == v).all()
    # what is allowed: every optional output left out, in both layouts; infinite thresholds of the classes; low_conf == high_conf
    for motion in (None, (0.05, 0.00625, 0.05)):
        st = states[motion is not None]
        st.zero_()
        assert call(motion=motion, hits=None, tpass=None, box=None, fd=None, fs=None, fc=None, second=(INF, -INF, 0.0, 0)) == 0
        assert call(motion=motion, hits=None, tpass=None, box=None, fd=None, fs=None, fc=None, second=(0.5, 0.5, 0.5, 7)) == 0
        torch.cuda.synchronize(dev)
        assert (outs[0] == 0).all() and (outs[1] == S_HITS).all() and (outs[5] == S_BOX).all() and (outs[6] == S_PASS).all()
        assert st[[0, 2], 2].tolist() == [2, 2] and st[1].eq(0).all()
    # track_hits left out, track_pass given: the plain layout through the C ABI
    states[False].zero_()
    d[:, 0] = torch.tensor([0.0, 0.0, 10.0, 10.0, 0.9, 0.0], device=dev)
    assert call(motion=None, box=None, hits=None) == 0
    torch.cuda.synchronize(dev)
    assert outs[0][:, 0].tolist() == [1, 1] and outs[6][:, 0].tolist() == [1, 1] and not outs[6][:, 1:].any() and (outs[1] == S_HITS).all()
    # Engine- and Tracker-level validation
    tr = yfv2.Tracker(eng, S, max_tracks=M, two_pass=dict(low_conf=0.2))
    assert tr.two_pass == dict(high_conf=0.5, low_conf=0.2, match_thres_low=0.5, tracked_only=True)
    with pytest.raises(ValueError):
        tr.update(d, c.to(torch.int64))
    with pytest.raises(ValueError):
        eng.track_update_two_pass(d, c, [0, 1], states[True], M)                    # the motion form's state without motion
    with pytest.raises(ValueError):
        eng.track_update_two_pass(d, c, [0, 1], states[False], M, motion=True)
    with pytest.raises(ValueError):
        eng.track_update_two_pass(d, c, [0, 1], states[False], M, box=True)
    with pytest.raises(ValueError):
        eng.track_update_two_pass(d, c, [0, 1], states[True], M, motion=dict(std=1.0))
    with pytest.raises(ValueError):
        tr.update(d, c, passes=True, out=outs[:2])
    with pytest.raises(yfv2.Yfv2Error):
        yfv2.Tracker(eng, S, max_tracks=M, two_pass=dict(low_conf=0.6)).update(d, c)
    with pytest.raises(yfv2.Yfv2Error):
        yfv2.Tracker(eng, S, max_tracks=M, two_pass=dict(match_thres_low=-1.0)).update(d, c)
    with pytest.raises(yfv2.Yfv2Error):
        tr.update(d, c, streams=[1, 1])
    assert not tr.state.any()


def test_a_state_moves_between_the_one_pass_and_the_two_pass_entry_point(yfv2, eng):
    """one state tensor, updated by yfv2_track_update and by the two-pass entry point in turn: the two models, sharing one state
    array, say the same"""
    rule = dict(max_tracks=8, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=3)
    seq = tp.walk_case(77, 1, 12, 12, 8)
    one, two = yfv2.Tracker(eng, 1, **rule), yfv2.Tracker(eng, 1, two_pass=True, **rule)
    two.state = one.state
    m1, m2 = tm.Model(1, **rule), tp.Model(1, **rule)
    m2.state = m1.state
    for t, (d, c) in enumerate(seq):
        dd, cc = torch.from_numpy(d).to(eng.device), torch.from_numpy(c).to(eng.device)
        got = (two if t % 2 else one).update(dd, cc)
        want = (m2 if t % 2 else m1).update(d, c)
        assert torch.equal(one.state.cpu(), torch.from_numpy(m1.state)) and torch.equal(got[0].cpu(), torch.from_numpy(want["track_id"]))
    assert m1.state[0, 6] > 0 and m1.state[0, 2] == 12
