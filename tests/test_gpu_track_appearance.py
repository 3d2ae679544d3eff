"""GPU tests of the tracker's appearance form: Engine.track_update_appearance / tracking.Tracker(appearance=...) (include/yfv2.h
yfv2_track_update_appearance).  Run with ``-m gpu`` on an MI355X.

The claim: after every call the int32 state - header word 7 included - the int32 features and every output (track_id, track_hits,
track_cos, track_pass with two passes, track_box with motion, the fresh outputs) equal the rule's numpy statement
(tests/track_appearance_model.py) bit for bit - torch.equal on int32 views, no tolerance anywhere; with app_thres = +inf the form is
the shipped form of its layout and pass count on the device, bit for bit, while the features are still the model's; rows of the
fresh outputs beyond fresh_count are not written; bad arguments fail before anything is launched.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import track_appearance_model as ta
import track_model as tm
from track_pair import (F32, LAYOUTS, PASSES, S_BOX, S_CNT, S_COS, S_DETS, S_HITS, S_ID, S_PASS, S_SRC, Pair, _bits, _diff, dev, eng,  # noqa: F401
                        yfv2)                                                                                                       # (dev, eng, yfv2: the fixtures)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")

# ---- 1 the scenarios
@pytest.mark.parametrize("second", PASSES)
@pytest.mark.parametrize("motion", LAYOUTS)
def test_the_jump(yfv2, eng, motion, second):
    """IoU 0.143 frame to frame, match_thres 0.3, prox_thres 0.1: the shipped form issues a new id per frame, the constant embedding
    keeps one (the plain layout: 7 matches by the cosine; the motion layout predicts a nearer box after the first leap)"""
    rule = dict(max_tracks=4, match_thres=0.3, max_misses=0, confirm_hits=3)
    p = Pair(yfv2, eng, 1, appearance=dict(dim=16, prox_thres=0.1, app_thres=0.75), second=second, motion=motion, **rule)
    shipped = yfv2.Tracker(eng, 1, **rule)
    ids, ids_shipped = [], []
    for d, c, e in ta.jump_case():
        ids.append(int(p.step(d, c, emb=e)["track_id"][0, 0]))
        ids_shipped.append(int(shipped.update(torch.from_numpy(d).to(p.dev), torch.from_numpy(c).to(p.dev))[0][0, 0]))
    assert ids_shipped == list(range(1, 9)) and ids[:2] == [1, 1]
    if motion is None:
        assert ids == [1] * 8 and p.header() == [1, 1, 8, 1, 0, 0, 0, 7] and p.tracker.header(0)["by_appearance"] == 7
        got = p.tracker.features(0)
        assert got["n_feat"].tolist() == [8] and torch.equal(got["f"].cpu(), torch.from_numpy(ta.unit(16, 3))[None])


@pytest.mark.parametrize("second", PASSES)
@pytest.mark.parametrize("motion", LAYOUTS)
def test_the_neighbour_the_tie_and_the_skipped_update(yfv2, eng, motion, second):
    rule = dict(max_tracks=4, match_thres=0.3, max_misses=5, confirm_hits=3)
    p = Pair(yfv2, eng, 1, appearance=dict(dim=16), second=second, motion=motion, **rule)
    for d, c, e in ta.neighbour_case():
        o = p.step(d, c, emb=e)
    assert o["track_id"][0, 0] == 2 and o["track_cos"][0, 0] == 1.0 and p.header()[7] == 1
    p = Pair(yfv2, eng, 1, appearance=dict(dim=16), second=second, motion=motion, **rule)
    for d, c, e in ta.neighbour_case(tie=True):
        o = p.step(d, c, emb=e)
    assert o["track_id"][0, 0] == 1 and o["track_cos"][0, 0] == 0.0 and p.header()[7] == 0
    p = Pair(yfv2, eng, 1, appearance=dict(dim=16, alpha=0.5), second=second, motion=motion, **rule)
    for d, c, e in ta.flip_case():
        o = p.step(d, c, emb=e)
    assert o["track_cos"][0, 0] == -1.0 and p.model.stats["skipped"] == 1 and p.model.features()[0][0] == 1


# ---- 2 the random walks
@pytest.mark.parametrize("second", PASSES)
@pytest.mark.parametrize("motion", LAYOUTS)
@pytest.mark.parametrize("R,M", sorted(ta.WALKS))
def test_random_walks(yfv2, eng, R, M, motion, second):
    """30 frames, 2 streams permuted per call, counts of 0, negative and beyond R, 5 % of the rows without appearance.  The model
    runs first and its counters are asserted at every shape (tests/test_track_appearance_host.py asserts the same without a
    device), then the device repeats every call against the recorded states, features and outputs"""
    m, calls, shown = ta.walk_calls(R, M, motion, second)
    for k, v in ta.LEAST.items():
        assert shown.get(k, 0) >= v, (k, shown)
    p = Pair(yfv2, eng, 2, appearance=dict(ta.WALK_APP, dim=ta.WALKS[(R, M)][0]), second=second, motion=motion, **m.rule)
    for d, c, e, streams, want, wstate, wfeat in calls:
        p.compare(d, c, streams, want, wstate, wfeat, e)


# ---- 3 equivalence with the shipped forms
@pytest.mark.parametrize("second", PASSES)
@pytest.mark.parametrize("motion", LAYOUTS)
def test_app_thres_inf_is_the_shipped_form_on_the_device(yfv2, eng, motion, second):
    """4 streams, 15 frames, R = 70, M = 33: the shipped entry point of the layout and pass count and the appearance entry point with
    app_thres = +inf on the same rows - state, header (word 7 stays 0) and every shared output identical; feat is the model's"""
    S, T, R, M, D = 4, 15, 70, 33, 32
    rule = dict(max_tracks=M, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=3)
    app = dict(dim=D, prox_thres=0.0, app_thres=INF)
    seq = ta.walk_case(31, S, T, R, M, D)
    old = yfv2.Tracker(eng, S, motion=motion, two_pass=second, **rule)
    new = yfv2.Tracker(eng, S, motion=motion, two_pass=second, appearance=app, **rule)
    model = ta.Model(S, appearance=app, second=second, motion=motion, **rule)
    kw = dict(fresh=True, box=motion is not None, passes=second is not None)
    assigned = 0
    for d, c, e in seq:
        model.update(d, c, e)
        d, c, e = torch.from_numpy(d).to(eng.device), torch.from_numpy(c).to(eng.device), torch.from_numpy(e).to(eng.device)
        a = old.update(d, c, **kw)
        b = new.update(d, c, emb=e, cos=True, **kw)
        assert torch.equal(old.state, new.state)
        written = torch.arange(R, device=eng.device)[None, :] < a[4][:, None]      # fresh rows beyond the counts are not written
        for i, (x, y) in enumerate(zip(a, b)):
            x, y = (x[written], y[written]) if i in (2, 3) else (x, y)
            assert torch.equal(_bits(x), _bits(y)), i
        _diff("feat", new.feat.cpu(), torch.from_numpy(model.feat))
        assigned += int((b[0] != 0).sum())
    head = new.state[:, :8].sum(0).tolist()
    assert assigned > 500 and head[4] > 0 and head[7] == 0 and model.stats["gated"] > 100 and (b[-1] != 0).any(), (assigned, head)


def test_a_state_moves_between_the_entry_points(yfv2, eng):
    """one state tensor, updated by yfv2_track_update and by the appearance entry point in turn: the two models, sharing one state
    array, say the same; the features only move in the appearance calls"""
    rule = dict(max_tracks=8, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=3)
    app = dict(dim=16, prox_thres=0.1)
    seq = ta.walk_case(77, 1, 12, 12, 8, 16, jump=0.4)
    one, two = yfv2.Tracker(eng, 1, **rule), yfv2.Tracker(eng, 1, appearance=app, **rule)
    two.state = one.state
    m1, m2 = tm.Model(1, **rule), ta.Model(1, appearance=app, **rule)
    m2.state = m1.state
    for t, (d, c, e) in enumerate(seq):
        dd, cc, ee = torch.from_numpy(d).to(eng.device), torch.from_numpy(c).to(eng.device), torch.from_numpy(e).to(eng.device)
        got = two.update(dd, cc, emb=ee) if t % 2 else one.update(dd, cc)
        want = m2.update(d, c, e) if t % 2 else m1.update(d, c)
        assert torch.equal(one.state.cpu(), torch.from_numpy(m1.state)) and torch.equal(got[0].cpu(), torch.from_numpy(want["track_id"]))
        _diff("feat", two.feat.cpu(), torch.from_numpy(m2.feat))
    assert m1.state[0, 7] > 0 and m1.state[0, 2] == 12


# ---- 4 sizes
def test_the_widest_embedding(yfv2, eng):
    """D = 2048 at R = 65, M = 64: 128 steps per partial sum, three calls"""
    R, M, D = 65, 64, 2048
    rule = dict(max_tracks=M, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=2)
    p = Pair(yfv2, eng, 1, appearance=dict(ta.WALK_APP, dim=D), motion=True, second=True, **rule)
    for d, c, e in ta.walk_case(5, 1, 3, R, M, D, objects=80, bad=0.1):
        d[0, 0], c[0] = (10.0, 10.0, 50.0, 60.0, 0.9, 0.0), max(int(c[0]), 1) if c[0] <= R else R
        p.step(d, c, emb=e)
    assert p.header()[7] > 0 and p.model.stats["matched_without"] + p.model.stats.get("born_without", 0) > 0


def test_the_largest_table_the_lds_admits_and_the_first_it_refuses(yfv2, eng, dev):
    """28 R + 52 M <= 163328: R = 4096 admits M = 935.  The table is filled by the model (a state does not depend on R), then one
    frame of 4096 rows, 1100 of them counted, runs on the device against it; M = 936 is an argument error and launches nothing"""
    R, M, D = 4096, 935, 16
    assert 28 * R + 52 * M <= 163328 < 28 * R + 52 * (M + 1)
    rule = dict(max_tracks=M, match_thres=0.3, max_misses=1, confirm_hits=2)
    p = Pair(yfv2, eng, 1, appearance=dict(ta.WALK_APP, dim=D), **rule)
    rng = np.random.default_rng(11)
    n0, n1 = 900, 1100

    def frame(n, shift):
        d = np.tile(np.array([9000.0, 9000.0, 9040.0, 9040.0, 0.97, 1.0], F32), (1, R, 1))
        k = np.arange(n)
        x, y = 70.0 * (k % 40) + shift, 70.0 * (k // 40)
        d[0, :n] = np.stack([x, y, x + 40.0, y + 40.0, np.full(n, 0.9), np.zeros(n)], axis=1)
        e = np.ones((1, R, D), F32)
        proto = np.random.default_rng(3).normal(size=(n1, D))
        e[0, :n] = (proto[:n] + 0.05 * rng.normal(size=(n, D))).astype(F32)
        return d, np.array([n], np.int32), e

    d, c, e = frame(n0, 0.0)
    p.model.update(d[:, :n0], c, e[:, :n0])                                           # the model alone: 900 tracks
    p.tracker.state.copy_(torch.from_numpy(p.model.state))
    p.tracker.feat.copy_(torch.from_numpy(p.model.feat))
    d, c, e = frame(n1, 28.0)                                                         # IoU 12 / 68 = 0.18: matched by the cosine; 200 more rows, 35 slots
    o = p.step(d, c, emb=e)
    assert p.header()[7] >= 800 and p.header()[1] == M and p.header()[5] == n1 - M and (o["track_id"][0, :n1] != 0).sum() == M
    big = torch.zeros((1, 8 + 10 * (M + 1)), device=dev, dtype=torch.int32)
    feat = torch.zeros((1, (M + 1) * (4 + D)), device=dev, dtype=torch.int32)
    with pytest.raises(yfv2.Yfv2Error, match="28 R"):
        eng.track_update_appearance(torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(e).to(dev), [0], big, feat, M + 1, dim=D)
    torch.cuda.synchronize(dev)
    assert not big.any() and not feat.any()


@pytest.mark.parametrize("second", PASSES)
@pytest.mark.parametrize("motion", LAYOUTS)
def test_launch_split(yfv2, eng, motion, second):
    """B = 769, R = 4, M = 4, D = 16: one frame more than a launch carries; the second launch's frame, stream, embeddings, track_cos
    and the other outputs are addressed like the first's"""
    B, R, D = 769, 4, 16
    rng = np.random.default_rng(2)
    streams = rng.permutation(B).tolist()
    d = np.zeros((B, R, 6), F32)
    d[:, 0] = np.concatenate([rng.uniform(0, 20, (B, 2)), rng.uniform(60, 90, (B, 2)), np.full((B, 1), 0.9), np.zeros((B, 1))], axis=1)
    d[:, 1] = d[:, 0] + F32(200.0)
    d[:, 1, 4:] = (0.8, 0.0)
    e = rng.normal(size=(B, R, D)).astype(F32)
    p = Pair(yfv2, eng, B, appearance=dict(dim=D, prox_thres=0.1), second=second, motion=motion, max_tracks=4, confirm_hits=2)
    p.step(d, np.full(B, 2, np.int32), streams, emb=e)
    d[:, :2, :4] += F32(3.0)
    o = p.step(d, np.full(B, 2, np.int32), streams, emb=e)
    assert (o["fresh_count"] == 2).all() and (p.model.state[:, 0] == 2).all() and (p.model.state[:, 7] == 2).all()
    assert (np.abs(o["track_cos"][768, :2] - 1.0) < 1e-5).all() and not o["track_cos"][768, 2:].any()


# ---- 5 optional outputs
@pytest.mark.parametrize("second", PASSES)
@pytest.mark.parametrize("motion", LAYOUTS)
def test_optional_outputs(yfv2, eng, motion, second):
    """every combination of the optional outputs the form admits: the state, the features and the other outputs are the same bits
    (track_hits, which the Python layer always passes, is left out through the C ABI in the argument test)"""
    seq = ta.jump_case(frames=4)
    combos = [c for c in itertools.product([False, True], repeat=4) if (motion or not c[1]) and (second or not c[2])]      # fresh, box, passes, cos
    ps = [Pair(yfv2, eng, 1, appearance=dict(dim=16, prox_thres=0.1), second=second, motion=motion, max_tracks=4, confirm_hits=2) for _ in combos]
    for d, c, e in seq:
        for p, (fresh, box, passes, cos) in zip(ps, combos):
            p.step(d, c, emb=e, fresh=fresh, box=box, passes=passes, cos=cos)
    for p in ps[1:]:
        assert torch.equal(p.tracker.state, ps[0].tracker.state) and torch.equal(p.tracker.feat, ps[0].tracker.feat)
    assert ps[0].header()[:6] == [1, 1, 4, 1, 0, 0] and ps[0].header()[7] >= 1


# ---- 6 argument errors
def test_argument_errors_launch_nothing(yfv2, eng, dev):
    from yolo_fastestv2_amd import _lib
    L = _lib.lib()
    B, R, S, M, D = 2, 8, 3, 4, 16
    states = {False: torch.full((S, 8 + 10 * M), 0x5A5A5A5, device=dev, dtype=torch.int32), True: torch.full((S, 8 + 32 * M), 0x5A5A5A5, device=dev, dtype=torch.int32)}
    feat = torch.full((S, M * (4 + D)), 0x3C3C3C3, device=dev, dtype=torch.int32)
    clones = {k: v.clone() for k, v in states.items()}
    feat0 = feat.clone()
    d = torch.zeros((B, R, 6), device=dev)
    c = torch.full((B,), 3, device=dev, dtype=torch.int32)
    e = torch.ones((B, R, D), device=dev)
    outs = (torch.full((B, R), S_ID, device=dev, dtype=torch.int32), torch.full((B, R), S_HITS, device=dev, dtype=torch.int32),
            torch.full((B, R, 6), S_DETS, device=dev), torch.full((B, R), S_SRC, device=dev, dtype=torch.int32), torch.full((B,), S_CNT, device=dev, dtype=torch.int32),
            torch.full((B, R, 4), S_BOX, device=dev), torch.full((B, R), S_PASS, device=dev, dtype=torch.int32), torch.full((B, R), S_COS, device=dev))
    good = dict(h=eng._h, dets=d.data_ptr(), count=c.data_ptr(), R=R, B=B, streams=[0, 2], S=S, rule=True, motion=(0.05, 0.00625, 0.05),
                second=(0.5, 0.1, 0.5, 1), app=(D, 0.5, 0.75, 0.9), emb=e.data_ptr(), feat=feat.data_ptr(), tid=outs[0].data_ptr(), hits=outs[1].data_ptr(),
                fd=outs[2].data_ptr(), fs=outs[3].data_ptr(), fc=outs[4].data_ptr(), box=outs[5].data_ptr(), tpass=outs[6].data_ptr(), cos=outs[7].data_ptr())

    def call(rule_kw=None, **over):
        a = dict(good, **over)
        r = _lib.TrackRule()
        r.max_tracks, r.match_thres, r.class_aware, r.init_conf, r.max_misses, r.confirm_hits = M, 0.3, 1, 0.0, 30, 3
        for k, v in (rule_kw or {}).items():
            setattr(r, k, v)
        arr = (C.c_int32 * max(len(a["streams"]), 1))(*a["streams"]) if a["streams"] is not None else None
        mo = C.byref(_lib.TrackMotion(*a["motion"])) if a["motion"] is not None else None
        se = C.byref(_lib.TrackSecond(*a["second"])) if a["second"] is not None else None
        ap = C.byref(_lib.TrackAppearance(*a["app"])) if a["app"] is not None else None
        state = a["state"] if "state" in a else states[a["motion"] is not None].data_ptr()
        return L.yfv2_track_update_appearance(a["h"], a["dets"], a["count"], a["R"], a["B"], arr, state, a["S"], C.byref(r) if a["rule"] else None, mo, se, ap,
                                              a["emb"], a["feat"], a["tid"], a["hits"], a["tpass"], a["box"], a["cos"], a["fd"], a["fs"], a["fc"], None)

    cases = [
        # the appearance form's own
        ("null appearance", dict(app=None)), ("null emb", dict(emb=None)), ("null feat", dict(feat=None)), ("emb unaligned", dict(emb=e.data_ptr() + 4)),
        ("dim 0", dict(app=(0, 0.5, 0.75, 0.9))), ("dim 8", dict(app=(8, 0.5, 0.75, 0.9))), ("dim 24", dict(app=(24, 0.5, 0.75, 0.9))),
        ("dim 2064", dict(app=(2064, 0.5, 0.75, 0.9))), ("dim < 0", dict(app=(-16, 0.5, 0.75, 0.9))),
        ("prox NaN", dict(app=(D, NAN, 0.75, 0.9))), ("prox inf", dict(app=(D, INF, 0.75, 0.9))), ("prox < 0", dict(app=(D, -0.1, 0.75, 0.9))),
        ("app NaN", dict(app=(D, 0.5, NAN, 0.9))), ("alpha NaN", dict(app=(D, 0.5, 0.75, NAN))), ("alpha inf", dict(app=(D, 0.5, 0.75, INF))),
        ("alpha < 0", dict(app=(D, 0.5, 0.75, -0.01))), ("alpha > 1", dict(app=(D, 0.5, 0.75, 1.01))),
        ("LDS", dict(R=4096, rule_kw={"max_tracks": 936})), ("LDS, M = 1024", dict(R=3932, rule_kw={"max_tracks": 1024})),
        ("track_box without motion", dict(motion=None)), ("track_pass without second", dict(second=None)),
        # every check of the forms it extends
        ("high_conf NaN", dict(second=(NAN, 0.1, 0.5, 1))), ("low_conf NaN", dict(second=(0.5, NAN, 0.5, 1))),
        ("low > high", dict(second=(0.3, 0.4, 0.5, 1))), ("thres_low NaN", dict(second=(0.5, 0.1, NAN, 1))), ("thres_low inf", dict(second=(0.5, 0.1, INF, 1))),
        ("thres_low < 0", dict(second=(0.5, 0.1, -0.1, 1))),
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
        assert "yfv2_track_update_appearance" in _lib.last_error(eng._h), what
        torch.cuda.synchronize(dev)
        for k in states:
            assert torch.equal(states[k], clones[k]), what
        assert torch.equal(feat, feat0), what
    assert call(h=None) == _lib.ERR_ARG
    torch.cuda.synchronize(dev)
    for t, v in zip(outs, (S_ID, S_HITS, S_DETS, S_SRC, S_CNT, S_BOX, S_PASS, S_COS)):
        assert (t == v).all()
    # what is allowed: every optional output left out, in both layouts and pass counts; an infinite app_thres of either sign; alpha 0 and 1
    for motion, second in itertools.product((None, (0.05, 0.00625, 0.05)), (None, (0.5, 0.1, 0.5, 1))):
        st = states[motion is not None]
        st.zero_()
        feat.zero_()
        none = dict(motion=motion, second=second, hits=None, tpass=None, box=None, cos=None, fd=None, fs=None, fc=None)
        assert call(app=(D, 0.0, INF, 0.0), **none) == 0
        assert call(app=(D, 0.5, -INF, 1.0), **none) == 0
        torch.cuda.synchronize(dev)
        assert (outs[0] == 0).all() and (outs[1] == S_HITS).all() and (outs[5] == S_BOX).all() and (outs[6] == S_PASS).all() and (outs[7] == S_COS).all()
        assert st[[0, 2], 2].tolist() == [2, 2] and st[1].eq(0).all() and not feat.any()
    # track_hits left out, track_cos given: the plain layout, one pass, through the C ABI
    states[False].zero_()
    d[:, 0] = torch.tensor([0.0, 0.0, 10.0, 10.0, 0.9, 0.0], device=dev)
    for _ in range(2):
        assert call(motion=None, second=None, box=None, tpass=None, hits=None) == 0
    torch.cuda.synchronize(dev)
    assert outs[0][:, 0].tolist() == [1, 1] and (outs[7][:, 0] - 1.0).abs().max() < 1e-6 and not outs[7][:, 1:].any() and (outs[1] == S_HITS).all()
    assert feat.view(S, M, 4 + D)[[0, 2], 0, 0].tolist() == [2, 2] and not feat[1].any()
    # Engine- and Tracker-level validation
    tr = yfv2.Tracker(eng, S, max_tracks=M, appearance=dict(dim=D, alpha=0.8))
    assert tr.appearance == dict(dim=D, prox_thres=0.5, app_thres=0.75, alpha=0.8) and tuple(tr.feat.shape) == (S, M * (4 + D))
    with pytest.raises(ValueError):
        tr.update(d, c)                                                             # no emb
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, S, max_tracks=M).update(d, c, emb=e)                      # emb without appearance
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, S, max_tracks=M).update(d, c, cos=True)
    with pytest.raises(ValueError):
        tr.update(d, c, emb=e[:, :, :8])
    with pytest.raises(ValueError):
        tr.update(d, c, emb=e.double())
    with pytest.raises(ValueError):
        tr.update(d, c, emb=e, passes=True)
    with pytest.raises(ValueError):
        tr.update(d, c, emb=e, box=True)
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, S, max_tracks=M, appearance=dict(dim=20))
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, S, max_tracks=M, appearance=dict(momentum=0.5))
    with pytest.raises(ValueError):
        yfv2.Tracker(eng, S, max_tracks=M).features(0)
    with pytest.raises(ValueError):
        eng.track_update_appearance(d, c, e, [0, 1], states[False], feat[:, :-1].contiguous(), M, dim=D)
    with pytest.raises(yfv2.Yfv2Error):
        yfv2.Tracker(eng, S, max_tracks=M, appearance=dict(dim=D, alpha=1.5)).update(d, c, emb=e)
    with pytest.raises(yfv2.Yfv2Error):
        tr.update(d, c, emb=e, streams=[1, 1])
    assert not tr.state.any() and not tr.feat.any()
    tr.update(d, c, emb=e)
    assert tr.feat[:2].any() and tr.features(0)["n_feat"].tolist() == [1]
    tr.reset(0)
    assert not tr.feat[0].any() and not tr.state[0].any() and tr.feat[1].any()
    tr.reset()
    assert not tr.feat.any() and not tr.state.any()
