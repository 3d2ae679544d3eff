"""CPU-only checks of the tracker's appearance form (include/yfv2.h yfv2_track_update_appearance):
  * the new symbols are declared, exported and bound, the ABI number is still 7
  * the model's arithmetic (tests/track_appearance_model.py: dot16, the norm, the cosine, the feature update) IS the C arithmetic
    behind yfv2_track_cosine / yfv2_track_feature_step, bit for bit, on random and on degenerate vectors
  * with app_thres = +inf the model is the model of the same layout and pass form, while the features are still kept
  * the scenarios the device tests repeat do what they claim on the model alone: the jump, the neighbour, the tie of the limits, the
    skipped feature update
  * the random walks the device tests repeat show every counter the device must be asked about
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import track_appearance_model as ta
import track_model as tm
import track_motion_model as mm
import track_two_pass_model as tp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF, NAN = float("inf"), float("nan")
PF = C.POINTER(C.c_float)


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _p(a):
    return a.ctypes.data_as(PF)


def c_cosine(e, f):
    L = _lib().lib()
    e, f = np.ascontiguousarray(e, F32), np.ascontiguousarray(f, F32)
    n, c = C.c_float(), C.c_float()
    assert L.yfv2_track_cosine(_p(e), _p(f), len(e), C.byref(n), C.byref(c)) == 0
    return np.array([n.value, c.value], F32)


def c_feature_step(f, n_feat, e, alpha):
    L = _lib().lib()
    f, e = np.ascontiguousarray(f, F32), np.ascontiguousarray(e, F32)
    out, n_out = np.empty_like(f), C.c_int32()
    assert L.yfv2_track_feature_step(_p(f), n_feat, _p(e), len(e), alpha, _p(out), C.byref(n_out)) == 0
    return out, n_out.value


def test_appearance_symbols_are_declared_exported_and_bound():
    m = _lib()
    hdr = open(os.path.join(REPO, "include", "yfv2.h")).read()
    declared = set(re.findall(r"YFV2_API\s+[\w\s\*]+?\b(yfv2_\w+)\s*\(", hdr))
    raw = C.CDLL(m.LIB_PATH)
    for name in ("yfv2_track_update_appearance", "yfv2_track_feature_words", "yfv2_track_cosine", "yfv2_track_feature_step"):
        assert name in declared and name in m._PROTOTYPES and hasattr(raw, name), name
    args = m._PROTOTYPES["yfv2_track_update_appearance"][1]
    assert len(args) == 23 and args[11] == C.POINTER(m.TrackAppearance)
    assert m.lib().yfv2_abi_version() == m.ABI_VERSION == 7
    assert [f[0] for f in m.TrackAppearance._fields_] == ["dim", "prox_thres", "app_thres", "alpha"]
    assert C.sizeof(m.TrackAppearance) == 32 and m.TrackAppearance.prox_thres.offset == 8 and m.TrackAppearance.alpha.offset == 24
    assert "typedef struct yfv2_track_appearance" in hdr
    import yolo_fastestv2_amd as yfv2
    assert hasattr(yfv2.Engine, "track_update_appearance") and "appearance" in yfv2.Tracker.__init__.__code__.co_varnames
    assert yfv2.tracking.APPEARANCE_DEFAULTS == ta.DEFAULT and yfv2.tracking.FEATURE_HEAD_WORDS == ta.HEAD


def test_feature_words_and_the_helpers_argument_errors():
    m = _lib()
    L = m.lib()
    assert L.yfv2_track_feature_words(64, 128) == 64 * 132 == ta.feature_words(64, 128)
    assert L.yfv2_track_feature_words(1024, 2048) == 1024 * 2052 and L.yfv2_track_feature_words(1, 16) == 20
    for M, D in ((0, 16), (1025, 16), (4, 0), (4, 8), (4, 24), (4, 2064), (4, -16)):
        assert L.yfv2_track_feature_words(M, D) == m.ERR_ARG, (M, D)
        assert "yfv2_track_feature_words" in m.last_error()
    e = np.ones(16, F32)
    n, c, k = C.c_float(), C.c_float(), C.c_int32()
    out = np.zeros(16, F32)
    for args in ((None, _p(e), 16, C.byref(n), C.byref(c)), (_p(e), None, 16, C.byref(n), C.byref(c)), (_p(e), _p(e), 16, None, C.byref(c)),
                 (_p(e), _p(e), 16, C.byref(n), None), (_p(e), _p(e), 8, C.byref(n), C.byref(c)), (_p(e), _p(e), 40, C.byref(n), C.byref(c)),
                 (_p(e), _p(e), 2064, C.byref(n), C.byref(c))):
        assert L.yfv2_track_cosine(*args) == m.ERR_ARG
        assert "yfv2_track_cosine" in m.last_error()
    for args in ((None, 0, _p(e), 16, 0.9, _p(out), C.byref(k)), (_p(e), 0, None, 16, 0.9, _p(out), C.byref(k)), (_p(e), 0, _p(e), 16, 0.9, None, C.byref(k)),
                 (_p(e), 0, _p(e), 16, 0.9, _p(out), None), (_p(e), -1, _p(e), 16, 0.9, _p(out), C.byref(k)), (_p(e), 0, _p(e), 17, 0.9, _p(out), C.byref(k)),
                 (_p(e), 0, _p(e), 16, NAN, _p(out), C.byref(k)), (_p(e), 0, _p(e), 16, -0.1, _p(out), C.byref(k)), (_p(e), 0, _p(e), 16, 1.5, _p(out), C.byref(k)),
                 (_p(e), 0, _p(e), 16, INF, _p(out), C.byref(k))):
        assert L.yfv2_track_feature_step(*args) == m.ERR_ARG
        assert "yfv2_track_feature_step" in m.last_error()
    assert not out.any()


def _vectors(D, rng):
    """(name, e) pairs: random vectors and every degenerate one the rule speaks of"""
    one_nan, one_inf = rng.normal(size=D).astype(F32), rng.normal(size=D).astype(F32)
    one_nan[D // 3] = np.nan
    one_inf[D - 1] = np.inf
    return [("random", rng.normal(size=D).astype(F32)), ("scaled", (rng.normal(size=D) * 37.5).astype(F32)), ("tiny", (rng.normal(size=D) * 1e-3).astype(F32)),
            ("zero", np.zeros(D, F32)), ("nan", one_nan), ("inf", one_inf), ("1e30", np.full(D, 1e30, F32)), ("1e-30", np.full(D, 1e-30, F32)),
            ("mixed", (rng.normal(size=D) * 10.0 ** rng.integers(-6, 6, D)).astype(F32))]


@pytest.mark.parametrize("D", [16, 48, 128, 2048])
def test_the_model_is_the_c_arithmetic(D):
    """norm, cosine and the feature update, the model against the library's host entry points: array_equal on bits"""
    rng = np.random.default_rng(D)
    f = rng.normal(size=D).astype(F32)
    f = ta.feature_step(np.zeros(D, F32), 0, f, 0.9)[0]             # a unit feature, by the rule's own first step
    shown = set()
    for name, e in _vectors(D, rng):
        n, has = ta.norm(e)
        got = c_cosine(e, f)
        want = np.array([n, ta.cosine(e, f, n)], F32)
        assert np.array_equal(_bits(got), _bits(want)), (name, got, want)
        if name in ("zero", "nan", "inf", "1e30", "1e-30"):
            assert not has, name                                    # each fails the one test of the norm, no element is looked at
        else:
            assert has and abs(float(c_cosine(e, e / n)[1]) - 1.0) < 1e-5
        for alpha in (0.0, 1.0, 0.9):
            for n_feat in (0, 1, 7):
                wf, wn, skipped = ta.feature_step(f, n_feat, e, alpha)
                gf, gn = c_feature_step(f, n_feat, e, alpha)
                assert gn == wn and np.array_equal(_bits(gf), _bits(wf)), (name, alpha, n_feat)
                assert wn == (n_feat if not has else n_feat + 1) and not skipped
                if not has:
                    assert np.array_equal(_bits(gf), _bits(f))
                shown.add((bool(has), n_feat > 0))
    assert len(shown) == 4
    u = ta.unit(D, D // 2)                                          # a norm of exactly 1: the average of u and -u is exactly zero,
    wf, wn, skipped = ta.feature_step(u, 3, -u * F32(4.0), 0.5)     # has no norm, and the feature stays
    gf, gn = c_feature_step(u, 3, -u * F32(4.0), 0.5)
    assert skipped and wn == gn == 3 and np.array_equal(_bits(gf), _bits(u)) and np.array_equal(_bits(wf), _bits(u))
    assert ta.dot16(f, f).dtype == F32 and abs(float(ta.dot16(f, f)) - 1.0) < 1e-5


def test_dot16_is_the_order_the_header_states():
    """the sixteen partial sums and the tree, written out with scalars"""
    rng = np.random.default_rng(3)
    a, b = (rng.normal(size=48) * 1e3).astype(F32), rng.normal(size=48).astype(F32)
    P = [F32(0)] * 16
    for i in range(3):
        for j in range(16):
            P[j] = F32(P[j] + F32(a[16 * i + j] * b[16 * i + j]))
    for stride in (8, 4, 2, 1):
        for j in range(stride):
            P[j] = F32(P[j] + P[j + stride])
    assert _bits(ta.dot16(a, b)) == _bits(P[0])
    assert np.array_equal(_bits(ta.dot16(np.stack([a, b]), b[None])), _bits([ta.dot16(a, b), ta.dot16(b, b)]))


RULE = dict(max_tracks=24, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=3)


@pytest.mark.parametrize("second", [None, True])
@pytest.mark.parametrize("motion", [None, True])
def test_app_thres_inf_is_the_model_of_the_same_form(motion, second):
    """+inf: no pair passes; state, header (word 7 stays 0) and every shared output are the shipped model's bits, and the features
    are kept all the same"""
    seq = ta.walk_case(21, S=3, T=25, R=40, M=24, D=32)
    if second:
        old = tp.Model(3, second=True, motion=motion, **RULE)
    else:
        old = tm.Model(3, **RULE) if motion is None else mm.Model(3, **RULE)
    new = ta.Model(3, appearance=dict(dim=32, app_thres=INF, prox_thres=0.0), second=second, motion=motion, **RULE)
    for d, c, e in seq:
        a, b = old.update(d, c), new.update(d, c, e)
        assert np.array_equal(old.state, new.state)
        for k in a:
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32)), k
    n_feat, f = new.features(0)
    live = new.state[0, tm.HEADER:].reshape(24, -1)[:, 6] != 0
    assert new.stats["by_appearance"] == 0 and not new.state[:, 7].any() and new.stats["gated"] > 100
    assert live.sum() > 5 and n_feat[live].max() > 3 and not n_feat[~live].any() and not f[~live].any()
    norms = np.linalg.norm(f[live & (n_feat > 0)].astype(np.float64), axis=1)
    assert np.abs(norms - 1.0).max() < 1e-5


def _ids(model, case, **kw):
    return [model.update(d, c, e, **kw) if e is not None else model.update(d, c) for d, c, e in case]


@pytest.mark.parametrize("second", [None, True])
@pytest.mark.parametrize("motion", [None, True])
def test_the_jump(motion, second):
    """IoU 0.143 frame to frame, match_thres 0.3: the IoU alone issues a new id every frame; with prox_thres 0.1 the constant
    embedding keeps the one id, and each of the 7 matches was valued by the cosine.  (The motion form sees a track at rest in frame
    2 and a moving one afterwards: its predicted box overlaps more, never less than prox_thres.)"""
    case = ta.jump_case()
    rule = dict(max_tracks=4, match_thres=0.3, max_misses=0, confirm_hits=3)
    plain = tm.Model(1, **rule)
    assert [int(plain.update(d, c)["track_id"][0, 0]) for d, c, _e in case] == list(range(1, 9))
    assert float(tm.iou(case[0][0][0, 0, :4], case[1][0][0, 0, :4])) == F32(400.0) / F32(2800.0)
    m = ta.Model(1, appearance=dict(dim=16, prox_thres=0.1, app_thres=0.75), second=second, motion=None if motion is None else True, **rule)
    outs = [m.update(d, c, e) for d, c, e in case]
    if motion is None:
        assert [int(o["track_id"][0, 0]) for o in outs] == [1] * 8 and m.state[0, 7] == 7 and m.state[0, 0] == 1
        assert [float(o["track_cos"][0, 0]) for o in outs] == [0.0] + [1.0] * 7 and m.features()[0][0] == 8
    else:
        assert int(outs[1]["track_id"][0, 0]) == 1 and m.state[0, 7] >= 1


def test_the_neighbour_and_the_tie():
    rule = dict(max_tracks=4, match_thres=0.3, max_misses=5, confirm_hits=3)
    case = ta.neighbour_case()
    v = tm.iou(case[1][0][0, 0, :4], case[0][0][0, :, :4])
    assert np.allclose(v, [32.0 / 48.0, 28.0 / 52.0]) and v[0] > v[1] > 0.5
    plain = tm.Model(1, **rule)
    assert [plain.update(d, c)["track_id"][0, 0] for d, c, _e in case] == [1, 1]               # the better box wins
    m = ta.Model(1, appearance=dict(dim=16), **rule)                                           # the defaults: prox 0.5, app 0.75
    outs = [m.update(d, c, e) for d, c, e in case]
    assert outs[1]["track_id"][0, 0] == 2 and outs[1]["track_cos"][0, 0] == 1.0 and m.state[0, 7] == 1
    assert m.features()[0].tolist() == [1, 2, 0, 0] and m.state[0, tm.HEADER:].reshape(4, 10)[:, 8].tolist() == [1, 0, 0, 0]
    # the tie the limits state: IoU exactly 1 with the wrong track, cosine exactly 1 with the right one - the maximum cannot separate
    # them, and the order (value, then row, then SLOT) takes the IoU pair
    tie = ta.neighbour_case(tie=True)
    m = ta.Model(1, appearance=dict(dim=16), **rule)
    outs = [m.update(d, c, e) for d, c, e in tie]
    assert outs[1]["track_id"][0, 0] == 1 and outs[1]["track_cos"][0, 0] == 0.0 and m.state[0, 7] == 0
    f = m.features()[1]
    assert abs(float(np.linalg.norm(f[0].astype(np.float64))) - 1.0) < 1e-6 and f[0, 0] > 0.9 and f[0, 1] > 0.05      # track 1's feature is now polluted


def test_the_skipped_feature_update():
    rule = dict(max_tracks=2, match_thres=0.3, max_misses=5, confirm_hits=3)
    m = ta.Model(1, appearance=dict(dim=16, alpha=0.5), **rule)
    before = None
    for d, c, e in ta.flip_case():
        o = m.update(d, c, e)
        before = m.features()[1][0].copy() if before is None else before
    assert o["track_id"][0, 0] == 1 and o["track_cos"][0, 0] == -1.0 and m.stats["skipped"] == 1
    assert m.features()[0][0] == 1 and np.array_equal(_bits(m.features()[1][0]), _bits(before))


@pytest.mark.parametrize("second", [None, True])
@pytest.mark.parametrize("motion", [None, True])
@pytest.mark.parametrize("R,M", sorted(ta.WALKS))
def test_the_random_walks_show_every_counter(R, M, motion, second):
    """the walks the device repeats: 30 frames, 2 streams, 5 % of the rows without appearance.  The model alone must show matches
    valued by the cosine, matches the IoU alone would not have made, matched rows and births without appearance and deaths - and
    the parallel form of the walk must agree with the walk as written on the fused values"""
    m, calls, shown = ta.walk_calls(R, M, motion, second)
    for k, v in ta.LEAST.items():
        assert shown.get(k, 0) >= v, (k, shown)
    assert m.state[:, 7].sum() == shown["by_appearance"]
    if second:
        assert shown["second"] >= 1 and m.state[:, 6].sum() == shown["second"]
    else:
        assert not m.state[:, 6].any()
    odd = set()
    for d, c, *_ in calls:
        odd |= {"zero" if v == 0 else "negative" if v < 0 else "beyond" if v > R else "" for v in c.tolist()}
    assert odd >= {"zero", "negative", "beyond"}
    if (R, M) == (65, 64):                                          # the parallel form on the fused values, once
        par = ta.Model(2, appearance=dict(ta.WALK_APP, dim=ta.WALKS[(R, M)][0]), second=second, motion=motion, **m.rule)
        for d, c, e, streams, _want, wstate, wfeat in calls:
            par.update(d, c, e, streams, match=tm.mutual_best)
            assert np.array_equal(par.state, wstate) and np.array_equal(par.feat, wfeat)
