"""CPU-only checks of the tracker's motion form (include/yfv2.h yfv2_track_update_motion):
  * every new symbol is declared, exported and bound, and the ABI number is still 7
  * yfv2_track_motion_state_words' values and errors
  * yfv2_track_filter_step and yfv2_track_birth - the host entry points of the one function the kernel calls - equal the model
    (tests/track_motion_model.py) bit for bit, subnormal and overflowing squares included
  * the model's behaviour: an occluded object keeps its id (and is fresh once) where the plain rule issues a second one; static
    rows give both rules the same ids; the walk and its parallel form agree on predicted boxes; a track whose width shrinks
    through zero goes blind and dies without a NaN in the state
"""
import ctypes as C
import os
import re

import numpy as np

import track_model as tm
import track_motion_model as mm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN, INF = float("nan"), float("inf")


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


NEW = ("yfv2_track_motion_state_words", "yfv2_track_filter_step", "yfv2_track_birth", "yfv2_track_update_motion")


def test_motion_symbols_are_declared_exported_and_bound():
    m = _lib()
    hdr = open(os.path.join(REPO, "include", "yfv2.h")).read()
    declared = set(re.findall(r"YFV2_API\s+[\w\s\*]+?\b(yfv2_\w+)\s*\(", hdr))
    raw = C.CDLL(m.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in m._PROTOTYPES, name
        assert hasattr(raw, name), name
    assert m.lib().yfv2_abi_version() == m.ABI_VERSION == 7
    assert C.sizeof(m.TrackMotion) == 12 and [f[0] for f in m.TrackMotion._fields_] == ["std_pos", "std_vel", "std_meas"]
    assert "typedef struct yfv2_track_motion" in hdr
    import yolo_fastestv2_amd as yfv2
    assert hasattr(yfv2.Engine, "track_update_motion") and "motion" in yfv2.Tracker.__init__.__code__.co_varnames


def test_motion_state_words():
    m = _lib()
    L = m.lib()
    for M in (1, 2, 64, 256, 1024):
        assert L.yfv2_track_motion_state_words(M) == 8 + 32 * M == mm.state_words(M)
    for M in (0, -1, 1025, 2 ** 31 - 1, -2 ** 31):
        assert L.yfv2_track_motion_state_words(M) == m.ERR_ARG, M
        assert "yfv2_track_motion_state_words" in m.last_error()


def _motion(m, d):
    return m.TrackMotion(d["std_pos"], d["std_vel"], d["std_meas"])


def _c_step(m, f, z, lp, lu, mo):
    out = (C.c_float * 5)(*([-77.0] * 5))
    zz = None if z is None else C.byref(C.c_float(float(z)))
    assert m.lib().yfv2_track_filter_step((C.c_float * 5)(*[float(v) for v in f]), zz, float(lp), float(lu), C.byref(mo), out) == 0
    return np.array(list(out), F32).view(np.int32)


def _filter_cases():
    """(filter (5), z or None, scale_predict, scale_update, motion dict): ordinary tracks, then scales over the whole fp32 range"""
    rng = np.random.default_rng(41)
    cases = []
    for i in range(1500):                                   # ordinary: a track a few frames old, pixels
        l = float(rng.uniform(4, 400))
        f = mm.birth(np.array([0, 0, l, l], F32))[0]
        f[mm.X], f[mm.V] = rng.uniform(-100, 2000), rng.uniform(-20, 20)
        f[mm.P01] = F32(rng.uniform(0, 1)) * np.sqrt(f[mm.P00] * f[mm.P11])
        mo = mm.DEFAULT if i % 3 else dict(std_pos=float(rng.uniform(0.01, 0.2)), std_vel=float(rng.uniform(0.001, 0.05)), std_meas=float(rng.uniform(0.01, 0.2)))
        z = None if i % 5 == 0 else f[mm.X] + rng.uniform(-30, 30)
        cases.append((f, z, l, l * float(rng.uniform(0.8, 1.2)), mo))
    for i in range(2500):                                   # scales 2^-75 .. 2^70: squares that are subnormal, that overflow
        e = rng.uniform(-75, 70)
        l = float(F32(2.0 ** e) * F32(rng.uniform(1, 2)))
        f = np.zeros(5, F32)
        with np.errstate(all="ignore"):
            f[mm.X] = F32(l) * F32(rng.uniform(-4, 4))
            f[mm.V] = F32(l) * F32(rng.uniform(-0.5, 0.5))
            f[mm.P00] = (F32(l) * F32(rng.uniform(0, 0.3))) ** 2
            f[mm.P11] = (F32(l) * F32(rng.uniform(0, 0.1))) ** 2
            f[mm.P01] = F32(rng.uniform(-1, 1)) * np.sqrt(f[mm.P00]) * np.sqrt(f[mm.P11])
            z = None if i % 7 == 0 else float(f[mm.X] + F32(l) * F32(rng.uniform(-1, 1)))
        cases.append((f, z, l, l if i % 2 else -l, mm.DEFAULT))
    z5 = np.zeros(5, F32)
    cases += [(z5, 0.0, 0.0, 0.0, mm.DEFAULT),                                    # s = 0: 0 / 0
              (np.array([1, 2, INF, 0, 1], F32), 3.0, 1.0, 1.0, mm.DEFAULT),      # inf / inf
              (np.array([NAN, 0, 1, 0, 1], F32), 3.0, 1.0, 1.0, mm.DEFAULT),
              (np.array([3e38, 3e38, 1, 0, 1], F32), 0.0, 1.0, 1.0, mm.DEFAULT),  # x + v overflows
              (np.array([1, 1, 1e-45, 1e-45, 1e-45], F32), 1.0, 1e-30, 1e-30, mm.DEFAULT)]
    return cases


def test_filter_step_matches_the_model_bit_for_bit():
    m = _lib()
    cases = _filter_cases()
    assert len(cases) > 4000
    sub = nonfinite = nans = 0
    for f, z, lp, lu, mo in cases:
        want = mm.predict(f, F32(lp), mo)
        if z is not None:
            want = mm.update(want, F32(z), F32(lu), mo)
        got = _c_step(m, f, z, lp, lu, _motion(m, mo))
        assert np.array_equal(got, want.view(np.int32)), (f.tolist(), z, lp, lu, mo, got.view(F32).tolist(), want.tolist())
        with np.errstate(all="ignore"):
            sub += int(((np.abs(want) > 0) & (np.abs(want) < F32(1.17549435e-38))).any())
            nonfinite += int(not np.isfinite(want).all())
            nans += int(np.isnan(want).any())
            assert (want.view(np.int32)[np.isnan(want)] == 0x7FC00000).all()             # one NaN, whatever made it
    assert sub > 50 and nonfinite > 50 and nans > 20, (sub, nonfinite, nans)             # every regime
    # by hand, all dyadic: std 1/4, 1/8, 1/2, scale 8 -> tp = 2, tv = 1, tm = 4
    mo = dict(std_pos=0.25, std_vel=0.125, std_meas=0.5)
    p = mm.predict(np.array([10, 2, 4, 1, 1], F32), F32(8), mo)
    assert p.tolist() == [12, 2, 11, 2, 2]                  # x + v; 4 + 1 + 1 + 1 + 4; 1 + 1; 1 + 1
    u = mm.update(np.array([12, 2, 16, 4, 2], F32), F32(20), F32(8), mo)
    assert u.tolist() == [16, 3, 8, 2, 1.5]                 # s = 32, k0 = 1/2, k1 = 1/8, y = 8; p11 = 2 - 4 / 8
    assert _c_step(m, [10, 2, 4, 1, 1], None, 8, 0, _motion(m, mo)).view(F32).tolist() == [12, 2, 11, 2, 2]


def test_birth_matches_the_model_bit_for_bit():
    m = _lib()
    rng = np.random.default_rng(43)
    boxes = []
    for _ in range(800):
        x, y = rng.uniform(-50, 2000, 2)
        boxes.append(np.array([x, y, x + rng.uniform(0.5, 500), y + rng.uniform(0.5, 500)], F32))
    for _ in range(800):                                    # 2^-75 .. 2^70 wide, somewhere as large
        l = F32(2.0 ** rng.uniform(-75, 70))
        x, y = (F32(rng.uniform(-2, 2)) * l for _ in range(2))
        with np.errstate(all="ignore"):
            boxes.append(np.array([x, y, x + l * F32(rng.uniform(0.5, 2)), y + l * F32(rng.uniform(0.5, 2))], F32))
    boxes += [np.array([3e38, 0, 3.2e38, 1], F32), np.array([-3e38, 0, 3e38, 1], F32), np.array([0, 0, 0, 0], F32), np.array([5, 5, 1, 1], F32)]
    sub = over = 0
    for i, b in enumerate(boxes):
        mo = mm.DEFAULT if i % 3 else dict(std_pos=float(rng.uniform(0.01, 0.2)), std_vel=float(rng.uniform(0.001, 0.05)), std_meas=0.05)
        out = (C.c_float * 20)(*([-77.0] * 20))
        assert m.lib().yfv2_track_birth((C.c_float * 4)(*[float(v) for v in b]), C.byref(_motion(m, mo)), out) == 0
        want = mm.birth(b, mo)
        assert np.array_equal(np.array(list(out), F32).view(np.int32), want.reshape(20).view(np.int32)), (b.tolist(), mo)
        with np.errstate(all="ignore"):
            sub += int(((want > 0) & (want < F32(1.17549435e-38))).any())
            over += int(np.isinf(want).any())
    assert sub > 10 and over > 10, (sub, over)
    f = mm.birth(np.array([10, 20, 18, 36], F32), dict(std_pos=0.25, std_vel=0.125, std_meas=0.5))
    assert f[:, mm.X].tolist() == [14, 28, 8, 16] and f[:, mm.P00].tolist() == [16, 64, 16, 64] and f[:, mm.P11].tolist() == [100, 400, 100, 400]
    assert not f[:, mm.V].any() and not f[:, mm.P01].any()
    assert mm.corners(f).tolist() == [10, 20, 18, 36]


def test_filter_entry_points_argument_errors():
    m = _lib()
    L = m.lib()
    f, out, z = (C.c_float * 5)(1, 0, 1, 0, 1), (C.c_float * 5)(*([-77.0] * 5)), C.c_float(1.0)
    good = m.TrackMotion(0.05, 0.00625, 0.05)
    bad = [m.TrackMotion(*v) for v in ((0.0, 0.1, 0.1), (0.1, -0.1, 0.1), (0.1, 0.1, NAN), (INF, 0.1, 0.1), (0.1, NAN, 0.1), (0.1, 0.1, 0.0))]
    for args in [(None, C.byref(z), 1.0, 1.0, C.byref(good), out), (f, C.byref(z), 1.0, 1.0, None, out), (f, C.byref(z), 1.0, 1.0, C.byref(good), None)] + \
            [(f, C.byref(z), 1.0, 1.0, C.byref(b), out) for b in bad]:
        assert L.yfv2_track_filter_step(*args) == m.ERR_ARG
        assert "yfv2_track_filter_step" in m.last_error()
    assert list(out) == [-77.0] * 5
    box, out20 = (C.c_float * 4)(0, 0, 4, 4), (C.c_float * 20)(*([-77.0] * 20))
    for args in [(None, C.byref(good), out20), (box, None, out20), (box, C.byref(good), None)] + [(box, C.byref(b), out20) for b in bad]:
        assert L.yfv2_track_birth(*args) == m.ERR_ARG
        assert "yfv2_track_birth" in m.last_error()
    assert list(out20) == [-77.0] * 20


def _run(model, seq):
    ids, fresh = [], 0
    for d, c in seq:
        o = model.update(d, c)
        ids.append(int(o["track_id"][0, 0]) if c[0] else None)
        fresh += int(o["fresh_count"][0])
    return ids, fresh


def test_occlusion_keeps_the_id_where_the_plain_rule_issues_a_second():
    """a 64 x 64 box moving 8 px / frame, seen for 10 frames, missing for 6, seen again (the issue's case and its figures)"""
    seq = mm.occlusion_case()
    motion, plain = mm.Model(1, max_tracks=4, confirm_hits=1), tm.Model(1, max_tracks=4, confirm_hits=1)
    # the figures: the returning row against the last box, and against the predicted box
    worst = 1.0
    for t, (d, c) in enumerate(seq[:-1]):
        motion.update(d, c)
        if t < 9:
            nxt = mm.predict(motion.filters()[0], mm.scales(motion.filters()[0]))
            worst = min(worst, float(tm.iou(mm.corners(nxt), seq[t + 1][0][0, 0, :4])))
    back = seq[-1][0][0, 0, :4]
    last = motion.state[0, tm.HEADER:tm.HEADER + 4].view(F32)
    nxt = mm.predict(motion.filters()[0], mm.scales(motion.filters()[0]))
    v_last, v_pred = float(tm.iou(last, back)), float(tm.iou(mm.corners(nxt), back))
    assert abs(v_last - 0.067) < 0.001 and abs(v_pred - 0.877) < 0.005 and abs(worst - 0.778) < 0.005, (v_last, v_pred, worst)
    ids_m, fresh_m = _run(mm.Model(1, max_tracks=4, confirm_hits=1), seq)
    ids_p, fresh_p = _run(plain, seq)
    assert ids_m == [1] * 10 + [None] * 6 + [1] and fresh_m == 1
    assert ids_p == [1] * 10 + [None] * 6 + [2] and fresh_p == 2
    assert motion.state[0, :6].tolist()[:2] == [1, 1]


def test_static_rows_give_both_rules_the_same_ids():
    rng = np.random.default_rng(8)
    cells = rng.permutation(64)[:24]
    xy = np.stack([cells % 8, cells // 8], axis=1) * 60.0
    rows = np.concatenate([xy, xy + rng.uniform(20, 50, (24, 2)), rng.uniform(0.3, 1, (24, 1)), rng.integers(0, 3, (24, 1))], axis=1).astype(F32)
    a, b = mm.Model(1, max_tracks=32, confirm_hits=3), tm.Model(1, max_tracks=32, confirm_hits=3)
    for t in range(10):
        perm = rng.permutation(24)
        d = rows[perm][None]
        oa, ob = a.update(d, [24]), b.update(d, [24])
        for k in ("track_id", "track_hits", "fresh_count", "fresh_src", "fresh_dets"):
            assert np.array_equal(oa[k], ob[k]), (t, k)
        assert (oa["track_hits"] == t + 1).all()
    assert np.array_equal(a.state[0, :8], b.state[0, :8])
    assert np.array_equal(a.state[0, 8:].reshape(32, 32)[:, :10], b.state[0, 8:].reshape(32, 10))
    assert not a.filters()[:24, :, mm.V].any()              # nothing moved: every innovation was zero


def test_walk_and_parallel_form_agree_on_predicted_boxes():
    """chain_case after a birth frame: the slots' boxes are the filters' predictions (born at rest, so the chain is the same chain)"""
    tracks, rows = tm.chain_case(40)
    a, b = mm.Model(1, max_tracks=64, match_thres=0.1), mm.Model(1, max_tracks=64, match_thres=0.1)
    for m_, match in ((a, tm.greedy), (b, tm.mutual_best)):
        o = m_.update(tracks[None], [40], match=match)
        assert o["track_id"][0].tolist() == list(range(1, 41))
    st = a.state[0].copy()
    filt = mm.predict(a.filters(), mm.scales(a.filters()))
    V, E = tm.edges(rows, mm.corners(filt), np.zeros(64, F32), st[tm.HEADER:].reshape(64, 32)[:, 6] != 0, 0.1, True)
    walk = tm.greedy(V, E)
    par, rounds = tm.mutual_best(V, E)
    assert np.array_equal(walk, par) and walk.tolist() == list(range(40)) and rounds == 40 and int(E.sum()) == 79
    oa, ob = a.update(rows[None], [40], match=tm.greedy), b.update(rows[None], [40], match=tm.mutual_best)
    assert oa["track_id"][0].tolist() == list(range(1, 41)) and np.array_equal(a.state, b.state)
    assert all(np.array_equal(oa[k], ob[k]) for k in oa)
    assert np.array_equal(mm.corners(mm.birth(tracks[:, :4])), tracks[:, :4])   # dyadic boxes: the corners of the born state are the row's


def test_a_shrinking_track_goes_blind_and_dies_without_a_nan():
    """w falls by 6 a frame from 40: the filter learns the velocity; then the object is gone, the predicted w runs through zero, the
    slot is blind (no edge even to a row on top of its last box) and dies of its misses"""
    m = mm.Model(1, max_tracks=2, max_misses=8, confirm_hits=1)
    for t in range(6):
        w = 40.0 - 6.0 * t
        d = np.array([[[100 - w / 2, 50, 100 + w / 2, 90, 0.9, 0]]], F32)
        assert m.update(d, [1])["track_id"][0, 0] == 1
    assert m.filters()[0, 2, mm.V] < -3
    last = m.state[0, tm.HEADER:tm.HEADER + 6].copy()
    blind_at = None
    for t in range(9):
        w = float(m.filters()[0, 2, mm.X] + m.filters()[0, 2, mm.V])           # the w this frame's predict will give
        o = m.update(np.array([[[95, 50, 105, 90, 0.9, 0]]], F32), [1] if w <= 0 else [0])
        assert np.isfinite(m.state[0, tm.HEADER:].reshape(2, 32)[:, :30].view(F32)).all()
        if t < 8:
            assert np.array_equal(m.state[0, tm.HEADER:tm.HEADER + 6], last)   # words 0..5 keep the last matched row
        if w <= 0:
            blind_at = t if blind_at is None else blind_at
            assert o["track_id"][0, 0] == 2                                     # the row on top of it starts (then continues) ANOTHER track
    assert blind_at is not None and 0 < blind_at < 8
    assert m.state[0, :6].tolist() == [2, 1, 15, 2, 1, 0]                        # track 1 died at its ninth miss
    assert not m.state[0, tm.HEADER:tm.HEADER + 32].any()                        # ... and its slot is all zero
