"""CPU-only checks of the per-stream IoU tracker (include/yfv2.h yfv2_track_update):
  * every new symbol is declared, exported and bound, and the ABI number is still 7
  * yfv2_track_state_words' values and errors
  * yfv2_track_iou - the host entry point of the one function the kernel calls - equals the model's fp32 IoU bit for bit
  * the model's walk (the rule as written) and its parallel form (what the kernel runs) agree on random tie-heavy inputs, on the
    case that separates "a slot's best row among all rows" from "among the rows that named it", and on the chain input, whose round
    count is pinned so that it cannot quietly stop exercising the loop
  * the model's lifecycle on a hand-computed case
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import track_model as tm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


NEW = ("yfv2_track_state_words", "yfv2_track_iou", "yfv2_track_update")


def test_track_symbols_are_declared_exported_and_bound():
    m = _lib()
    hdr = open(os.path.join(REPO, "include", "yfv2.h")).read()
    declared = set(re.findall(r"YFV2_API\s+[\w\s\*]+?\b(yfv2_\w+)\s*\(", hdr))
    raw = C.CDLL(m.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in m._PROTOTYPES, name
        assert hasattr(raw, name), name
    assert m.lib().yfv2_abi_version() == m.ABI_VERSION == 7
    # int32, (pad), double, int32, float, int32, int32: the C layout on LP64
    assert C.sizeof(m.TrackRule) == 32 and m.TrackRule.match_thres.offset == 8 and m.TrackRule.init_conf.offset == 20
    import yolo_fastestv2_amd as yfv2
    assert yfv2.Tracker is yfv2.tracking.Tracker and hasattr(yfv2.Engine, "track_update")


def test_track_state_words():
    m = _lib()
    L = m.lib()
    for M in (1, 2, 64, 256, 1024):
        assert L.yfv2_track_state_words(M) == 8 + 10 * M == tm.state_words(M)
    for M in (0, -1, 1025, 2 ** 31 - 1, -2 ** 31):
        assert L.yfv2_track_state_words(M) == m.ERR_ARG, M
        assert "yfv2_track_state_words" in m.last_error()


def _c_iou(L, a, b):
    v = C.c_float(-77.0)
    assert L.yfv2_track_iou((C.c_float * 4)(*[float(x) for x in a]), (C.c_float * 4)(*[float(x) for x in b]), C.byref(v)) == 0
    return np.array([v.value], F32).view(np.uint32)[0]


def _iou_pairs():
    rng = np.random.default_rng(77)
    pairs = []

    def box(x, y, w, h):
        return np.array([x, y, x + w, y + h], F32)
    for _ in range(1500):                                   # overlapping at random, fractional corners
        a = box(rng.uniform(0, 500), rng.uniform(0, 500), rng.uniform(0.5, 200), rng.uniform(0.5, 200))
        b = a + rng.uniform(-40, 40, 4).astype(F32)
        pairs.append((a, b))
    for _ in range(300):                                    # disjoint
        a = box(rng.uniform(0, 100), rng.uniform(0, 100), rng.uniform(1, 50), rng.uniform(1, 50))
        pairs.append((a, a + F32(rng.choice([300.0, -300.0]))))
    for _ in range(300):                                    # touching: a shared edge, a shared corner
        a = box(*np.floor(rng.uniform(0, 100, 2)), *np.floor(rng.uniform(1, 50, 2)))
        w, h = a[2] - a[0], a[3] - a[1]
        pairs.append((a, a + np.array([w, 0, w, 0], F32)))
        pairs.append((a, a + np.array([w, h, w, h], F32)))
    for _ in range(300):                                    # contained, and identical
        a = box(rng.uniform(0, 100), rng.uniform(0, 100), rng.uniform(10, 50), rng.uniform(10, 50))
        pairs.append((a, a + np.array([1, 1, -1, -1], F32) * F32(rng.uniform(0, 4))))
        pairs.append((a, a.copy()))
    for _ in range(300):                                    # sub-pixel boxes
        a = box(rng.uniform(0, 10), rng.uniform(0, 10), rng.uniform(1e-3, 0.9), rng.uniform(1e-3, 0.9))
        pairs.append((a, a + rng.uniform(-0.3, 0.3, 4).astype(F32)))
    for _ in range(300):                                    # 1e30-scale boxes: areas overflow, the IoU is 0 / inf, inf / inf
        a = (rng.uniform(-1, 1, 4) * 1e30).astype(F32)
        a = np.array([min(a[0], a[2]), min(a[1], a[3]), max(a[0], a[2]), max(a[1], a[3])], F32)
        pairs.append((a, (a * F32(rng.uniform(0.5, 1.5))).astype(F32)))
        pairs.append((a, box(rng.uniform(0, 100), rng.uniform(0, 100), 10, 10)))
    for _ in range(200):                                    # each area finite, their sum (the union) overflows to infinity
        s = F32(1.5e19)
        a = np.array([0, 0, s * F32(rng.uniform(0.9, 1.1)), s], F32)
        pairs.append((a, a * F32(rng.uniform(0.9, 1.0))))
    pairs.append((np.array([0, 0, 0, 0], F32), np.array([0, 0, 0, 0], F32)))       # 0 / 0
    pairs.append((np.array([5, 5, 1, 1], F32), np.array([0, 0, 9, 9], F32)))       # an inverted box: negative extents
    return pairs


def test_track_iou_matches_the_model_bit_for_bit():
    L = _lib().lib()
    pairs = _iou_pairs()
    assert len(pairs) > 4000
    a = np.stack([p[0] for p in pairs]); b = np.stack([p[1] for p in pairs])
    want = tm.iou(a, b).view(np.uint32)
    got = np.array([_c_iou(L, x, y) for x, y in pairs], np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(pairs[i], hex(got[i]), hex(want[i])) for i in bad[:5]]
    v = want.view(F32)
    with np.errstate(invalid="ignore"):
        assert np.isnan(v).sum() > 100 and (v == 0).sum() > 300 and ((v > 0) & (v < 1)).sum() > 1500 and (v == 1).sum() >= 300   # every regime
    # hand values: half of a 2 x 1 union of two unit squares' worth; identical boxes; disjoint
    assert tm.iou([0, 0, 2, 2], [1, 0, 3, 2]) == F32(2.0) / F32(6.0)
    assert tm.iou([0, 0, 2, 2], [0, 0, 2, 2]) == F32(1.0) and tm.iou([0, 0, 2, 2], [2, 0, 4, 2]) == F32(0.0)


def test_track_iou_argument_errors():
    m = _lib()
    L = m.lib()
    a, v = (C.c_float * 4)(0, 0, 1, 1), C.c_float(-77.0)
    for args in ((None, a, C.byref(v)), (a, None, C.byref(v)), (a, a, None)):
        assert L.yfv2_track_iou(*args) == m.ERR_ARG
        assert "yfv2_track_iou" in m.last_error()
    assert v.value == -77.0


def _tie_heavy(rng, n, M):
    """rows and slots on a coarse grid: few distinct sizes and offsets, so that many edges share their IoU exactly"""
    def boxes(k):
        x, y = rng.integers(0, 6, k) * 4.0, rng.integers(0, 3, k) * 4.0
        w, h = rng.choice([8.0, 12.0], k), rng.choice([8.0, 12.0], k)
        return np.stack([x, y, x + w, y + h], axis=1).astype(F32)
    rows = np.concatenate([boxes(n), np.full((n, 1), 0.9, F32), rng.integers(0, 2, (n, 1)).astype(F32)], axis=1)
    return rows, boxes(M), rng.integers(0, 2, M).astype(F32), rng.random(M) < 0.8


def test_walk_and_parallel_form_agree_on_tie_heavy_inputs():
    rng = np.random.default_rng(5)
    most, ties = 0, 0
    for case in range(300):
        n, M = int(rng.integers(1, 24)), int(rng.integers(1, 16))
        rows, sbox, scls, live = _tie_heavy(rng, n, M)
        V, E = tm.edges(rows, sbox, scls, live, (0.0, 0.1, 0.3)[case % 3], case % 2 == 0)
        a = tm.greedy(V, E)
        b, rounds = tm.mutual_best(V, E)
        assert np.array_equal(a, b), case
        got = a[a >= 0]
        assert len(set(got.tolist())) == len(got) and E[np.nonzero(a >= 0)[0], got].all()
        most = max(most, rounds)
        vals = V[E]
        ties += int(len(vals) - len(np.unique(vals)))
    assert most >= 3 and ties > 1000        # the inputs need several rounds and are full of equal weights


def _named_only(V, E):
    """the tempting shortcut: a slot looks only at the rows that NAMED it.  Not the rule - see the test below."""
    n, M = E.shape
    K = np.where(E, tm._bits(V), 0)
    out = np.full(n, -1, np.int64)
    fr, fs = np.ones(n, bool), np.ones(M, bool)
    while True:
        Kf = np.where(fr[:, None] & fs[None, :], K, 0)
        if not (Kf > 0).any():
            return out
        named = Kf.argmax(axis=1)
        for s in range(M):
            cand = [r for r in range(n) if Kf[r].max() > 0 and named[r] == s]
            if cand:
                r = max(cand, key=lambda r: (Kf[r, s], -r))
                out[r] = s; fr[r] = False; fs[s] = False


def test_a_slot_hears_every_row_with_an_edge_not_only_those_that_named_it():
    """Slots A (x 0..10) and B (x 6..16); row 0 sits on A (IoU 9/11), row 1 between them prefers A (2/3) to B (3/7), row 2 has B alone
    (1/4).  The walk: (0, A), then (1, A) fails, (1, B) is taken, (2, B) fails.  A slot that listens only to the rows that named it
    gives B to row 2 in the first round, while row 1 is still busy losing A."""
    sbox = np.array([[0, 0, 10, 10], [6, 0, 16, 10]], F32)
    rows = np.array([[1, 0, 11, 10, 0.9, 0], [2, 0, 12, 10, 0.9, 0], [12, 0, 22, 10, 0.9, 0]], F32)
    V, E = tm.edges(rows, sbox, np.zeros(2, F32), np.ones(2, bool), 0.2, True)
    assert E.tolist() == [[True, True], [True, True], [False, True]] and V[1, 0] > V[1, 1] > V[2, 1] and V[0, 0] > V[1, 0]
    assert tm.greedy(V, E).tolist() == [0, 1, -1]
    got, rounds = tm.mutual_best(V, E)
    assert got.tolist() == [0, 1, -1] and rounds == 2
    assert _named_only(V, E).tolist() == [0, -1, 1]


def test_chain_input_needs_a_round_per_pair():
    tracks, rows = tm.chain_case(40)
    m = tm.Model(1, max_tracks=64, match_thres=0.1)
    out = m.update(tracks[None], [40])
    assert out["track_id"][0].tolist() == list(range(1, 41)) and m.state[0, :6].tolist() == [40, 40, 1, 40, 0, 0]
    slots = m.state[0, tm.HEADER:].reshape(64, tm.SLOT)
    V, E = tm.edges(rows, slots[:, :4].view(F32), slots[:, 5].view(F32), slots[:, 6] != 0, 0.1, True)
    assert int(E.sum()) == 79                               # row j - track j and row j - track j + 1, but for the last row
    walk = tm.greedy(V, E)
    par, rounds = tm.mutual_best(V, E)
    assert np.array_equal(walk, par) and walk.tolist() == list(range(40))
    assert rounds >= 32 and rounds == 40
    # every edge but the last has a heavier neighbour: the weights rise strictly along the chain
    w = [float(V[j // 2, (j + 1) // 2]) for j in range(79)]
    assert all(x < y for x, y in zip(w, w[1:]))
    out = m.update(rows[None], [40], match=tm.mutual_best)
    assert out["track_id"][0].tolist() == list(range(1, 41)) and (out["track_hits"][0] == 2).all()


def test_model_lifecycle_by_hand():
    """one stream of 2 slots, max_misses 1, confirm_hits 2: birth, match and confirmation, a miss kept, death with the freed slot
    reused in the same frame, a dropped birth, ids never reused"""
    m = tm.Model(1, max_tracks=2, match_thres=0.3, max_misses=1, confirm_hits=2, init_conf=0.5)
    A = [0, 0, 10, 10, 0.9, 1]; A2 = [1, 0, 11, 10, 0.8, 1]; Bx = [50, 50, 60, 60, 0.9, 2]; Cx = [100, 0, 110, 10, 0.9, 3]; Dx = [200, 0, 210, 10, 0.9, 3]
    weak = [300, 0, 310, 10, 0.4, 3]
    z = [0] * 6

    def step(rows, count):
        d = np.array([rows + [z] * (4 - len(rows))], F32)
        return m.update(d, [count])
    o = step([A, Bx, Cx, weak], 4)                          # two births, the third dropped; conf 0.4 < init_conf starts nothing
    assert o["track_id"][0].tolist() == [1, 2, 0, 0] and o["track_hits"][0].tolist() == [1, 1, 0, 0] and o["fresh_count"][0] == 0
    assert m.state[0, :6].tolist() == [2, 2, 1, 2, 0, 1]
    o = step([A2], 1)                                       # track 1 matched and confirmed, track 2 misses once
    assert o["track_id"][0].tolist() == [1, 0, 0, 0] and o["fresh_count"][0] == 1 and o["fresh_src"][0, 0] == 0
    assert np.array_equal(o["fresh_dets"][0, 0], np.array(A2, F32))
    s = m.state[0, tm.HEADER:].reshape(2, tm.SLOT)
    assert s[0, 6:].tolist() == [1, 2, 0, 2] and s[1, 6:].tolist() == [2, 1, 1, 2] and s[0, :6].view(F32).tolist() == [1, 0, 11, 10, F32(0.8), 1]
    o = step([A2, Cx, Dx], 3)                               # track 2 dies (2 misses > 1); Cx takes its slot at once, Dx is dropped
    assert o["track_id"][0].tolist() == [1, 3, 0, 0] and o["track_hits"][0].tolist() == [3, 1, 0, 0] and o["fresh_count"][0] == 0
    assert m.state[0, :6].tolist() == [3, 2, 3, 3, 1, 2]
    o = step([], 0)                                         # nothing seen: both miss
    o = step([], -5)                                        # ... and die (track 3 after 2 misses, track 1 likewise)
    assert m.state[0, :6].tolist() == [3, 0, 5, 3, 3, 2] and not m.state[0, tm.HEADER:].any()
    o = step([A], 9)                                        # count > R is R; the id is new
    assert o["track_id"][0].tolist() == [4, 0, 0, 0]


def _output_description_in_every_combination():
    """the package's one description of what an update returns: names, shapes and dtypes in the order the docstrings promise"""
    import itertools

    import torch
    from yolo_fastestv2_amd import tracking
    B, R = 3, 5
    i32, f32 = torch.int32, torch.float32
    for fresh, box, passes, cos in itertools.product((False, True), repeat=4):
        want = [("track_id", (B, R), i32), ("track_hits", (B, R), i32)]
        if fresh:
            want += [("fresh_dets", (B, R, 6), f32), ("fresh_src", (B, R), i32), ("fresh_count", (B,), i32)]
        want += [("track_box", (B, R, 4), f32)] * box + [("track_pass", (B, R), i32)] * passes + [("track_cos", (B, R), f32)] * cos
        assert list(tracking.outputs(B, R, fresh, box, passes, cos)) == want, (fresh, box, passes, cos)
        assert list(tracking.outputs(B, R, fresh=fresh, box=box, passes=passes, cos=cos)) == want
    assert [n for n, _, _ in tracking.outputs(B, R)] == ["track_id", "track_hits"]


def _option_errors_come_from_the_one_normaliser_under_each_callers_name():
    """motion / two_pass / appearance: None, False, True or a dict of known keys - Tracker and the two engine methods that take such
    an option refuse an unknown key with the same sentence under their own name, before anything touches a device"""
    import yolo_fastestv2_amd as yfv2
    from yolo_fastestv2_amd import tracking
    t = tracking
    assert t.MOTION_DEFAULTS == dict(std_pos=1.0 / 20, std_vel=1.0 / 160, std_meas=1.0 / 20)
    assert t.TWO_PASS_DEFAULTS == dict(high_conf=0.5, low_conf=0.1, match_thres_low=0.5, tracked_only=True)
    assert t.APPEARANCE_DEFAULTS == dict(dim=128, prox_thres=0.5, app_thres=0.75, alpha=0.9)
    for off in (None, False):
        assert t.option("x", "motion", off, t.MOTION_DEFAULTS) is None
    assert t.option("x", "motion", True, t.MOTION_DEFAULTS) == t.MOTION_DEFAULTS
    got = t.option("x", "two_pass", dict(low_conf=0, tracked_only=0), t.TWO_PASS_DEFAULTS)
    assert got == dict(high_conf=0.5, low_conf=0.0, match_thres_low=0.5, tracked_only=False)
    assert [type(v) for v in got.values()] == [float, float, float, bool]
    got = t.option("x", "appearance", dict(dim=64.0, alpha=1), t.APPEARANCE_DEFAULTS)
    assert got == dict(dim=64, prox_thres=0.5, app_thres=0.75, alpha=1.0) and type(got["dim"]) is int and type(got["alpha"]) is float
    assert t.option("x", "motion", True, t.MOTION_DEFAULTS) is not t.MOTION_DEFAULTS
    motion = "%s: motion takes std_pos, std_vel and std_meas, not ['sigma', 'zeta']"
    two = "%s: two_pass takes high_conf, low_conf, match_thres_low and tracked_only, not ['mid_conf']"
    app = "%s: appearance takes dim, prox_thres, app_thres and alpha, not ['width']"
    bad_motion, bad_two, bad_app = dict(zeta=1, std_pos=1, sigma=2), dict(mid_conf=0.3), dict(width=3)
    eng = object.__new__(yfv2.Engine)                        # no handle, no device: the option errors come first
    args = (None,) * 5
    callers = {
        ("Tracker", "motion"): lambda: yfv2.Tracker(None, 1, motion=bad_motion),
        ("Tracker", "two_pass"): lambda: yfv2.Tracker(None, 1, two_pass=bad_two),
        ("Tracker", "appearance"): lambda: yfv2.Tracker(None, 1, appearance=bad_app),
        ("track_update_two_pass", "motion"): lambda: eng.track_update_two_pass(*args, motion=bad_motion),
        ("track_update_appearance", "motion"): lambda: eng.track_update_appearance(*args, None, None, motion=bad_motion),
        ("track_update_appearance", "two_pass"): lambda: eng.track_update_appearance(*args, None, None, two_pass=bad_two),
    }
    for (caller, name), call in callers.items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == dict(motion=motion, two_pass=two, appearance=app)[name] % caller
        with pytest.raises(ValueError) as e:
            t.option(caller, name, dict(motion=bad_motion, two_pass=bad_two, appearance=bad_app)[name],
                     dict(motion=t.MOTION_DEFAULTS, two_pass=t.TWO_PASS_DEFAULTS, appearance=t.APPEARANCE_DEFAULTS)[name])
        assert str(e.value) == dict(motion=motion, two_pass=two, appearance=app)[name] % caller


def test_tracker_python_layer_states_outputs_and_options_once():
    _output_description_in_every_combination()
    _option_errors_come_from_the_one_normaliser_under_each_callers_name()
