"""CPU-only checks of the tracker's two-pass form (include/yfv2.h yfv2_track_update_two_pass):
  * the new symbol is declared, exported and bound, the ABI number is still 7
  * the model (tests/track_two_pass_model.py) with high_conf = -inf IS track_model.Model, and with motion track_motion_model.Model,
    on seeded random walks: state and every output, array_equal on bits
  * the rule's walk and its parallel form agree in both passes - also on chain_case(40) given low scores, where the data-dependent
    round count occurs in the second pass
  * the model's behaviour on the cases the device tests repeat: the dip, no birth from LOW, the pass order, tracked_only
  * the Python layer's argument errors that need no device
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import track_model as tm
import track_motion_model as mm
import track_two_pass_model as tp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_two_pass_symbol_is_declared_exported_and_bound():
    m = _lib()
    hdr = open(os.path.join(REPO, "include", "yfv2.h")).read()
    declared = set(re.findall(r"YFV2_API\s+[\w\s\*]+?\b(yfv2_\w+)\s*\(", hdr))
    raw = C.CDLL(m.LIB_PATH)
    name = "yfv2_track_update_two_pass"
    assert name in declared and name in m._PROTOTYPES and hasattr(raw, name)
    assert len(m._PROTOTYPES[name][1]) == 19 and m._PROTOTYPES[name][1][10] == C.POINTER(m.TrackSecond)
    assert m.lib().yfv2_abi_version() == m.ABI_VERSION == 7
    assert [f[0] for f in m.TrackSecond._fields_] == ["high_conf", "low_conf", "match_thres_low", "tracked_only"]
    assert C.sizeof(m.TrackSecond) == 24 and m.TrackSecond.match_thres_low.offset == 8 and m.TrackSecond.tracked_only.offset == 16
    assert "typedef struct yfv2_track_second" in hdr
    import yolo_fastestv2_amd as yfv2
    assert hasattr(yfv2.Engine, "track_update_two_pass") and "two_pass" in yfv2.Tracker.__init__.__code__.co_varnames
    assert yfv2.tracking.TWO_PASS_DEFAULTS == tp.DEFAULT


RULE = dict(max_tracks=24, match_thres=0.3, init_conf=0.3, max_misses=2, confirm_hits=3)


@pytest.mark.parametrize("motion", [None, True])
def test_high_conf_minus_inf_is_the_one_pass_model(motion):
    """-inf: every valid row is HIGH; state, header (word 6 stays 0) and all outputs are the shipped model's bits"""
    seq = tp.walk_case(21, S=3, T=25, R=40, M=24)
    one = tm.Model(3, **RULE) if motion is None else mm.Model(3, **RULE)
    two = tp.Model(3, second=tp.ONE_PASS, motion=motion, **RULE)
    assigned = 0
    for d, c in seq:
        a, b = one.update(d, c), two.update(d, c)
        assert np.array_equal(one.state, two.state)
        for k in a:
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32)), k
        assert np.array_equal(b["track_pass"], (b["track_id"] != 0).astype(np.int32))
        assigned += int((b["track_id"] != 0).sum())
    assert assigned > 500 and one.state[:, 4].sum() > 0 and one.state[:, 5].sum() > 0 and not two.state[:, 6].any()
    assert two.stats["second"] == 0


@pytest.mark.parametrize("motion", [None, True])
def test_walk_and_parallel_form_agree_in_both_passes(motion):
    seq = tp.walk_case(22, S=2, T=30, R=40, M=24)
    a = tp.Model(2, motion=motion, **RULE)
    b = tp.Model(2, motion=motion, **RULE)
    for d, c in seq:
        oa, ob = a.update(d, c, match=tm.greedy), b.update(d, c, match=tm.mutual_best)
        assert np.array_equal(a.state, b.state)
        assert all(np.array_equal(oa[k], ob[k]) for k in oa)
    assert a.stats["second"] >= 30 and a.stats["barred"] > 0 and a.stats["lost"] > 0, a.stats
    assert a.state[:, 6].sum() == a.stats["second"]
    assert max(r2 for _r1, r2 in b.stats["rounds"]) >= 1


@pytest.mark.parametrize("motion", [None, True])
def test_the_chain_in_the_second_pass(motion):
    """chain_case(40): the tracks are born HIGH, the rows come LOW - 40 rounds, all of them in the second pass"""
    tracks, rows = tm.chain_case(40)
    rows = rows.copy()
    rows[:, 4] = 0.3
    second = dict(match_thres_low=0.1)
    a = tp.Model(1, second=second, motion=motion, max_tracks=40, match_thres=0.1)
    b = tp.Model(1, second=second, motion=motion, max_tracks=40, match_thres=0.1)
    for m_, match in ((a, tm.greedy), (b, tm.mutual_best)):
        assert m_.update(tracks[None], [40], match=match)["track_id"][0].tolist() == list(range(1, 41))
    oa, ob = a.update(rows[None], [40], match=tm.greedy), b.update(rows[None], [40], match=tm.mutual_best)
    assert np.array_equal(a.state, b.state) and all(np.array_equal(oa[k], ob[k]) for k in oa)
    assert oa["track_id"][0].tolist() == list(range(1, 41)) and (oa["track_pass"][0] == 2).all() and a.state[0, 6] == 40
    assert b.stats["rounds"][-1] == (0, 40)


def _ids(model, seq, keep=None):
    ids, fresh, passes = [], 0, []
    for d, c in seq:
        if keep is not None:                                        # the caller's single threshold: rows below it removed beforehand
            d, c = d.copy(), c.copy()
            if d[0, 0, 4] < keep:
                c[0] = 0
        o = model.update(d, c)
        ids.append(int(o["track_id"][0, 0]))
        fresh += int(o["fresh_count"][0])
        passes.append(int(o["track_pass"][0, 0]) if "track_pass" in o else None)
    return ids, fresh, passes


@pytest.mark.parametrize("motion", [None, True])
def test_the_dip(motion):
    """conf 0.9 for 5 frames, 0.3 for 4, 0.9 again; max_misses 2, confirm_hits 3: one id and one fresh row in the two-pass form, two
    ids and two fresh rows through the one-pass form at a threshold of 0.5"""
    rule = dict(max_tracks=4, match_thres=0.3, max_misses=2, confirm_hits=3)
    seq = tp.dip_case()
    assert abs(float(tm.iou(seq[0][0][0, 0, :4], seq[1][0][0, 0, :4])) - 9.0 / 11.0) < 1e-6
    two = tp.Model(1, motion=motion, **rule)
    ids, fresh, passes = _ids(two, seq)
    assert ids == [1] * 12 and fresh == 1 and passes == [1] * 5 + [2] * 4 + [1] * 3
    assert two.state[0, tm.HEADER + 7] == 12 and two.state[0, 6] == 4 and two.state[0, 0] == 1
    one = tm.Model(1, **rule) if motion is None else mm.Model(1, **rule)
    ids, fresh, _ = _ids(one, seq, keep=0.5)
    assert ids == [1] * 5 + [0] * 4 + [2] * 3 and fresh == 2 and one.state[0, 0] == 2


def _box(x, y=0.0, w=10.0, h=10.0, conf=0.9, cls=0.0):
    return [x, y, x + w, y + h, conf, cls]


def _frame(rows, R=4):
    d = np.tile(np.array([900.0, 900.0, 910.0, 910.0, 0.99, 0.0], F32), (1, R, 1))
    if rows:
        d[0, :len(rows)] = np.array(rows, F32)
    return d, [len(rows)]


def test_no_birth_from_low_pass_order_and_tracked_only():
    m = tp.Model(1, max_tracks=4, match_thres=0.3, init_conf=0.7, max_misses=5, confirm_hits=2)
    o = m.update(*_frame([_box(0), _box(100, conf=0.3), _box(200, conf=0.6)]))       # HIGH; LOW far away; HIGH below init_conf
    assert o["track_id"][0].tolist() == [1, 0, 0, 0] and o["track_pass"][0].tolist() == [1, 0, 0, 0] and m.state[0, :7].tolist() == [1, 1, 1, 1, 0, 0, 0]
    # one track at x = 0..10: a HIGH row at IoU 3 / 7 = 0.43 and a LOW row at IoU 9 / 11: the HIGH row takes the slot
    o = m.update(*_frame([_box(1, conf=0.3), _box(4, conf=0.9)]))
    assert o["track_id"][0].tolist() == [0, 1, 0, 0] and o["track_pass"][0].tolist() == [0, 1, 0, 0] and m.stats["lost"] == 1
    for only, want in ((True, [0, 0, 0, 0]), (False, [1, 0, 0, 0])):
        for high_row in (False, True):
            t = tp.Model(1, second=dict(tracked_only=only), max_tracks=4, max_misses=5, confirm_hits=2)
            t.update(*_frame([_box(0)]))
            t.update(*_frame([]))                                                      # misses == 1
            o = t.update(*_frame([_box(1, conf=0.9 if high_row else 0.3)]))
            assert o["track_id"][0].tolist() == ([1, 0, 0, 0] if high_row else want), (only, high_row)
            assert t.state[0, tm.HEADER + 8] == (0 if high_row or not only else 2)
            assert t.stats["barred"] == (1 if only and not high_row else 0)


def test_python_layer_argument_errors_without_a_device():
    import torch

    import yolo_fastestv2_amd as yfv2

    class Eng:                                                      # Tracker only stores it and asks for its device
        device = torch.device("cpu")

    with pytest.raises(ValueError, match="two_pass takes"):
        yfv2.Tracker(Eng(), 2, two_pass=dict(high=0.5))
    with pytest.raises(ValueError, match="motion takes"):
        yfv2.Tracker(Eng(), 2, two_pass=True, motion=dict(std=1.0))
    tr = yfv2.Tracker(Eng(), 2, max_tracks=4, two_pass=dict(low_conf=0.2, tracked_only=0))
    assert tr.two_pass == dict(high_conf=0.5, low_conf=0.2, match_thres_low=0.5, tracked_only=False) and tuple(tr.state.shape) == (2, 8 + 10 * 4)
    assert yfv2.Tracker(Eng(), 2, max_tracks=4, two_pass=True, motion=True).state.shape[1] == 8 + 32 * 4
    assert set(tr.header(0)) == {"issued", "live", "frames", "births", "deaths", "dropped", "second"}
    assert set(yfv2.Tracker(Eng(), 2).header(0)) == {"issued", "live", "frames", "births", "deaths", "dropped"}
    d, c = torch.zeros((2, 3, 6)), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="passes=True needs"):
        yfv2.Tracker(Eng(), 2).update(d, c, passes=True)
    with pytest.raises(ValueError, match="passes=True needs"):
        yfv2.Tracker(Eng(), 2, motion=True).update(d, c, passes=True)
    with pytest.raises(ValueError, match="box=True needs"):
        tr.update(d, c, box=True)
