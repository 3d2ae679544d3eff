"""CPU-only checks of the ncnn sample's deployment path (include/yfv2.h yfv2_export_maps / yfv2_deploy_post /
yfv2_detect_deploy_frames_u8):
  * tests/deploy_model.py - the numpy statement of the rule - reproduces every record and count the reference's compiled sample
    returned for the cases of tests/golden/golden_deploy.npz (made by tests/golden/make_golden_deploy.py), bit for bit
  * equal scores rank by candidate order (the point std::sort leaves open)
  * the entry points are exported and bound, and refuse a null handle with a code
"""
import ctypes as C
import os

import numpy as np
import pytest

import deploy_model as dm
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden_deploy():
    return dict(np.load(os.path.join(GOLDEN, "golden_deploy.npz"), allow_pickle=False))


def case_args(z, c):
    in_h, in_w, classes = (int(v) for v in z[c + "_hw"])
    thresh, nms, sw, sh = (np.float32(v) for v in z[c + "_par"])
    return in_h, in_w, classes, thresh, nms, sw, sh


def test_golden_covers_the_cases_the_rule_needs(golden_deploy):
    z = golden_deploy
    names = set(str(c) for c in z["cases"])
    assert {"s32_c1", "s32_c4", "s32_c80", "s64x96_c5", "real352_c80", "dense128_c2", "hand32_c3", "hand32_c3_unit"} <= names
    assert os.path.getsize(os.path.join(GOLDEN, "golden_deploy.npz")) < 1 << 20
    assert z["s64x96_c5_map0"].shape == (4, 6, 20) and z["real352_c80_map0"].shape == (22, 22, 95)
    hand = z["hand32_c3_unit_rec"]
    assert (hand[:, 0] < 0).any()                                                   # negative coordinates, truncated toward zero
    assert ((hand[:, 0] == hand[:, 2]) & (hand[:, 1] == hand[:, 3])).sum() == 2     # two zero-area boxes on one point: 0 / 0 keeps both
    assert any((hand[:, :4] == [0, 0, 16, 16]).all(1)) and any((hand[:, :4] == [16, 0, 32, 16]).all(1))   # touching boxes: both kept
    assert tuple(z["hand32_c3_par"][2:]) == (1.5, 0.75)
    d = z["dense128_c2_rec"]
    assert float(z["dense128_c2_par"][0]) == 0.0 and len(d) < 240                   # every row a candidate, many suppressed


def test_model_reproduces_the_sample_bit_for_bit(golden_deploy):
    z = golden_deploy
    for c in (str(c) for c in z["cases"]):
        in_h, _, _, thresh, nms, sw, sh = case_args(z, c)
        rec, dropped = dm.deploy_image(z[c + "_map0"], z[c + "_map1"], z[c + "_anchors"], in_h, thresh, nms, sw, sh)
        want = z[c + "_rec"]
        assert dropped == 0, c
        assert len(rec) == len(want), "%s: %d boxes, the sample returned %d" % (c, len(rec), len(want))
        assert np.array_equal(rec, want), "%s: first differing record %s" % (c, np.argwhere(rec != want)[:1].tolist())
        score = rec[:, 5].view(np.float32)
        assert (np.diff(score) < 0).all(), c                                         # tie-free by construction: strictly descending


def _tie_maps():
    """32x32, 2 classes: scale-0 cells (0,0) and (0,1) hold the SAME values (equal scores per anchor), the scale-1 cell repeats them"""
    m0 = np.zeros((2, 2, 17), np.float32)
    m1 = np.zeros((1, 1, 17), np.float32)
    cell = np.array([0.5, 0.5, 0.5, 0.5] * 3 + [0.9, 0.9, 0.5] + [0.75, 0.25], np.float32)
    m0[0, 0] = m0[0, 1] = m0[1, 1] = cell
    m1[0, 0] = cell
    return m0, m1


def test_equal_scores_rank_by_candidate_order():
    m0, m1 = _tie_maps()
    anchors = [16.0] * 12
    rec, dropped = dm.deploy_image(m0, m1, anchors, 32, 0.3, 2.0)          # nms 2.0: nothing is suppressed, the order alone shows
    assert dropped == 0 and len(rec) == 12
    score = rec[:, 5].view(np.float32)
    hi, lo = np.float32(0.75) * np.float32(0.9), np.float32(0.75) * np.float32(0.5)
    assert np.array_equal(score, np.float32([hi] * 8 + [lo] * 4))
    # equal scores in candidate order: cell (0,0) anchors 0, 1; cell (0,1) anchors 0, 1; cell (1,1) anchors 0, 1; then the scale-1 cell
    assert rec[:8, 0].tolist() == [0, 0, 16, 16, 16, 16, 8, 8]
    assert rec[:8, 1].tolist() == [0, 0, 0, 0, 16, 16, 8, 8]
    assert rec[8:, 0].tolist() == [0, 16, 16, 8]
    # with suppression on, the FIRST of two equal, identical boxes survives: one box per distinct place, all at the high score
    rec2, _ = dm.deploy_image(m0, m1, anchors, 32, 0.3, 0.25)
    assert [tuple(int(v) for v in r[:4]) for r in rec2] == [(0, 0, 16, 16), (16, 0, 32, 16), (16, 16, 32, 32), (8, 8, 24, 24)]
    assert (rec2[:, 5].view(np.float32) == hi).all()


def test_entry_points_are_exported_and_refuse_a_null_handle():
    from yolo_fastestv2_amd import _lib as m
    if not os.path.exists(m.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = m.lib()
    raw = C.CDLL(m.LIB_PATH)
    for name in ("yfv2_export_maps", "yfv2_deploy_post", "yfv2_deploy_dropped", "yfv2_detect_deploy_frames_u8"):
        assert hasattr(raw, name) and name in m._PROTOTYPES
    assert L.yfv2_abi_version() == 7                                         # additive: the ABI number stays
    assert L.yfv2_export_maps(None, None, 1, None, None, None) == m.ERR_ARG and "null handle" in m.last_error()
    assert L.yfv2_deploy_post(None, None, None, 1, None, 0.3, 0.25, None, None, 1, None) == m.ERR_ARG
    assert L.yfv2_detect_deploy_frames_u8(None, None, 1, 0.3, 0.25, None, None, 1, None) == m.ERR_ARG
    n = C.c_int32(5)
    assert L.yfv2_deploy_dropped(None, C.byref(n), None) == m.ERR_ARG


def test_python_surface_has_the_deploy_methods():
    import yolo_fastestv2_amd as yfv2
    for name in ("export_maps", "deploy_post", "deploy_dropped", "detect_deploy_frames", "new_deploy_buffers"):
        assert callable(getattr(yfv2.Engine, name))
    assert callable(yfv2.DetectPipeline.submit_deploy_frames) and callable(yfv2.ncnn_sample.detection)
    assert yfv2.ncnn_sample.NMS_THRESH == 0.25
