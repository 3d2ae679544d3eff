"""The CPU oracle's non_max_suppression against the reference's own, on crafted decoded tensors (tests/adversarial_post.py,
fixture tests/golden/golden_post_adversarial.npz made by make_golden.py adversarial): NaN class scores (torch.max propagates
them, the row is dropped), negative and signed-zero conf, objectness and conf exactly at conf_thres, IoU exactly at iou_thres,
zero-area boxes, negative / zero / unit IoU thresholds, a class filter.  The GPU NMS is held to the same fixture
(tests/test_gpu_post_adversarial.py); this pins the oracle it is also compared with.  CPU only."""
import os

import numpy as np
import pytest

import adversarial_post as A
from conftest import GOLDEN
from oracle import yfv2_oracle as oracle


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_post_adversarial.npz")))


def test_fixture_grid_is_the_builders_grid(golden):
    assert [tuple(c) for c in golden["configs"]] == list(A.DECODED_CONFIGS)
    assert list(golden["conf_thres"]) == list(A.CONF_THRES) and list(golden["iou_thres"]) == list(A.IOU_THRES)
    assert list(golden["cases"]) == [n for n, _ in A.DECODED_CASES]
    assert golden["result"].shape == (len(A.DECODED_CONFIGS), len(A.CONF_THRES), len(A.IOU_THRES), len(A.CLASS_FILTER), len(A.DECODED_CASES))
    assert (golden["result"] >= 0).all()


@pytest.mark.parametrize("c", range(len(A.DECODED_CONFIGS)), ids=["%d-rows-%d-classes" % rc for rc in A.DECODED_CONFIGS])
def test_oracle_nms_equals_reference_on_crafted_rows(golden, c):
    rows, nc = A.DECODED_CONFIGS[c]
    dec = A.decoded_batch(rows, nc)
    assert np.array_equal(A.probe(dec), golden["probe%d" % c]), "the builders no longer make the inputs the fixture was made from"
    with np.errstate(invalid="ignore"):
        for a, ct in enumerate(A.CONF_THRES):
            for i, it in enumerate(A.IOU_THRES):
                for f, cl in enumerate(A.CLASS_FILTER):
                    o_rows, o_idx = oracle.non_max_suppression(dec, ct, it, classes=None if cl is None else list(cl))
                    for b in range(dec.shape[0]):
                        g_rows, g_idx = A.golden_result(golden, c, a, i, f, b)
                        where = (A.DECODED_CASES[b][0], ct, it, cl)
                        assert A.same_bits(o_rows[b], g_rows), where
                        assert np.array_equal(o_idx[b], g_idx), where


def test_fixture_reaches_the_edges(golden):
    """the fixture is not vacuous: the crafted rows change the outcome where the kernel used to differ"""
    dec = A.decoded_batch(1815, 80)
    nan_img = A.DECODED_CASES.index(("nan_and_signs", A._nan_and_signs))
    g_rows, g_idx = A.golden_result(golden, 0, 0, 0, 0, nan_img)          # conf 0.3, iou 0.4
    nan_rows = np.flatnonzero(np.isnan(dec[nan_img, :, 5:]).any(1) & (dec[nan_img, :, 4] > 0.3))
    assert nan_rows.size >= 5 and not np.isin(g_idx, nan_rows).any()     # rows with a NaN class score are dropped
    g_rows, _ = A.golden_result(golden, 0, A.CONF_THRES.index(-1.0), 0, 0, nan_img)
    conf = g_rows[:, 4]
    assert (conf < 0).any() and (np.signbit(conf) & (conf == 0)).any()   # negative and -0.0 conf survive at conf_thres -1
    assert np.all(np.diff(conf[np.isfinite(conf)].astype(np.float64)) <= 0)
    tie = A.DECODED_CASES.index(("tie_cut", A._tie_cut))
    g_rows, g_idx = A.golden_result(golden, 0, 0, 0, 0, tie)
    assert len(g_idx) == 300 and (g_rows[:, 4] == np.float32(0.5)).sum() > 200
