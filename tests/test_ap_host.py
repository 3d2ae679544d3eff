"""Average precision on the device, the part that needs no GPU: the entry points exist (library symbol, binding, Python
surface), and the numpy model of the kernels (tests/ap_model.py) holds against the reference's own ap_per_class on the goldens
(tests/golden/golden_ap.npz, made by make_golden.py from the reference's utils/utils.py).  The model is what
tests/test_gpu_ap.py compares the device with bit for bit."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import anchors_model
import ap_model as apm


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(apm.GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def model_runs(golden):
    """the model's result for every golden case, computed once"""
    runs = []
    for i in range(int(golden["n"])):
        tp, conf, cls, labels, ref = apm.load_case(golden, i)
        runs.append((apm.ap_per_class(tp, conf, cls, labels), ref))
    return runs


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_the_entry_point_is_exported_bound_and_reachable_from_python():
    import yolo_fastestv2_amd as yfv2
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert "yfv2_ap_per_class" in _lib._PROTOTYPES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "yfv2_ap_per_class")
    assert _lib.lib().yfv2_abi_version() == 7          # additive: the ABI number stays
    assert callable(yfv2.ap_per_class_device) and callable(yfv2.Engine.ap_per_class)
    assert list(inspect.signature(yfv2.ap_per_class_device).parameters) == ["tp", "conf", "pred_cls", "target_cls", "device"]
    sw = inspect.signature(yfv2.evaluation).parameters["ap_on_device"]
    assert sw.kind is inspect.Parameter.KEYWORD_ONLY and sw.default is False


def test_install_does_not_rebind_ap_per_class():
    import types

    import yolo_fastestv2_amd as yfv2
    ref = types.SimpleNamespace(ap_per_class="theirs")
    yfv2.install(reference_utils_module=ref)
    assert ref.ap_per_class == "theirs" and not hasattr(ref, "ap_per_class_device")


def test_result_struct_matches_the_header():
    from yolo_fastestv2_amd import _lib
    assert C.sizeof(_lib.ApResult) == 16 + 5 * 256 * 8 + 4 * 8
    assert _lib.ApResult.struct_size.offset == 0 and _lib.ApResult.n_gt.offset == 16 and _lib.ApResult.mean_p.offset == 16 + 5 * 2048
    header = open(os.path.join(os.path.dirname(apm.__file__), "..", "include", "yfv2.h")).read()
    body = header.split("typedef struct yfv2_ap_result {")[1].split("} yfv2_ap_result;")[0]
    assert body.count("int32_t ") == 3 and body.count("[256]") == 5 and "mean_p, mean_r, mean_ap, mean_f1" in body
    # the constants of the result's definition are the same on both sides
    internal = open(os.path.join(os.path.dirname(apm.__file__), "..", "yolo_fastestv2_amd", "csrc", "yfv2_internal.h")).read()
    assert "YFV2_AP_CH = %d;" % apm.CH in internal and "YFV2_AP_TILE = %d;" % apm.SORT_TILE in internal
    assert apm.CH == anchors_model.CH == 4 * anchors_model.LANES      # one tree: four terms per lane of tree_sum


@pytest.mark.parametrize("i", [0, 2, 3, 4, 5])
def test_model_matches_the_reference_where_no_tie_can_matter(golden, model_runs, i):
    """Cases without ties (0, 2, 3, 4) and case 5, whose ties cannot matter because every tp is 1: the stable rank is the
    reference's, so P, R and F1 are its bits.  Mean AP is summed by another tree than numpy's: it stays within (m + C) * 2**-52
    relative, the worst-case gap between two summation orders of m non-negative terms plus a C-term mean (m = the largest
    per-class true-positive count, C = the present classes) - a bound from the arithmetic, not a measured number."""
    m, ref = model_runs[i]
    tp, conf, cls, labels, _ = apm.load_case(golden, i)
    got = m["means"]
    assert bits(got[0]) == bits(ref[0]) and bits(got[1]) == bits(ref[1]) and bits(got[3]) == bits(ref[3])
    bound = apm.sum_bound(tp, cls, labels)
    assert bound <= 2.6e-14
    err = abs(got[2] - ref[2]) / ref[2] if ref[2] != 0 else abs(got[2])
    print("case %d: mean AP %r, reference %r, relative difference %.3g (bound %.3g)" % (i, got[2], float(ref[2]), err, bound))
    assert err <= bound


def test_model_on_the_case_with_ties_differs_only_in_ap(golden, model_runs):
    """Case 1 has 21 distinct confidences and mixed tp.  P, R and F1 depend on the counts alone: the reference's bits.  Mean AP
    depends on the order among equal confidences, which the reference leaves to numpy's unstable sort and the device fixes as
    the input order: the two differ (by 2.1e-4 relative when this was written), so this is a closeness check, not equality."""
    m, ref = model_runs[1]
    got = m["means"]
    assert bits(got[0]) == bits(ref[0]) and bits(got[1]) == bits(ref[1]) and bits(got[3]) == bits(ref[3])
    err = abs(got[2] - ref[2]) / ref[2]
    print("case 1: mean AP %r, reference %r, relative difference %.3g" % (got[2], float(ref[2]), err))
    assert err < 1e-3


def test_model_counts_and_absent_classes(golden, model_runs):
    m, _ = model_runs[2]                      # predictions over 80 classes, ground truth in 10
    tp, conf, cls, labels, _ = apm.load_case(golden, 2)
    assert list(m["present"]) == sorted(set(int(v) for v in labels))
    for c in range(256):
        assert m["n_gt"][c] == int((labels == c).sum())
        assert m["n_pred"][c] == (int((cls == c).sum()) if m["n_gt"][c] else 0)
    m1, _ = model_runs[1]                     # ground-truth classes nobody predicted score zero on all three
    silent = [c for c in m1["present"] if m1["n_pred"][c] == 0]
    assert silent and all(m1["p"][c] == 0 and m1["r"][c] == 0 and m1["ap"][c] == 0 for c in silent)
    assert m["bad_input"] == 0 and len(m["means_seq"]) == 4
    assert np.allclose(m["means_seq"], m["means"], rtol=1e-13, atol=0)


def test_model_rank_is_stable_and_holds_the_two_zeros_equal():
    conf = np.array([0.0, 1.0, -0.0, 1e-45, 0.0, 1.0, -0.0], np.float32)
    assert list(apm.rank(conf)) == [1, 5, 3, 0, 2, 4, 6]


def test_model_flags_bad_input_and_empty_targets():
    one = np.ones(3)
    assert apm.ap_per_class(one, [0.5, 0.25, np.nan], one, [1.0])["bad_input"] == 1
    assert apm.ap_per_class(one, [0.5, 0.25, np.inf], one, [1.0])["bad_input"] == 1
    for bad in (255.0, 3.5, -1.0, np.nan):
        assert apm.ap_per_class(one, [0.5, 0.25, 0.125], one, [1.0, bad])["bad_input"] == 1
    empty = apm.ap_per_class(one, [0.5, 0.25, 0.125], one, [])
    assert empty["bad_input"] == 0 and len(empty["present"]) == 0 and all(np.isnan(v) for v in empty["means"] + empty["means_seq"])


def test_chunked_sum_is_the_documented_tree():
    rng = np.random.RandomState(1)
    v = rng.rand(2 * apm.CH + 5)
    want = (anchors_model.tree_sum(v[:apm.CH]) + anchors_model.tree_sum(v[apm.CH:2 * apm.CH])) + anchors_model.tree_sum(v[2 * apm.CH:])
    assert apm.chunked_sum(v) == want
    assert apm.chunked_sum(np.zeros(0)) == 0.0
