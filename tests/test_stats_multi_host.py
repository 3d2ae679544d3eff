"""Matching at K IoU thresholds, the part that needs no GPU: the numpy statement of the two-phase rule (tests/stats_multi_model.py:
best target once, one walk per threshold) gives the reference's get_batch_statistics at every threshold - on the detections and
targets of tests/golden/golden_stats.npz, whose flags at 0.5 and 0.75 are the reference's own, at the ten COCO thresholds, and on
hand-built cases.  The model is what tests/test_gpu_stats_multi.py holds the device against, next to K single-threshold launches."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import stats_multi_model as smm
from conftest import unpack_ragged
from oracle import yfv2_oracle as oracle


def test_two_phase_rule_is_the_reference_at_the_ten_coco_thresholds(golden_stats):
    dets, _ = unpack_ragged(golden_stats, "dets")
    targets = golden_stats["targets"]
    got = smm.batch_statistics_multi(dets, targets, smm.COCO_THRESHOLDS)
    want = smm.reference_masks(dets, targets, smm.COCO_THRESHOLDS)
    assert len(got) == len(dets) and all(np.array_equal(g, w) for g, w in zip(got, want))
    flat = np.concatenate(got)
    assert flat.max() < (1 << 10) and (flat & 1).any() and ((flat >> 9) & 1).sum() < (flat & 1).sum()
    # bit 0 (0.5) is the reference's own recorded flags; 0.75 is between two COCO values, so it gets a run of its own
    assert np.array_equal((flat & 1).astype(np.uint8), golden_stats["tp_050"])
    at075 = np.concatenate(smm.batch_statistics_multi(dets, targets, [0.75]))
    assert np.array_equal(at075.astype(np.uint8), golden_stats["tp_075"])


@pytest.mark.parametrize("name", sorted(smm.hand_cases()))
def test_two_phase_rule_on_the_hand_built_cases(name):
    outputs, targets, thr = smm.hand_cases()[name]
    got = smm.batch_statistics_multi(outputs, targets, thr)
    want = smm.reference_masks(outputs, targets, thr)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), (name, got, want)


def test_hand_built_cases_show_what_they_were_built_for():
    cases = smm.hand_cases()
    o, t, thr = cases["threshold equals the iou"]
    assert oracle.bbox_iou_plus1(o[0][0, :4], t[:1, 2:])[0] == np.float32(0.5) and oracle.bbox_iou_plus1(o[0][1, :4], t[1:, 2:])[0] == np.float32(0.25)
    m = smm.batch_statistics_multi(o, t, thr)[0]
    assert m.tolist() == [0b11101, 0b01000]            # 0.5: hit at 0.5 and below it, miss one ulp above; 0.25: hit at 0.25 only
    o, t, thr = cases["non-monotone tp"]
    first, second = smm.batch_statistics_multi(o, t, thr)[0]
    bit = lambda v, k: (int(v) >> k) & 1
    assert bit(first, 0) == 1 and bit(second, 0) == 0          # at 0.5 the higher-ranked detection takes the shared target
    assert bit(first, 5) == 0 and bit(second, 5) == 1          # at 0.75 it fails and the lower-ranked one hits
    assert bit(second, 9) == 0                                  # at 0.95 nobody does: 0, 1, 0 along k - not monotone
    o, t, thr = cases["unsorted thresholds, a repeat, a NaN, out of range"]
    first, second = smm.batch_statistics_multi(o, t, thr)[0]
    assert bit(first, 2) == 0 and bit(second, 2) == 0 and bit(first, 1) == bit(first, 3) == 1 and bit(first, 5) == 1 and bit(second, 6) == 0
    o, t, thr = cases["label not among the targets"]
    m = smm.batch_statistics_multi(o, t, thr)
    assert m[0][0] == 0 and m[0][1] == 0b0001111111 and m[0][2] == 0b0111111111
    assert m[1][0] == 0                                     # IoU 1 with its image's only target, whose label is another


def test_the_entry_points_are_exported_bound_and_reachable_from_python():
    import yolo_fastestv2_amd as yfv2
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("yfv2_batch_statistics_multi", "yfv2_batch_statistics_multi_async", "yfv2_ap_per_class_multi"):
        assert name in _lib._PROTOTYPES and hasattr(L, name), name
    assert _lib.lib().yfv2_abi_version() == 7          # additive: the ABI number stays
    assert list(inspect.signature(yfv2.Engine.batch_statistics_multi).parameters) == ["self", "dets", "cnt", "targets", "thresholds", "sync"]
    assert list(inspect.signature(yfv2.Engine.ap_per_class_multi).parameters) == ["self", "tpmask", "conf", "pred_cls", "target_cls", "K"]
    assert list(inspect.signature(yfv2.ap_per_class_multi_device).parameters) == ["tpmask", "conf", "pred_cls", "target_cls", "K", "device"]
    p = inspect.signature(yfv2.evaluation_multi).parameters
    assert list(p) == ["val_dataloader", "cfg", "model", "device", "conf_thres", "nms_thresh", "iou_thresholds"] and p["iou_thresholds"].default is None
    assert "ap_on_device" in inspect.signature(yfv2.evaluation).parameters and "iou_thresholds" not in inspect.signature(yfv2.evaluation).parameters
    for fn in (yfv2.evaluation_multi, yfv2.ap_per_class_multi_device, yfv2.Engine.ap_per_class_multi):
        assert "101-point" in fn.__doc__ and "crowd" in fn.__doc__ and "area ranges" in fn.__doc__


def test_evaluation_multi_has_no_cpu_path():
    import yolo_fastestv2_amd as yfv2
    with pytest.raises(RuntimeError, match="no CPU path"):
        yfv2.evaluation_multi([], {}, None, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path|no MI355X"):
        yfv2.ap_per_class_multi_device([1], [0.5], [0.0], [0.0], 1, device="cpu")
