"""GPU tests of average precision on the device: Engine.ap_per_class / yolo_fastestv2_amd.ap_per_class_device /
evaluation(..., ap_on_device=True) (include/yfv2.h yfv2_ap_per_class, csrc/yfv2_ap.hip).  Run with ``-m gpu`` on an MI355X.

The claim: on every case the per-class p, r, ap, n_gt, n_pred of the device and the four means of ap_per_class_device are
BIT-IDENTICAL to the numpy model of the kernels (tests/ap_model.py: stable rank, the curve's terms, the one summation tree) -
through every size at which the sort or the sum takes another path, ties, absent classes, recall above 1, degenerate and bad
input.  Where no tie can matter P, R and F1 are also the reference's own bits (tests/golden/golden_ap.npz).
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import ap_model as apm
from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert os.path.exists(yolo_fastestv2_amd.LIB_PATH), "libyfv2.so not built"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engine(yfv2, dev):
    return yfv2.Engine(dev, 64, 64, classes=2, plan={})   # any configuration will do; no weights, no anchors


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(apm.GOLDEN, allow_pickle=False))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(a, b):
    """bit equality, any NaN equal to any NaN (0 / 0 of the library and of numpy may differ in the sign bit)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def device_run(engine, dev, tp, conf, cls, labels):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)
    return engine.ap_per_class(t(np.asarray(tp) != 0, np.int32), t(conf, np.float32), t(cls, np.float32), t(np.asarray(labels).reshape(-1), np.float32))


def check(yfv2, engine, dev, tp, conf, cls, labels, what=""):
    """device == model in every bit: the per-class arrays and counts, the library's sequential means, ap_per_class_device's means"""
    m = apm.ap_per_class(tp, conf, cls, labels)
    assert m["bad_input"] == 0
    d = device_run(engine, dev, tp, conf, cls, labels)
    assert d["bad_input"] == 0 and d["classes_present"] == len(m["present"]) and np.array_equal(d["present"], m["present"])
    assert np.array_equal(d["n_gt"], m["n_gt"]) and np.array_equal(d["n_pred"], m["n_pred"]), what
    for key in ("p", "r", "ap"):
        diff = np.flatnonzero(bits(d[key]) != bits(m[key]))
        assert len(diff) == 0, "%s: %s differs from the model in classes %s: %r / %r" % (what, key, diff[:5], d[key][diff[:5]], m[key][diff[:5]])
    assert same_bits(d["means"], m["means_seq"]), (what, d["means"], m["means_seq"])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # np.mean of an empty list warns, in the reference as here
        got = yfv2.ap_per_class_device(np.asarray(tp, np.float64), conf, cls, labels, device=dev)
    assert len(got) == 4 and same_bits(got, m["means"]), (what, got, m["means"])
    return m, d, got


def synthetic(seed, n, classes, n_gt, p_tp=0.4, quantum=None):
    rng = np.random.default_rng(seed)
    conf = rng.random(n).astype(np.float32)
    if quantum:
        conf = (np.round(conf * quantum) / quantum).astype(np.float32)
    cls = rng.integers(0, classes, n).astype(np.float32)
    tp = (rng.random(n) < p_tp).astype(np.float64)
    labels = rng.integers(0, classes, n_gt).astype(np.float32)
    return tp, conf, cls, labels


@pytest.mark.parametrize("i", range(6))
def test_golden_cases_match_the_model_bit_for_bit_and_the_reference_where_ties_cannot_matter(yfv2, engine, dev, golden, i):
    tp, conf, cls, labels, ref = apm.load_case(golden, i)
    m, d, got = check(yfv2, engine, dev, tp, conf, cls, labels, "golden %d" % i)
    if i != 1:     # case 1: 21 distinct confidences and mixed tp - the reference's order among ties is numpy's accident
        assert bits(got[0]) == bits(ref[0]) and bits(got[1]) == bits(ref[1]) and bits(got[3]) == bits(ref[3])
        assert abs(got[2] - ref[2]) <= apm.sum_bound(tp, cls, labels) * abs(ref[2])
    else:
        assert bits(got[0]) == bits(ref[0]) and bits(got[1]) == bits(ref[1]) and bits(got[3]) == bits(ref[3])
        assert abs(got[2] - ref[2]) < 1e-3 * ref[2]


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, apm.SORT_TILE - 1, apm.SORT_TILE, apm.SORT_TILE + 1, apm.CH - 1, apm.CH + 1]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_wave_a_workgroup_the_sort_tile_and_the_sum_chunk(yfv2, engine, dev, n):
    tp, conf, cls, labels = synthetic(100 + n, n, 3, 40, quantum=64)     # 3 classes: segments of a few hundred; ties
    check(yfv2, engine, dev, tp, conf, cls, labels, "N = %d" % n)
    # ... and the same detections in ONE class: the segment itself has the size
    check(yfv2, engine, dev, tp, conf, np.full(n, 2.0, np.float32), labels, "N = %d, one class" % n)


def test_one_class_owns_everything(yfv2, engine, dev):
    n = 3 * apm.CH + 1
    tp, conf, _, _ = synthetic(7, n, 1, 1)
    m, d, _ = check(yfv2, engine, dev, tp, conf, np.full(n, 7.0, np.float32), np.full(900, 7.0, np.float32), "3 chunks + 1 in class 7")
    assert d["n_pred"][7] == n and d["ap"][7] > 0


def test_every_class_once_class_254_included(yfv2, engine, dev):
    cls = np.arange(255, dtype=np.float32)
    rng = np.random.default_rng(3)
    tp = (rng.random(255) < 0.5).astype(np.float64)
    tp[254] = 1
    m, d, _ = check(yfv2, engine, dev, tp, rng.random(255).astype(np.float32), cls, cls[::-1].copy(), "classes 0..254")
    assert d["classes_present"] == 255 and d["n_pred"][254] == 1 and d["ap"][254] == 1.0 and d["n_gt"][255] == 0


def test_skew_one_large_class_beside_many_single_rows(yfv2, engine, dev):
    tp, conf, _, _ = synthetic(11, 10000 + 79, 1, 1, p_tp=0.5)
    cls = np.concatenate([np.full(10000, 17.0), np.delete(np.arange(80.0), 17)]).astype(np.float32)
    perm = np.random.default_rng(12).permutation(len(cls))
    labels = np.concatenate([np.full(6000, 17.0), np.arange(80.0)]).astype(np.float32)
    check(yfv2, engine, dev, tp, conf, cls[perm], labels, "skew")


def test_ties_rank_by_input_index(yfv2, engine, dev):
    n = 1500
    tp = (np.arange(n) % 2 == 0).astype(np.float64)                       # 1, 0, 1, 0 ...
    cls = (np.arange(n) % 3).astype(np.float32)
    labels = np.array([0, 0, 1, 2, 2, 2] * 90, np.float32)
    m, d, _ = check(yfv2, engine, dev, tp, np.full(n, 0.5, np.float32), cls, labels, "all conf equal")
    # the order matters here: the reversed input gives another AP, so the bits above pin the stable order
    assert not np.array_equal(bits(m["ap"]), bits(apm.ap_per_class(tp[::-1], np.full(n, 0.5, np.float32), cls[::-1], labels)["ap"]))
    rng = np.random.default_rng(5)
    values = np.array([0.0, -0.0, 1.0, 1e-45], np.float32)                # +0 == -0 < the smallest denormal < 1
    assert values[3] > 0 and np.signbit(values[1])
    conf = values[rng.integers(0, 4, n)]
    check(yfv2, engine, dev, (rng.random(n) < 0.5).astype(np.float64), conf, cls, labels, "zeros, a denormal and 1")


def test_absent_classes_on_either_side(yfv2, engine, dev):
    tp, conf, cls, _ = synthetic(21, 700, 8, 1)
    labels = np.array([1, 1, 3, 5, 5, 5, 30, 254], np.float32)            # 30 and 254: ground truth nobody predicted
    cls[::7] = 200.0                                                      # predictions of a class without ground truth
    cls[1::50] = 2.5                                                      # ... and of no class at all
    m, d, _ = check(yfv2, engine, dev, tp, conf, cls, labels, "absent classes")
    assert d["n_pred"][30] == 0 and d["n_pred"][254] == 0 and d["p"][30] == 0 and d["ap"][254] == 0
    assert d["n_pred"][200] == 0 and d["n_gt"][200] == 0 and d["n_pred"][:8].sum() < 700


def test_recall_above_one(yfv2, engine, dev):
    # the matching pairs a detection with the best-IoU target of ANY class: a class can hold more true positives than targets
    tp = np.ones(50)
    tp[::5] = 0
    m, d, _ = check(yfv2, engine, dev, tp, np.linspace(0.9, 0.1, 50).astype(np.float32), np.full(50, 4.0, np.float32), np.full(10, 4.0, np.float32), "tpc > n_gt")
    assert d["r"][4] == 4.0 and d["ap"][4] > 1.0


@pytest.mark.parametrize("value", [0.0, 1.0])
def test_degenerate_tp(yfv2, engine, dev, value):
    _, conf, cls, labels = synthetic(31, 2500, 5, 200, quantum=20)
    m, d, _ = check(yfv2, engine, dev, np.full(2500, value), conf, cls, labels, "all tp = %g" % value)
    assert (d["ap"][:5] == 0).all() if value == 0 else (d["p"][:5] == 1).all()


def test_empty_targets_give_nan_means(yfv2, engine, dev):
    tp, conf, cls, _ = synthetic(41, 300, 5, 1)
    m, d, got = check(yfv2, engine, dev, tp, conf, cls, np.zeros(0, np.float32), "T = 0")
    assert d["classes_present"] == 0 and all(np.isnan(v) for v in d["means"]) and all(np.isnan(v) for v in got)
    assert not d["n_pred"].any() and not d["ap"].any()


def test_bad_input_is_reported_and_leaves_the_handle_usable(yfv2, engine, dev):
    tp, conf, cls, labels = synthetic(51, 3000, 6, 90)
    bad_conf = conf.copy()
    bad_conf[1234] = np.nan
    for c, l in ((bad_conf, labels), (conf, np.append(labels, np.float32(255.0))), (conf, np.append(labels, np.float32(3.5)))):
        assert apm.ap_per_class(tp, c, cls, l)["bad_input"] == 1
        assert device_run(engine, dev, tp, c, cls, l)["bad_input"] == 1
        with pytest.raises(ValueError, match="0..254"):
            yfv2.ap_per_class_device(tp, c, cls, l, device=dev)
        check(yfv2, engine, dev, tp, conf, cls, labels, "after bad input")


def test_argument_errors(yfv2, engine, dev):
    import ctypes as C

    from yolo_fastestv2_amd import _lib
    res = _lib.ApResult()
    res.struct_size, res.classes_present = C.sizeof(_lib.ApResult), -7
    t = torch.zeros(8, dtype=torch.float32, device=dev)
    P = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    for args in ((None, P(t), P(t), 4, P(t), 4, C.byref(res)), (P(t), P(t), P(t), -1, P(t), 4, C.byref(res)), (P(t), P(t), P(t), 4, None, 4, C.byref(res)),
                 (P(t), P(t), P(t), 4, P(t), 4, None), (P(t), P(t, 2), P(t), 4, P(t), 4, C.byref(res)), (P(t), P(t), P(t), 2 ** 31, P(t), 4, C.byref(res))):
        assert L.yfv2_ap_per_class(engine._h, *args, stream) == _lib.ERR_ARG
        assert "yfv2_ap_per_class" in _lib.last_error(engine._h)
    assert res.classes_present == -7
    with pytest.raises(ValueError):
        engine.ap_per_class(t.int(), t, t[:4], t)
    with pytest.raises(ValueError):
        engine.ap_per_class(t.int().cpu(), t, t, t)


def test_a_larger_set_with_real_ties_twice(yfv2, engine, dev):
    tp, conf, cls, labels = synthetic(61, 200001, 80, 60000, quantum=4096)      # ~49 rows per confidence value: ties in every class
    m, d, _ = check(yfv2, engine, dev, tp, conf, cls, labels, "N = 200001")
    again = device_run(engine, dev, tp, conf, cls, labels)
    for key in ("p", "r", "ap"):
        assert np.array_equal(bits(again[key]), bits(d[key]))
    assert again["means"] == d["means"] and np.array_equal(again["n_pred"], d["n_pred"])


def test_a_set_whose_table_rows_need_several_scan_steps(yfv2, engine, dev):
    """ap_scan_kernel walks a digit's row of the (digit, tile) table 256 tiles at a time with a carry.  Up to 256 tiles
    (524 288 detections) that loop runs once; here it runs three times, the last time on a tail of 2 tiles - the regime of a
    real validation set (1.5 M rows: 733 tiles)."""
    n = 2 * 256 * apm.SORT_TILE + apm.SORT_TILE + 1
    assert -(-n // apm.SORT_TILE) == 514 and 514 % 256 != 0
    tp, conf, cls, labels = synthetic(81, n, 80, 30000, quantum=65536)      # ~16 rows per confidence value: ties in every class
    m, d, _ = check(yfv2, engine, dev, tp, conf, cls, labels, "N = %d" % n)
    assert d["n_pred"][:80].sum() == n and d["n_pred"][:80].min() > 12 * apm.CH


def test_ap_per_class_device_refuses_a_device_that_is_not_the_gpu(yfv2):
    with pytest.raises(RuntimeError, match="no CPU path"):
        yfv2.ap_per_class_device([1.0], [0.5], [0.0], [0.0], device="cpu")


def test_cpp_host_class_reports_the_models_bits(yfv2, engine, dev, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "yfv2_ap_test")
    if not os.path.exists(exe):      # normally prebuilt by __graft_entry__.build() and shipped with the tree
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(exe), "tests/cpp/yfv2_ap_test missing: run __graft_entry__.build()"
    tp, conf, cls, labels = synthetic(71, 5000, 12, 700, quantum=256)
    path = str(tmp_path / "stats.bin")
    with open(path, "wb") as f:
        np.array([len(tp), len(labels)], np.int64).tofile(f)
        tp.astype(np.int32).tofile(f); conf.tofile(f); cls.tofile(f); labels.tofile(f)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[:500])
    lines = r.stdout.strip().splitlines()
    m = apm.ap_per_class(tp, conf, cls, labels)
    assert lines[0] == "present %d bad 0" % len(m["present"]) and len(lines) == len(m["present"]) + 2
    for line, c in zip(lines[1:-1], m["present"]):
        w = line.split()
        assert [int(w[0]), int(w[1]), int(w[2])] == [c, m["n_gt"][c], m["n_pred"][c]]
        assert [float.fromhex(v) for v in w[3:]] == [m["p"][c], m["r"][c], m["ap"][c]]
    assert [float.fromhex(v) for v in lines[-1].split()[1:]] == list(m["means_seq"])


@pytest.fixture(scope="module")
def model(yfv2, dev, coco_weights):
    m = yfv2.Detector(80, 3, True).to(dev)
    missing = m.load_state_dict(coco_weights)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.eval()


def test_evaluation_with_the_ap_on_the_device(yfv2, model, dev, cfg, images_u8, coco_weights, monkeypatch):
    """evaluation(..., ap_on_device=True) over the two-batch loader of test_gpu_parity's evaluation test (reference images, targets
    derived from the oracle's own detections at 0.3): the arrays the run hands to Engine.ap_per_class go through the model -
    bit-equal - and the default path's four means agree within (m + C) * 2**-52, because on this subset no two kept detections
    of one class share a confidence, which is asserted first.  The subset is images 0..4 in batches of 4 and 1: image 5 of the
    shipped set is a copy of image 4, so with it every detection of image 4 would tie with its twin."""
    imgs = torch.from_numpy(images_u8[:5])
    x = imgs.float() / 255.0
    _, _, (rows03, _) = oracle.detect(coco_weights, x, cfg["anchors"], cfg["height"], 0.3, 0.4)
    rng = np.random.default_rng(5)
    W, H = float(cfg["width"]), float(cfg["height"])

    def targets_for(lo, hi):
        t = []
        for b in range(lo, hi):
            for r in rows03[b]:
                bx = r[:4] + rng.normal(0, 3.0, 4).astype(np.float32)
                t.append([b - lo, r[5], (bx[0] + bx[2]) / 2 / W, (bx[1] + bx[3]) / 2 / H, (bx[2] - bx[0]) / W, (bx[3] - bx[1]) / H])
            t.append([b - lo, 79.0, 0.1, 0.1, 0.05, 0.05])      # a ground-truth object nobody finds
        return torch.tensor(np.asarray(t, np.float32))

    loader = [(imgs[0:4], targets_for(0, 4)), (imgs[4:5], targets_for(4, 5))]
    seen = []
    plain = yfv2.Engine.ap_per_class

    def recording(self, tp, conf, pred_cls, target_cls):
        seen.append([t.cpu().numpy() for t in (tp, conf, pred_cls, target_cls)] + [t.device for t in (tp, conf, pred_cls, target_cls)])
        return plain(self, tp, conf, pred_cls, target_cls)

    monkeypatch.setattr(yfv2.Engine, "ap_per_class", recording)
    got = yfv2.evaluation(loader, cfg, model, dev, ap_on_device=True)
    assert got is not None and len(got) == 4 and len(seen) == 1
    tp, conf, cls, labels = seen[0][:4]
    assert all(d == dev for d in seen[0][4:]) and tp.dtype == np.int32 and len(labels) == sum(len(t) for _, t in loader)
    m = apm.ap_per_class(tp, conf, cls, labels)
    assert same_bits(got, m["means"]) and got[2] > 0.2

    for c in np.unique(cls):          # the condition under which the stable rank IS the reference's rank
        mine = conf[cls == c]
        assert len(np.unique(mine)) == len(mine), "class %d holds two detections of one confidence" % int(c)
    want = yfv2.evaluation(loader, cfg, model, dev)
    bound = apm.sum_bound(tp, cls, labels)
    print("device %r\nhost   %r\nbound %.3g" % (got, want, bound))
    for g, w in zip(got, want):
        assert abs(g - w) <= bound * abs(w)
    assert yfv2.evaluation([], cfg, model, dev, ap_on_device=True) is None
