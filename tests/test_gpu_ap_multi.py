"""GPU tests of average precision at K thresholds in one device pass: Engine.ap_per_class_multi / ap_per_class_multi_device /
evaluation_multi (include/yfv2.h yfv2_ap_per_class_multi, csrc/yfv2_ap.hip).  Run with ``-m gpu`` on an MI355X.

The claim is one sentence: record k equals, bit for bit and in every field, what the single-threshold entry point returns for
tp = bit k of the mask.  The single form is held against the numpy model and the reference by tests/test_gpu_ap.py; here every
case compares the multi call with K calls of it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SORT_TILE, CH = 2048, 1024       # YFV2_AP_TILE, YFV2_AP_CH
KS = (1, 10, 32)


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
def cfg():
    z = np.load(os.path.join(GOLDEN, "cfg_coco.npz"))
    return {"anchors": [float(a) for a in z["anchors"]], "classes": int(z["classes"]), "anchor_num": int(z["anchor_num"]),
            "width": int(z["width"]), "height": int(z["height"])}


@pytest.fixture(scope="module")
def images_u8():
    return np.load(os.path.join(GOLDEN, "images_u8.npz"))["images"]


@pytest.fixture(scope="module")
def coco_weights():
    return oracle.load_weights(os.path.join(GOLDEN, "weights_coco.npz"))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def to_dev(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)


def mask_tensor(mask, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(mask, np.uint32)).view(np.int32)).to(dev)


def same_record(a, b, what):
    for key in ("n_gt", "n_pred", "present"):
        assert np.array_equal(a[key], b[key]), (what, key)
    for key in ("p", "r", "ap"):
        diff = np.flatnonzero(bits(a[key]) != bits(b[key]))
        assert len(diff) == 0, "%s: %s differs in classes %s: %r / %r" % (what, key, diff[:5], a[key][diff[:5]], b[key][diff[:5]])
    assert a["bad_input"] == b["bad_input"] and a["classes_present"] == b["classes_present"], what
    assert same_bits(a["means"], b["means"]), (what, a["means"], b["means"])


def check(engine, dev, mask, conf, cls, labels, K, what=""):
    """record k of the multi call == the single call on bit k, every field"""
    mask = np.asarray(mask, np.uint32)
    conf_t, cls_t, lab_t = to_dev(conf, np.float32, dev), to_dev(cls, np.float32, dev), to_dev(np.asarray(labels).reshape(-1), np.float32, dev)
    outs = engine.ap_per_class_multi(mask_tensor(mask, dev), conf_t, cls_t, lab_t, K)
    assert len(outs) == K
    for k in range(K):
        one = engine.ap_per_class(to_dev((mask >> np.uint32(k)) & 1, np.int32, dev), conf_t, cls_t, lab_t)
        same_record(outs[k], one, "%s, K = %d, k = %d" % (what, K, k))
    return outs


def synthetic(seed, n, classes, n_gt, K, quantum=None, high_bits=False):
    rng = np.random.default_rng(seed)
    conf = rng.random(n).astype(np.float32)
    if quantum:
        conf = (np.round(conf * quantum) / quantum).astype(np.float32)
    cls = rng.integers(0, classes, n).astype(np.float32)
    # per threshold another density of true positives, as a rising threshold gives; the bits are otherwise independent
    mask = np.zeros(n, np.uint32)
    for k in range(K):
        mask |= (rng.random(n) < 0.6 * (1 - k / (K + 1.0))).astype(np.uint32) << np.uint32(k)
    if high_bits and K < 32:
        mask |= rng.integers(0, 2 ** (32 - K), n, dtype=np.uint64).astype(np.uint32) << np.uint32(K)
    labels = rng.integers(0, classes, n_gt).astype(np.float32)
    return mask, conf, cls, labels


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_which_the_sort_tile_or_the_sum_chunk_takes_another_path(engine, dev, n):
    for K in KS:
        classes = 3 + (n + K) % 3                                        # 3 to 5 classes ...
        mask, conf, cls, labels = synthetic(1000 * K + n, n, classes, 60, K)
        cls[cls == 1] = 9.0                                              # ... class 1 has targets and no predictions, class 9 the reverse
        check(engine, dev, mask, conf, cls, labels, K, "N = %d" % n)
        mask, conf, cls, labels = synthetic(2000 * K + n, n, classes, 60, K, quantum=20)     # about 20 confidence values: real ties
        cls[cls == 1] = 9.0
        check(engine, dev, mask, conf, cls, labels, K, "N = %d, ties" % n)


def test_one_class_owns_everything(engine, dev):
    n = 4 * CH + 1
    for K in KS:
        mask, conf, _, _ = synthetic(7 + K, n, 1, 1, K)
        outs = check(engine, dev, mask, conf, np.full(n, 7.0, np.float32), np.full(900, 7.0, np.float32), K, "4 chunks + 1 in class 7")
        assert all(o["n_pred"][7] == n and o["ap"][7] > 0 for o in outs)
        assert len({o["ap"][7] for o in outs}) == K                       # K different curves, not one curve K times


def test_class_254_is_present(engine, dev):
    cls = np.arange(255, dtype=np.float32)
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 1 << 10, 255).astype(np.uint32)
    mask[254] = (1 << 10) - 1
    outs = check(engine, dev, mask, rng.random(255).astype(np.float32), cls, cls[::-1].copy(), 10, "classes 0..254")
    assert all(o["classes_present"] == 255 and o["n_pred"][254] == 1 and o["ap"][254] == 1.0 and o["n_gt"][255] == 0 for o in outs)


def test_bits_at_and_above_k_are_ignored(engine, dev):
    for K in (1, 10, 31):
        mask, conf, cls, labels = synthetic(90 + K, 3000, 4, 80, K, quantum=50, high_bits=True)
        assert (mask >> np.uint32(K)).any()
        dirty = check(engine, dev, mask, conf, cls, labels, K, "high bits set")
        clean = check(engine, dev, mask & np.uint32((1 << K) - 1), conf, cls, labels, K, "high bits clear")
        for a, b in zip(dirty, clean):
            same_record(a, b, "dirty / clean")


def test_empty_targets_give_k_records_with_nan_means(yfv2, engine, dev):
    mask, conf, cls, _ = synthetic(41, 300, 5, 1, 10)
    outs = check(engine, dev, mask, conf, cls, np.zeros(0, np.float32), 10, "T = 0")
    assert len(outs) == 10
    for o in outs:
        assert o["classes_present"] == 0 and all(np.isnan(v) for v in o["means"]) and not o["n_pred"].any() and not o["ap"].any()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # np.mean of an empty list warns, in the reference as here
        got = yfv2.ap_per_class_multi_device(mask, conf, cls, np.zeros(0, np.float32), 10, device=dev)
    assert len(got) == 10 and all(len(g) == 4 and all(np.isnan(v) for v in g) for g in got)


def test_ap_per_class_multi_device_is_the_single_form_on_each_bit(yfv2, dev):
    mask, conf, cls, labels = synthetic(43, 2500, 5, 200, 10, quantum=100)
    got = yfv2.ap_per_class_multi_device(mask, conf, cls, labels, 10, device=dev)
    assert len(got) == 10
    for k, g in enumerate(got):
        want = yfv2.ap_per_class_device(((mask >> np.uint32(k)) & 1).astype(np.float64), conf, cls, labels, device=dev)
        assert len(g) == 4 and same_bits(g, want), (k, g, want)
    assert len({g[2] for g in got}) == 10


def test_bad_input_is_reported_in_every_record_and_leaves_the_handle_usable(yfv2, engine, dev):
    mask, conf, cls, labels = synthetic(51, 3000, 6, 90, 10)
    bad_conf = conf.copy()
    bad_conf[1234] = np.nan
    for c, l in ((bad_conf, labels), (conf, np.append(labels, np.float32(255.0))), (conf, np.append(labels, np.float32(3.5)))):
        outs = engine.ap_per_class_multi(mask_tensor(mask, dev), to_dev(c, np.float32, dev), to_dev(cls, np.float32, dev), to_dev(l, np.float32, dev), 10)
        assert [o["bad_input"] for o in outs] == [1] * 10
        with pytest.raises(ValueError, match="0..254"):
            yfv2.ap_per_class_multi_device(mask, c, cls, l, 10, device=dev)
        check(engine, dev, mask, conf, cls, labels, 10, "after bad input")


def test_argument_errors(engine, dev):
    from yolo_fastestv2_amd import _lib
    res = (_lib.ApResult * 32)()
    for r in res:
        r.struct_size, r.classes_present = C.sizeof(_lib.ApResult), -7
    t = torch.zeros(8, dtype=torch.float32, device=dev)
    P = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    for args in ((None, P(t), P(t), 4, P(t), 4, 10, res), (P(t), P(t), P(t), -1, P(t), 4, 10, res), (P(t), P(t), P(t), 4, None, 4, 10, res),
                 (P(t), P(t), P(t), 4, P(t), 4, 10, None), (P(t), P(t, 2), P(t), 4, P(t), 4, 10, res), (P(t), P(t), P(t), 2 ** 31, P(t), 4, 10, res),
                 (P(t), P(t), P(t), 4, P(t), 4, 0, res), (P(t), P(t), P(t), 4, P(t), 4, 33, res), (P(t), P(t), P(t), 4, P(t), 4, -1, res)):
        assert L.yfv2_ap_per_class_multi(engine._h, *args, stream) == _lib.ERR_ARG
        assert "yfv2_ap_per_class_multi" in _lib.last_error(engine._h)
    assert all(r.classes_present == -7 for r in res)
    with pytest.raises(ValueError):
        engine.ap_per_class_multi(t.int(), t, t[:4], t, 10)
    with pytest.raises(ValueError):
        engine.ap_per_class_multi(t.int().cpu(), t, t, t, 10)
    mask, conf, cls, labels = synthetic(52, 500, 4, 40, 10)
    check(engine, dev, mask, conf, cls, labels, 10, "after argument errors")


def test_cpp_host_class_reports_the_python_paths_bits(engine, dev, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "yfv2_ap_multi_test")
    if not os.path.exists(exe):      # normally prebuilt by __graft_entry__.build() and shipped with the tree
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(exe), "tests/cpp/yfv2_ap_multi_test missing: run __graft_entry__.build()"
    K = 10
    mask, conf, cls, labels = synthetic(71, 5000, 12, 700, K, quantum=256)
    path = str(tmp_path / "stats.bin")
    with open(path, "wb") as f:
        np.array([len(mask), len(labels), K], np.int64).tofile(f)
        mask.tofile(f); conf.tofile(f); cls.tofile(f); labels.tofile(f)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[:500])
    lines = r.stdout.strip().splitlines()
    outs = check(engine, dev, mask, conf, cls, labels, K, "the C++ driver's case")
    per = len(outs[0]["present"]) + 2
    assert len(lines) == K * per
    for k, m in enumerate(outs):
        blk = lines[k * per:(k + 1) * per]
        assert blk[0] == "threshold %d present %d bad 0" % (k, len(m["present"]))
        for line, c in zip(blk[1:-1], m["present"]):
            w = line.split()
            assert [int(w[0]), int(w[1]), int(w[2])] == [c, m["n_gt"][c], m["n_pred"][c]]
            assert [float.fromhex(v) for v in w[3:]] == [m["p"][c], m["r"][c], m["ap"][c]]
        assert [float.fromhex(v) for v in blk[-1].split()[1:]] == list(m["means"])


@pytest.fixture(scope="module")
def model(yfv2, dev, coco_weights):
    m = yfv2.Detector(80, 3, True).to(dev)
    missing = m.load_state_dict(coco_weights)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.eval()


@pytest.fixture(scope="module")
def loader(cfg, images_u8, coco_weights):
    """the two-batch loader of test_gpu_ap's evaluation test: reference images 0..4 in batches of 4 and 1, targets = the oracle's own
    detections at 0.3, jittered by a few pixels (IoUs spread over 0.5..0.95), plus one object per image nobody finds"""
    imgs = torch.from_numpy(images_u8[:5])
    _, _, (rows03, _) = oracle.detect(coco_weights, imgs.float() / 255.0, cfg["anchors"], cfg["height"], 0.3, 0.4)
    rng = np.random.default_rng(5)
    W, H = float(cfg["width"]), float(cfg["height"])

    def targets_for(lo, hi):
        t = []
        for b in range(lo, hi):
            for r in rows03[b]:
                bx = r[:4] + rng.normal(0, 3.0, 4).astype(np.float32)
                t.append([b - lo, r[5], (bx[0] + bx[2]) / 2 / W, (bx[1] + bx[3]) / 2 / H, (bx[2] - bx[0]) / W, (bx[3] - bx[1]) / H])
            t.append([b - lo, 79.0, 0.1, 0.1, 0.05, 0.05])
        return torch.tensor(np.asarray(t, np.float32))

    return [(imgs[0:4], targets_for(0, 4)), (imgs[4:5], targets_for(4, 5))]


def test_evaluation_multi_at_one_threshold_is_evaluation(yfv2, model, dev, cfg, loader):
    want = yfv2.evaluation(loader, cfg, model, dev, iou_thres=0.5, ap_on_device=True)
    got = yfv2.evaluation_multi(loader, cfg, model, dev, iou_thresholds=[0.5])
    assert set(got) == {"thresholds", "per_threshold", "map", "map50"}
    assert got["thresholds"].dtype == np.float32 and got["thresholds"].tolist() == [0.5] and len(got["per_threshold"]) == 1
    assert same_bits(got["per_threshold"][0], want) and want[2] > 0.2
    assert bits(got["map"]) == bits(want[2]) and bits(got["map50"]) == bits(want[2])
    assert yfv2.evaluation_multi([], cfg, model, dev) is None
    assert "map50" not in yfv2.evaluation_multi(loader, cfg, model, dev, iou_thresholds=[0.75])


def test_evaluation_multi_at_the_ten_default_thresholds(yfv2, model, dev, cfg, loader):
    got = yfv2.evaluation_multi(loader, cfg, model, dev)
    thr = got["thresholds"]
    assert thr.dtype == np.float32 and np.array_equal(thr, np.linspace(0.5, 0.95, 10).astype(np.float32)) and len(got["per_threshold"]) == 10
    singles = [yfv2.evaluation(loader, cfg, model, dev, iou_thres=float(t), ap_on_device=True) for t in thr]
    for k, (g, w) in enumerate(zip(got["per_threshold"], singles)):
        assert same_bits(g, w), (k, thr[k], g, w)
    assert bits(got["map"]) == bits(np.mean([w[2] for w in singles])) and bits(got["map50"]) == bits(singles[0][2])
    aps = [w[2] for w in singles]
    print("mAP per threshold", aps, "mAP@[.5:.95]", got["map"])
    assert aps[0] > aps[-1] and got["map"] < aps[0]          # the thresholds do something on this set
