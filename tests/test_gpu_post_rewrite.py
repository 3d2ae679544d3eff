"""Synthetic decoded tensors through Engine.nms, bit-exact against oracle.non_max_suppression: the shapes the NMS launch's
sort and greedy phases branch on (candidate counts around 64 / 1024 / 2048, one key per thread up to 1024, four per thread
at 512 x 512), all rows candidates of one class, conf ties across rows, and a class filter."""
import numpy as np
import pytest
import torch

from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    import yolo_fastestv2_amd as yfv2
    return {s: yfv2.Engine(dev, s, s, 80, 3, anchors=ANCHORS, max_batch=4) for s in (352, 512)}


def synthetic(rng, rows, n_cand, n_classes=20, tie=False, size=352):
    """(rows, 85) decoded rows: n_cand of them pass conf 0.3 (obj and dominant class score >= 0.6), the others fail on obj"""
    d = np.zeros((rows, 85), np.float32)
    d[:, 0:2] = rng.uniform(0, size, (rows, 2))
    d[:, 2:4] = (rng.uniform(0.2, 2, (rows, 2)) ** 2 * rng.uniform(10, 120, (rows, 2)))
    d[:, 4] = 0.1
    d[:, 5:] = rng.uniform(0, 0.01, (rows, 80))
    cand = rng.permutation(rows)[:n_cand]
    d[cand, 4] = rng.uniform(0.6, 1.0, n_cand)
    cls = rng.integers(0, n_classes, rows)
    d[np.arange(rows), 5 + cls] = rng.uniform(0.6, 1.0, rows)
    if tie:   # many rows with the same conf (obj and class score alike): ties broken by the lower row
        d[cand[::2], 4] = np.float32(0.75)
        d[cand[::2], 5 + cls[cand[::2]]] = np.float32(0.8)
    return d.astype(np.float32)


def check_nms(eng, dev, dec, conf, iou, classes=None):
    dets, idx, cnt = eng.nms(torch.from_numpy(dec).to(dev), conf, iou, classes=classes)
    torch.cuda.synchronize()
    o_rows, o_idx = oracle.non_max_suppression(dec, conf, iou, classes=classes)
    for b in range(dec.shape[0]):
        c = int(cnt[b])
        assert c == len(o_idx[b]), (b, c, len(o_idx[b]))
        assert np.array_equal(dets[b, :c].cpu().numpy().view(np.uint32), o_rows[b].view(np.uint32)), b
        assert np.array_equal(idx[b, :c].cpu().numpy(), o_idx[b]), b


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 1023, 1024, 1025, 1815])
def test_nms_candidate_counts(engines, dev, n_cand):
    rng = np.random.default_rng(n_cand)
    dec = np.stack([synthetic(rng, 1815, n_cand), synthetic(rng, 1815, n_cand, tie=True)])
    check_nms(engines[352], dev, dec, 0.3, 0.4)
    check_nms(engines[352], dev, dec, 0.3, 0.6)


def test_nms_all_rows_one_class(engines, dev):
    rng = np.random.default_rng(1)
    dec = np.stack([synthetic(rng, 1815, 1815, n_classes=1), synthetic(rng, 1815, 1815, n_classes=1, tie=True)])
    for iou in (0.4, 0.45, 0.6):
        check_nms(engines[352], dev, dec, 0.3, iou)


def test_nms_class_filter(engines, dev):
    rng = np.random.default_rng(2)
    dec = np.stack([synthetic(rng, 1815, 1200), synthetic(rng, 1815, 900, tie=True)])
    for classes in ([0], [3, 7, 11], list(range(10))):
        check_nms(engines[352], dev, dec, 0.3, 0.4, classes=classes)


@pytest.mark.parametrize("n_cand", [1500, 2047, 2048, 2049, 3840])
def test_nms_512(engines, dev, n_cand):
    rows = 3 * (32 * 32 + 16 * 16)
    rng = np.random.default_rng(n_cand)
    dec = np.stack([synthetic(rng, rows, n_cand, size=512), synthetic(rng, rows, n_cand, n_classes=2, tie=True, size=512)])
    check_nms(engines[512], dev, dec, 0.3, 0.45)
