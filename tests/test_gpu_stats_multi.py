"""GPU tests of matching at K IoU thresholds in one launch: Engine.batch_statistics_multi (include/yfv2.h
yfv2_batch_statistics_multi, csrc/yfv2_post.hip stats_multi_kernel).  Run with ``-m gpu`` on an MI355X.

The claim is one sentence: bit k of the mask equals what the single-threshold call writes to tp at thresholds[k].  Every case
compares the multi launch with K launches of the existing entry point; the hand-built cases are also held against the numpy
statement of the two-phase rule (tests/stats_multi_model.py), which test_stats_multi_host.py holds against the reference."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stats_multi_model as smm

pytestmark = pytest.mark.gpu
MAX_DET = 300


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


def pack(outputs, dev, fill=0.0):
    """list of (n_i, 6) -> padded (B, 300, 6) device rows and counts; rows past the count hold `fill` and must never matter"""
    B = len(outputs)
    dets = np.full((B, MAX_DET, 6), fill, np.float32)
    cnt = np.zeros(B, np.int32)
    for b, o in enumerate(outputs):
        o = np.asarray(o, np.float32).reshape(-1, 6)
        dets[b, :len(o)] = o
        cnt[b] = len(o)
    return torch.from_numpy(dets).to(dev), torch.from_numpy(cnt).to(dev)


def masks_of(t):
    return t.cpu().numpy().view(np.uint32)


def compare_with_single_launches(engine, dets, cnt, targets, thr):
    """-> the (B, 300) uint32 mask, after asserting bit k == tp of the single-threshold launch at thr[k], bits >= K == 0"""
    thr = np.asarray(thr, np.float32)
    got = masks_of(engine.batch_statistics_multi(dets, cnt, targets, thr, sync=False))
    assert got.shape == (dets.shape[0], MAX_DET) and got.dtype == np.uint32
    for k, t in enumerate(thr):
        tp = engine.batch_statistics(dets, cnt, targets, float(t), sync=False).cpu().numpy()
        assert tp.max() <= 1
        bad = np.argwhere(((got >> np.uint32(k)) & 1) != tp.astype(np.uint32))
        assert len(bad) == 0, "threshold %d (%r): bit differs from tp at (image, row) %s" % (k, t, bad[:5].tolist())
    if len(thr) < 32:
        assert (got >> np.uint32(len(thr))).max() == 0
    return got


def synthetic(seed, counts, tcounts):
    """per image: `counts[b]` detections with integer corners and `tcounts[b]` targets, most of them jittered copies of detections
    (IoU anywhere in 0.3..1, ties included), labels 0..4 on the targets and 0..5 on the detections; target rows interleaved"""
    rng = np.random.default_rng(seed)
    outputs, rows = [], []
    for b, (n, nt) in enumerate(zip(counts, tcounts)):
        xy = rng.integers(0, 300, (n, 2)).astype(np.float32)
        wh = rng.integers(10, 90, (n, 2)).astype(np.float32)
        conf = np.sort(rng.random(n).astype(np.float32))[::-1]
        o = np.concatenate([xy, xy + wh, conf[:, None], rng.integers(0, 6, (n, 1)).astype(np.float32)], 1)
        outputs.append(o)
        for j in range(nt):
            if n and rng.random() < 0.8:
                src = o[rng.integers(0, n)]
                box = src[:4] + rng.integers(-8, 9, 4).astype(np.float32)
                lab = src[5] if rng.random() < 0.7 else float(rng.integers(0, 5))
                lab = min(lab, 4.0)
            else:
                p = rng.integers(0, 300, 2).astype(np.float32)
                box = np.concatenate([p, p + rng.integers(10, 90, 2).astype(np.float32)])
                lab = float(rng.integers(0, 5))
            rows.append([b, lab, *box])
    targets = np.asarray(rows, np.float32).reshape(-1, 6)
    return outputs, targets[rng.permutation(len(targets))]


THRESHOLDS = {1: np.float32([0.5]), 10: smm.COCO_THRESHOLDS,
              32: np.random.default_rng(1).permutation(np.linspace(0.05, 0.98, 32)).astype(np.float32)}


@pytest.mark.parametrize("tcounts", [(0, 1, 65, 1024), (1024, 65, 1, 0), (65, 1024, 0, 1)])
@pytest.mark.parametrize("K", [1, 10, 32])
def test_bit_k_is_the_single_launch_at_threshold_k(engine, dev, K, tcounts):
    counts = (0, 1, 64, 300)
    outputs, targets = synthetic(17, counts, tcounts)
    dets, cnt = pack(outputs, dev, fill=np.nan)
    got = compare_with_single_launches(engine, dets, cnt, torch.from_numpy(targets), THRESHOLDS[K])
    for b, (n, nt) in enumerate(zip(counts, tcounts)):
        assert not got[b, n:].any()
        if n > 1 and nt > 1:
            assert got[b, :n].any(), "image %d: the case matches nothing at any threshold and shows nothing" % b
    assert engine.stats_overflowed() == 0


@pytest.mark.parametrize("name", sorted(smm.hand_cases()))
def test_hand_built_cases(engine, dev, name):
    outputs, targets, thr = smm.hand_cases()[name]
    dets, cnt = pack(outputs, dev)
    got = compare_with_single_launches(engine, dets, cnt, torch.from_numpy(targets), thr)
    want = smm.batch_statistics_multi(outputs, targets, thr)
    for b, w in enumerate(want):
        assert got[b, :len(w)].tolist() == w.tolist(), (name, b)


def test_threshold_equal_to_the_iou_hits(engine, dev):
    outputs, targets, thr = smm.hand_cases()["threshold equals the iou"]
    dets, cnt = pack(outputs, dev)
    got = masks_of(engine.batch_statistics_multi(dets, cnt, torch.from_numpy(targets), thr))
    assert got[0, :2].tolist() == [0b11101, 0b01000]   # IoU 0.5: hit at 0.5 and one ulp below, miss one ulp above; IoU 0.25: hit at 0.25 alone


def test_tp_is_not_monotone_in_the_threshold(engine, dev):
    outputs, targets, thr = smm.hand_cases()["non-monotone tp"]
    dets, cnt = pack(outputs, dev)
    first, second = masks_of(engine.batch_statistics_multi(dets, cnt, torch.from_numpy(targets), thr))[0, :2]
    bit = lambda v, k: (int(v) >> k) & 1
    assert [bit(first, k) for k in range(10)] == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert [bit(second, k) for k in range(10)] == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0]     # 0 at 0.5, 1 at 0.75, 0 at 0.95


def test_unsorted_thresholds_with_a_repeat_and_a_nan(engine, dev):
    outputs, targets, thr = smm.hand_cases()["unsorted thresholds, a repeat, a NaN, out of range"]
    assert np.isnan(thr[2]) and thr[1] == thr[3] and thr[0] > thr[1]
    dets, cnt = pack(outputs, dev)
    got = masks_of(engine.batch_statistics_multi(dets, cnt, torch.from_numpy(targets), thr))[0, :2]
    bit = lambda v, k: (int(v) >> k) & 1
    assert bit(got[0], 2) == 0 and bit(got[1], 2) == 0                    # NaN: nothing
    assert all(bit(g, 1) == bit(g, 3) for g in got)                       # the repeat: the same column twice
    assert [bit(got[0], k) for k in range(8)] == [0, 1, 0, 1, 0, 1, 0, 1] and [bit(got[1], k) for k in range(8)] == [1, 0, 0, 0, 1, 0, 0, 0]


def test_label_not_among_the_targets(engine, dev):
    outputs, targets, thr = smm.hand_cases()["label not among the targets"]
    dets, cnt = pack(outputs, dev)
    got = masks_of(engine.batch_statistics_multi(dets, cnt, torch.from_numpy(targets), thr))
    assert got[0, 0] == 0 and got[0, 1] == 0b0001111111 and got[0, 2] == 0b0111111111 and got[1, 0] == 0


def test_1025_targets_in_one_image_set_the_sticky_flag_once(yfv2, engine, dev):
    outputs, _ = synthetic(5, (10, 10), (0, 0))
    dets, cnt = pack(outputs, dev)
    t = np.zeros((1025 + 3, 6), np.float32)
    t[:1025, 0], t[1025:, 0] = 1, 0
    t[:, 2:] = [10, 10, 50, 50]
    assert engine.stats_overflowed() == 0
    engine.batch_statistics_multi(dets, cnt, torch.from_numpy(t), smm.COCO_THRESHOLDS, sync=False)
    assert engine.stats_overflowed() == 1
    assert engine.stats_overflowed() == 0
    with pytest.raises(yfv2.Yfv2Error, match="1024 targets"):
        engine.batch_statistics_multi(dets, cnt, torch.from_numpy(t), smm.COCO_THRESHOLDS)
    assert engine.stats_overflowed() == 0
    engine.batch_statistics_multi(dets, cnt, torch.from_numpy(t[1:]), smm.COCO_THRESHOLDS)       # 1024: fine


def test_argument_errors_leave_the_handle_usable(engine, dev):
    from yolo_fastestv2_amd import _lib
    outputs, targets = synthetic(6, (5, 7), (4, 4))
    dets, cnt = pack(outputs, dev)
    tg = torch.from_numpy(targets).to(dev)
    mask = torch.full((2, MAX_DET), -7, dtype=torch.int32, device=dev)
    thr = (C.c_float * 33)(*([0.5] * 33))
    P = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    for fn in (L.yfv2_batch_statistics_multi, L.yfv2_batch_statistics_multi_async):
        for K, th, out in ((0, thr, P(mask)), (33, thr, P(mask)), (-1, thr, P(mask)), (10, None, P(mask)), (10, thr, None)):
            assert fn(engine._h, P(dets), P(cnt), 2, P(tg), len(targets), th, K, out, stream) == _lib.ERR_ARG
            assert "yfv2_batch_statistics_multi" in _lib.last_error(engine._h)
        assert fn(engine._h, None, P(cnt), 2, P(tg), len(targets), thr, 10, P(mask), stream) == _lib.ERR_ARG
        assert fn(engine._h, P(dets), P(cnt), 0, P(tg), len(targets), thr, 10, P(mask), stream) == _lib.ERR_BATCH
    torch.cuda.synchronize(dev)
    assert (mask == -7).all()                      # nothing was enqueued
    with pytest.raises(_lib.Yfv2Error):
        engine.batch_statistics_multi(dets, cnt, tg, [])
    compare_with_single_launches(engine, dets, cnt, tg, smm.COCO_THRESHOLDS)
