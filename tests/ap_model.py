"""Average precision per class: the numpy model of the device's arithmetic (yolo_fastestv2_amd/csrc/yfv2_ap.hip).

The model is the executable specification of ``yfv2_ap_per_class``: the stable rank (confidence descending, equal confidences -
+0 and -0 are equal - by ascending input index), the per-class curve exactly as the kernel forms it (each term a difference of
two quotients times the envelope) and - what makes it bit-exact rather than merely close - the same summation tree: chunks of
CH ranked positions of a class, ``anchors_model.tree_sum`` over each chunk, the chunk sums added in ascending order.
tests/test_ap_host.py holds it against the reference's goldens, tests/test_gpu_ap.py holds the device against it bit for bit.
"""
import os

import numpy as np

from anchors_model import tree_sum

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_ap.npz")

CH = 1024          # YFV2_AP_CH: terms per chunk of the AP sum (part of the result's definition)
SORT_TILE = 2048   # YFV2_AP_TILE: detections per workgroup of a sort pass (changes no bit; the tests cross it)
MAX_CLASS = 254    # classes are 0..254; bucket 255 holds the predictions of no target class


def load_case(z, i):
    """(tp float64, conf float32, pred_cls float32, labels float64, ref 4-tuple) of golden case i"""
    return z["tp%d" % i].astype(np.float64), z["conf%d" % i], z["cls%d" % i], z["labels%d" % i], z["ref%d" % i]


def rank(conf):
    """np.argsort(-conf, kind="stable"): numpy's comparison already holds +0 and -0 equal and orders denormals"""
    return np.argsort(-np.asarray(conf, np.float32), kind="stable")


def chunked_sum(terms):
    """the AP sum: tree_sum over each chunk of CH terms (the last one padded with +0.0), chunk sums added in ascending order"""
    n = len(terms)
    nch = max(1, -(-n // CH))
    padded = np.zeros(nch * CH)
    padded[:n] = terms
    sums = tree_sum(padded.reshape(nch, CH))
    total = sums[0]
    for s in sums[1:]:
        total = total + s
    return total


def ap_per_class(tp, conf, pred_cls, target_cls):
    """dict(n_gt, n_pred int64 [256]; p, r, ap float64 [256]; present; bad_input; means = the reference's last two lines (np.mean);
    means_seq = the four means added class after class, as the library's yfv2_ap_result holds them)"""
    tp = np.asarray(tp) != 0
    conf = np.asarray(conf, np.float32)
    pred_cls = np.asarray(pred_cls, np.float32)
    target_cls = np.asarray(target_cls, np.float32).reshape(-1)
    out = {"n_gt": np.zeros(256, np.int64), "n_pred": np.zeros(256, np.int64), "p": np.zeros(256), "r": np.zeros(256), "ap": np.zeros(256)}
    ok = (target_cls >= 0) & (target_cls <= MAX_CLASS) & (np.floor(target_cls) == target_cls)
    out["bad_input"] = int((~ok).any() or not np.isfinite(conf).all())
    out["n_gt"][:MAX_CLASS + 1] = np.bincount(target_cls[ok].astype(np.int64), minlength=MAX_CLASS + 1)
    order = rank(conf)
    tp_r, cls_r = tp[order], pred_cls[order]
    for c in np.flatnonzero(out["n_gt"]):
        hits = tp_r[cls_r == np.float32(c)]
        n_p, n_gt = len(hits), int(out["n_gt"][c])
        out["n_pred"][c] = n_p
        if n_p == 0:
            continue
        tpc = np.cumsum(hits.astype(np.int64))
        den = np.float64(n_gt) + 1e-16
        prec = tpc.astype(np.float64) / np.arange(1, n_p + 1).astype(np.float64)
        rec = tpc.astype(np.float64) / den
        rec_before = (tpc - 1).astype(np.float64) / den          # where tp = 1: the recall of the detection before (0 at the first)
        env = np.maximum.accumulate(prec[::-1])[::-1]
        terms = np.where(hits, (rec - rec_before) * env, 0.0)
        out["p"][c], out["r"][c], out["ap"][c] = prec[-1], rec[-1], chunked_sum(terms)
    present = np.flatnonzero(out["n_gt"])
    out["present"] = present
    p, r, ap = out["p"][present], out["r"][present], out["ap"][present]
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f1 = 2 * p * r / (p + r + 1e-16)
            out["means"] = (np.mean(p), np.mean(r), np.mean(ap), np.mean(f1))
            seq = [np.float64(0.0)] * 4
            for k in range(len(present)):
                seq = [seq[0] + p[k], seq[1] + r[k], seq[2] + ap[k], seq[3] + f1[k]]
            out["means_seq"] = tuple(s / np.float64(len(present)) for s in seq)
    return out


def sum_bound(tp, pred_cls, target_cls):
    """(m + C) * 2**-52: the worst-case relative gap between two summation orders of m non-negative terms followed by a C-term
    mean; m = the largest per-class true-positive count, C = the number of present classes"""
    tp = np.asarray(tp) != 0
    pred_cls = np.asarray(pred_cls)
    present = np.unique(np.asarray(target_cls))
    m = max([int(tp[pred_cls == c].sum()) for c in present] + [0])
    return (m + len(present)) * 2.0 ** -52
