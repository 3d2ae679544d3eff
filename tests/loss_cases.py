"""The shapes, batches, label counts and logit ranges the training loss (yfv2_loss) is pinned at beyond the 352x352 cases of
tests/golden/make_golden.py LOSS_CASES: ONE table, as data, read by the golden generator (make_golden.py loss_shapes), the CPU
test (tests/test_loss_shapes_host.py) and the GPU test (tests/test_gpu_loss_shapes.py).

A case is (classes, B, T, H, W, seed, flavour).  The network input is H x W, so the loss maps are H/16 x W/16 and H/32 x W/32;
the anchors are the COCO ones scaled per axis (w by W/352, h by H/352).  Inputs are rebuilt from the seed (numpy PCG64), never
stored.  Pure numpy / torch: importable without a device and without the native library."""
import collections
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import yfv2_oracle as oracle

Case = collections.namedtuple("Case", "classes B T H W seed flavour")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EDGE_SEED = 6         # the case whose labels carry centres on and past the right / lower edge (as LOSS_CASES' seed 6 does)
REG_SATURATION = 12.0  # beyond it the REFERENCE's autograd is NaN (at 30 the predicted width underflows against the centre in float64: atan(0/0))
OBJ_CLS_SATURATION = 60.0

CASES = (
    Case(80, 2, 12, 32, 32, 0, "plain"),          # 2x2 and 1x1 maps: no neighbour candidate on 1x1, every label of an image shares a cell
    Case(1, 1, 1, 32, 32, 29, "plain"),           # T = 1: both scales in one block of loss_match_kernel (seed 29: the one label matches on both); one class: no class term
    Case(2, 3, 3, 32, 64, 31, "plain"),           # T = 3 (same block for both scales; seed 31: matches on both); 2x4 and 1x2 maps: a 1-high map
    Case(3, 1, 200, 32, 64, 3, "plain"),          # crowded: tens of labels in one (image, anchor, cell) - the atomicAdd sums
    Case(80, 5, 40, 64, 32, 4, "saturated"),      # 4x2 and 2x1 maps: a 1-wide map
    Case(255, 2, 6, 64, 96, 5, "saturated"),      # small non-square map, the largest class count
    Case(2, 9, 60, 64, 96, EDGE_SEED, "plain"),   # centres on and past the right / lower edge, on a non-square map; B = 9
    Case(3, 3, 7, 352, 32, 7, "plain"),           # strip: 22x2 and 11x1; 15 * 7 % 128 != 0: a block straddles the two scales
    Case(80, 5, 50, 288, 384, 8, "plain"),        # the project's usual non-square size (first half of the handle-reuse test)
    Case(80, 2, 9, 288, 384, 9, "plain"),         # (second half: smaller batch, fewer labels; also the compute_loss drop-in's case)
    Case(2, 4, 90, 640, 384, 10, "saturated"),    # maps larger than 22x22: 40x24 and 20x12
    Case(80, 3, 30, 288, 384, 11, "bad_rows"),
    Case(3, 1, 5, 32, 32, 12, "bad_rows"),
    Case(80, 2, 0, 64, 32, 13, "plain"),          # no labels
    Case(255, 1, 16, 352, 32, 14, "saturated"),
    Case(1, 2, 20, 64, 96, 15, "bad_rows"),       # one class: the only valid class is 0, `classes` = 1 is out of range
)
CROWDED = 3            # index into CASES
REUSE = (8, 9)         # same H, W, classes: B = 5 then B = 2 with fewer labels on one handle
DROPIN = 9


def case_id(c):
    return "c%d_b%d_t%d_%dx%d_%s" % (c.classes, c.B, c.T, c.H, c.W, c.flavour)


def coco_anchors():
    return [float(a) for a in np.load(os.path.join(GOLDEN, "cfg_coco.npz"))["anchors"]]


def anchors_for(H, W):
    """the COCO anchors (352x352) scaled per axis to an H x W input: 12 floats, (w, h) pairs"""
    return [a * (W if i % 2 == 0 else H) / 352 for i, a in enumerate(coco_anchors())]


def map_shapes(c):
    return [(c.H // 16, c.W // 16), (c.H // 32, c.W // 32)]


def case_inputs(c):
    """-> (preds, targets, valid): the six fp32 NCHW logit maps, the (T', 6) fp32 label rows [image, class, cx, cy, w, h] and a
    bool mask of the rows that meet yfv2_loss's precondition (all of them unless the flavour is bad_rows, where T' = T + 4).
    Labels as make_golden.loss_case_inputs builds them - some at the image border, some at extreme sizes - and a quarter of
    the rows sized from a randomly chosen anchor times a factor in (0.55, 1.8), so that every anchor finds matches."""
    classes, B, T, H, W, seed, flavour = c
    rng = np.random.default_rng(2000 + seed)
    (h2, w2), (h3, w3) = map_shapes(c)
    shapes = [(B, 12, h2, w2), (B, 3, h2, w2), (B, classes, h2, w2), (B, 12, h3, w3), (B, 3, h3, w3), (B, classes, h3, w3)]
    preds = [(rng.standard_normal(sh) * 2).astype(np.float32) for sh in shapes]
    t = rng.random((T, 6)).astype(np.float32)
    if T:
        t[:, 0] = rng.integers(0, B, T)
        t[:, 1] = rng.integers(0, classes, T)
        t[:, 4:6] = t[:, 4:6] * 0.6 + 0.01
        edge = rng.random(T) < 0.25
        t[edge, 2] = np.where(rng.random(edge.sum()) < 0.5, 0.004, 0.997).astype(np.float32)
        t[rng.random(T) < 0.15, 4:6] = 0.9
        sized = np.flatnonzero(rng.random(T) < 0.25)
        anc = np.asarray(coco_anchors(), np.float64).reshape(6, 2) / 352.0       # normalised: the same at every input size
        t[sized, 4:6] = (anc[rng.integers(0, 6, len(sized))] * rng.uniform(0.55, 1.8, (len(sized), 2))).astype(np.float32)
        if seed == EDGE_SEED:
            t[0::3, 2] = 1.0
            t[1::4, 3] = 1.0
            t[2, 2], t[5, 3] = 1.003, 1.01
            t[:, 4:6] = np.minimum(t[:, 4:6], 0.3) + 0.05
    if flavour == "saturated":
        for k, p in enumerate(preds):
            mag = REG_SATURATION if k % 3 == 0 else OBJ_CLS_SATURATION
            hit = rng.random(p.shape) < 0.2
            p[hit] = np.where(rng.random(int(hit.sum())) < 0.5, -mag, mag).astype(np.float32)
    valid = np.ones(T, bool)
    if flavour == "bad_rows":
        # rows that WOULD match (sizes of anchors 1 and 4, centre of the image) but name no image / no class of the batch
        bad = np.zeros((4, 6), np.float32)
        bad[:, 2:4] = (0.45, 0.55)
        anc = np.asarray(coco_anchors(), np.float32).reshape(6, 2) / np.float32(352)
        bad[0::2, 4:6], bad[1::2, 4:6] = anc[1], anc[4]
        bad[:, 0] = (-1, B, 0, B - 1)
        bad[:, 1] = (0, classes - 1, -1, classes)
        pos = np.sort(rng.integers(0, T + 1, 4))                                  # interleaved with the valid rows
        t = np.insert(t, pos, bad, axis=0)
        valid = np.insert(valid, pos, False)
    return preds, np.ascontiguousarray(t, np.float32), valid


def swapped_axes(t):
    """the labels with the cx / cy columns exchanged (what an H / W mix-up in the cell arithmetic amounts to)"""
    s = t.copy()
    s[:, 2], s[:, 3] = t[:, 3], t[:, 2]
    return s


def oracle_loss(c, preds, t, dtype=torch.float32):
    """The CPU oracle on one case: (losses (4,) float64 array, the six gradients of the total as arrays of `dtype`).
    float32: oracle.compute_loss, the reference's arithmetic.  float64: the same expressions on float64 logits with
    build_target's (fp32, discrete) matching unchanged - the yardstick the rounding of both fp32 paths is measured against."""
    anchors = anchors_for(c.H, c.W)
    p = [torch.from_numpy(x.copy()).to(dtype).requires_grad_() for x in preds]
    tt = torch.from_numpy(t)
    if dtype == torch.float32:
        out = oracle.compute_loss(p, tt, anchors, c.classes, 3, c.W, c.H)
    else:
        out = _compute_loss64(p, tt, anchors, c.classes, c.W, c.H)
    out[3].backward()
    grads = [(a.grad if a.grad is not None else torch.zeros_like(a)).numpy() for a in p]
    return np.asarray([float(v.detach()) for v in out], np.float64), grads


def _compute_loss64(p, targets, anchors, classes, width, height):
    shapes = [(p[0].shape[2], p[0].shape[3]), (p[3].shape[2], p[3].shape[3])]
    tg = oracle.build_target(shapes, targets, anchors, 3, width, height)
    lbox, lobj, lcls = torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    for li in range(2):
        reg, obj, cls = p[3 * li], p[3 * li + 1], p[3 * li + 2]
        B, _, H, W = reg.shape
        b, a, gj, gi, tbox, anc, cl = tg[li]
        tobj = torch.zeros((B, 3, H, W), dtype=torch.float64)
        if len(b):
            ps = reg.reshape(B, 3, 4, H, W).permute(0, 1, 3, 4, 2)[b, a, gj, gi]
            pxy = ps[:, :2].sigmoid() * 2.0 - 0.5
            pwh = (ps[:, 2:4].sigmoid() * 2) ** 2 * anc
            lbox = lbox + (1.0 - oracle.ciou_xywh(torch.cat((pxy, pwh), 1), tbox.double())).mean()
            tobj[b, a, gj, gi] = 1.0
            if classes > 1:
                lcls = lcls + F.cross_entropy(cls.permute(0, 2, 3, 1)[b, gj, gi], cl) / classes
        lobj = lobj + F.binary_cross_entropy_with_logits(obj, tobj) * oracle.LOSS_BALANCE[li]
    lbox, lobj, lcls = lbox * 3.2, lobj * 64, lcls * 32
    return lbox, lobj, lcls, lbox + lobj + lcls


def golden_grads(z, ci, preds):
    """the six gradient maps of case ci out of golden_loss_shapes.npz (objectness dense, the others (index, value))"""
    out = []
    for k, p in enumerate(preds):
        if k % 3 == 1:
            out.append(z["grad%d_%d" % (ci, k)].reshape(p.shape))
        else:
            g = np.zeros(p.size, np.float32)
            g[z["grad%d_%d_idx" % (ci, k)]] = z["grad%d_%d_val" % (ci, k)]
            out.append(g.reshape(p.shape))
    return out


def match_census(c, t):
    """per scale: dict(nb, anchors = matches per anchor (3), candidates = matches per offset candidate (5),
    crowd = the most labels in one (image, anchor, cell)) - what test (b) of the host test counts, from oracle.build_target"""
    shapes = map_shapes(c)
    t = np.asarray(t, np.float32).reshape(-1, 6)
    tg = oracle.build_target(shapes, t, anchors_for(c.H, c.W), 3, c.W, c.H)
    out = []
    for li, ((b, a, gj, gi, tb, an, cl), (h, w)) in enumerate(zip(tg, shapes)):
        d = {"nb": int(len(b)), "anchors": [int((a == k).sum()) for k in range(3)], "candidates": [0] * 5, "crowd": 0}
        if len(b):
            key = ((b * 3 + a) * h + gj) * w + gi
            d["crowd"] = int(torch.bincount(key).max())
        out.append(d)
    if len(t):
        for k in range(5):
            for li, n in enumerate(_candidate_counts(c, t, k)):
                out[li]["candidates"][k] = n
    return out


def _candidate_counts(c, t, k):
    """matches of offset candidate k per scale: the conditions of oracle.build_target restated for counting only (build_target
    returns the candidates concatenated; the host test checks that these counts add up to its nb)"""
    res = []
    anc = np.asarray(anchors_for(c.H, c.W), np.float64).reshape(2, 3, 2)
    for li, (h, w) in enumerate(map_shapes(c)):
        stride = c.W / w
        g = t[:, 2:6] * np.asarray([w, h, w, h], np.float32)
        r = g[None, :, 2:4].astype(np.float64) / (anc[li] / stride)[:, None]
        ok = np.maximum(r, 1.0 / r).max(2) < 2
        gxy = g[:, :2]
        inv = np.asarray([w, h], np.float32) - gxy
        want = [np.ones(len(t), bool), (gxy[:, 0] % 1.0 < 0.5) & (gxy[:, 0] > 1.0), (gxy[:, 1] % 1.0 < 0.5) & (gxy[:, 1] > 1.0),
                (inv[:, 0] % 1.0 < 0.5) & (inv[:, 0] > 1.0), (inv[:, 1] % 1.0 < 0.5) & (inv[:, 1] > 1.0)][k]
        res.append(int((ok & want[None]).sum()))
    return res
