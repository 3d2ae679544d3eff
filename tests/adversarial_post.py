"""Deterministic builders of crafted post-processing inputs: logit tuples for decode / the fused decode + NMS launch, and decoded
(B, rows, 5 + classes) tensors for non_max_suppression.  numpy default_rng with fixed seeds, so that tests and
tests/golden/make_golden.py (`adversarial`) rebuild the same inputs without storing them.

Logit cases aim at the conf / class shortcuts of the row decode: exact and 2^-20-near ties between classes, saturated and
denormal class probabilities, objectness down to conf < 2^-100, per-cell anchor patterns around the threshold, non-finite
logits.  Decoded cases aim at non_max_suppression's edges: NaN class scores, negative and signed-zero conf, thresholds met
exactly, IoU exactly at the threshold, zero-area boxes, a 64-deep suppression chain, ties across the 300-detection cut,
boxes wider than the 4096 class offset.
"""
import numpy as np

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]   # data/coco.data

# thresholds the fixture and the NMS tests run at (conf in fp32, iou in double, as the reference compares them)
CONF_THRES = (0.3, 0.01, 0.0, -1.0)
IOU_THRES = (0.4, 0.5, 0.0, -0.1, 1.0)
CLASS_FILTER = (None, (0, 1, 3, 5))
# decoded-tensor configurations: (rows, classes) = 352 x 352 and 512 x 512 inputs, 80 and 255 classes
DECODED_CONFIGS = ((1815, 80), (3840, 80), (1815, 255), (3840, 255))

F32 = np.float32


def rows_of(h, w):
    return 3 * ((h // 16) * (w // 16) + (h // 32) * (w // 32))


# ---------------------------------------------------------------------------------------------------------------------------
# decoded rows (cx, cy, w, h, obj, cls_0 .. cls_{nc-1})
# ---------------------------------------------------------------------------------------------------------------------------
def _blank(rows, nc):
    """rows that pass no threshold used here (obj -2 < every conf_thres), each with its own box"""
    d = np.zeros((rows, 5 + nc), F32)
    i = np.arange(rows)
    d[:, 0] = 20 + (i % 40) * 9
    d[:, 1] = 20 + (i // 40 % 40) * 9
    d[:, 2:4] = 6
    d[:, 4] = -2
    d[:, 5:] = 0.01
    return d


def _put(d, r, box, obj, cls):
    """row r: xyxy box -> cx, cy, w, h (exact for the small integers and halves used here), objectness, class scores"""
    x1, y1, x2, y2 = box
    d[r, 0:4] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
    d[r, 4] = obj
    d[r, 5:] = cls


def _nan_and_signs(rows, nc, rng):
    d = _blank(rows, nc)
    r = iter(rng.permutation(rows)[:80].tolist())
    lo = np.full(nc, 0.05, F32)
    # the issue's reproduction: obj 0.9, class 0 NaN, class 1 0.8, next to an ordinary candidate
    c = lo.copy(); c[0] = np.nan; c[1 % nc] = 0.8
    _put(d, next(r), (10, 10, 50, 50), 0.9, c)
    c = lo.copy(); c[2 % nc] = 0.7
    _put(d, next(r), (12, 12, 52, 52), 0.9, c)
    # NaN in a late class, in two classes (different 16-lane slots), NaN after the maximum, NaN at the last class
    for j, k in ((37 % nc, 5 % nc), (17 % nc, 33 % nc), (nc - 1, 3 % nc)):
        c = lo.copy(); c[j] = np.nan; c[k] = 0.9 if k != j else np.nan
        _put(d, next(r), (100, 100, 140, 150), 0.8, c)
    c = lo.copy(); c[4 % nc] = 0.95; c[nc - 1] = np.nan
    _put(d, next(r), (200, 100, 240, 150), 0.8, c)
    # obj = +inf: a zero class score makes a NaN product (dropped); all scores positive: conf = +inf
    c = lo.copy(); c[6 % nc] = 0.0
    _put(d, next(r), (300, 10, 340, 40), np.inf, c)
    _put(d, next(r), (300, 50, 340, 90), np.inf, lo + 0.01)
    # obj NaN, obj -inf, all class scores -inf
    _put(d, next(r), (10, 200, 60, 260), np.nan, lo + 0.5)
    _put(d, next(r), (70, 200, 120, 260), -np.inf, lo + 0.5)
    _put(d, next(r), (130, 200, 180, 260), 0.9, np.full(nc, -np.inf, F32))
    # negative conf: negative obj with positive scores, positive obj with negative scores (pass conf_thres = -1 only)
    c = lo.copy(); c[1 % nc] = 0.5
    _put(d, next(r), (10, 300, 40, 330), -0.5, c)
    c = np.full(nc, -0.4, F32); c[2 % nc] = -0.1
    _put(d, next(r), (12, 302, 42, 332), 0.6, c)
    c = np.full(nc, -0.9, F32)
    _put(d, next(r), (14, 304, 44, 334), 0.95, c)
    # conf -0.0 and +0.0 (obj of either sign times a zero score), the -0.0 row both before and after the +0.0 row, same box
    # and class (the one kept first is the lower row: the reference sorts by value, stably)
    z = np.full(nc, -1.0, F32); z[0] = 0.0
    a, b = sorted((next(r), next(r)))
    _put(d, a, (200, 300, 260, 340), -0.5, z)
    _put(d, b, (200, 300, 260, 340), 0.5, z)
    a, b = sorted((next(r), next(r)))
    _put(d, a, (270, 300, 330, 340), 0.5, z)
    _put(d, b, (270, 300, 330, 340), -0.5, z)
    # +0.0 and -0.0 class scores tied as the maximum: the first index wins, its sign bit is the row's conf
    z = np.full(nc, -1.0, F32); z[3 % nc] = -0.0; z[min(nc - 1, 9)] = 0.0
    _put(d, next(r), (150, 300, 190, 340), 0.7, z)
    # NaN box of a candidate (a NaN IoU suppresses nothing), inf-free
    c = lo.copy(); c[0] = 0.99
    _put(d, next(r), (10, 10, 50, 50), 0.99, c)
    rr = next(r)
    _put(d, rr, (10, 10, 50, 50), 0.98, c)
    d[rr, 0] = np.nan
    return d


def _thresholds(rows, nc, rng):
    d = _blank(rows, nc)
    r = iter(rng.permutation(rows)[:120].tolist())
    one = np.zeros(nc, F32); one[0] = 1.0
    x = 10.0
    # obj exactly fp32(conf_thres) (dropped by obj > conf_thres), one ulp above, conf exactly fp32(conf_thres) with obj above it
    for ct in (0.3, 0.01):
        t = F32(ct)
        for obj in (t, np.nextafter(t, F32(1)), np.nextafter(t, F32(0))):
            _put(d, next(r), (x, 10, x + 8, 18), obj, one); x += 10
        half = np.zeros(nc, F32); half[1 % nc] = 0.5
        _put(d, next(r), (x, 10, x + 8, 18), t * F32(2), half); x += 10                       # conf = fl(0.5 * 2 t) = t
        _put(d, next(r), (x, 10, x + 8, 18), np.nextafter(t * F32(2), F32(1)), half); x += 10  # conf one ulp above t
    # obj 0.0 / -0.0 / denormal (conf_thres 0.0 and -1.0)
    for obj in (F32(0.0), F32(-0.0), F32(1e-45), F32(-1e-45), F32(2.0 ** -130)):
        _put(d, next(r), (x, 10, x + 8, 18), obj, one); x += 10
    # IoU exactly fp32(iou_thres): [0,0,5,1] vs [0,0,2,1] is 0.4f (> 0.4 in double: suppressed); [0,0,2,1] vs [0,0,1,1] is 0.5
    # (not > 0.5: kept); identical boxes: IoU 1 (not > 1.0); touching boxes: IoU 0 (not > 0.0)
    conf = iter(np.linspace(0.95, 0.6, 40).astype(F32).tolist())
    for boxes in (((0, 40, 5, 41), (0, 40, 2, 41)), ((10, 40, 12, 41), (10, 40, 11, 41)), ((20, 40, 30, 50), (20, 40, 30, 50)),
                  ((40, 40, 50, 50), (50, 40, 60, 50)), ((70, 40, 80, 50), (79, 40, 89, 50))):
        for bx in boxes:
            _put(d, next(r), tuple(v + 100 for v in bx), next(conf), one)
    # zero-area boxes: two identical (union 0, IoU NaN), one inside an ordinary box, one of zero width only
    for bx in ((300, 300, 300, 300), (300, 300, 300, 300), (310, 310, 310, 310), (305, 305, 330, 330), (320, 300, 320, 340)):
        _put(d, next(r), bx, next(conf), one)
    # equal conf, overlapping boxes: the lower row is kept
    rs = sorted(next(r) for _ in range(4))
    for k, rr in enumerate(rs):
        _put(d, rr, (200 + k, 200, 240 + k, 240), 0.8, one)
    return d


def _chain(rows, nc, rng):
    """a 64-deep suppression chain inside one 64-candidate chunk (box j overlaps j - 1 by IoU 7/13, j - 2 by 4/16), a 70-deep one
    across a chunk boundary, in descending conf; conf 0.9 .. : the chunks start at the first candidate"""
    d = _blank(rows, nc)
    r = rng.permutation(rows)[:134]
    one = np.zeros(nc, F32); one[2 % nc] = 1.0
    confs = (F32(0.95) - np.arange(134, dtype=F32) * F32(0.001)).astype(F32)
    for j in range(64):
        _put(d, r[j], (10 + 3 * j, 10, 20 + 3 * j, 20), confs[j], one)
    for j in range(70):
        _put(d, r[64 + j], (10 + 3 * j, 100, 20 + 3 * j, 110), confs[64 + j], one)
    return d


def _tie_cut(rows, nc, rng):
    """400 disjoint candidates, 340 of them with one and the same conf: the 300 kept are the higher confs, then the lowest rows"""
    d = _blank(rows, nc)
    r = rng.permutation(rows)[:400]
    for k, rr in enumerate(r):
        c = np.zeros(nc, F32); c[k % min(nc, 8)] = 1.0
        x, y = 10 + (k % 20) * 12, 10 + (k // 20) * 12
        _put(d, rr, (x, y, x + 10, y + 10), F32(0.9) if k % 7 == 0 else F32(0.5), c)
    return d


def _wide_classes(rows, nc, rng):
    """boxes wider than the 4096 class offset reach into the next classes' range; the last class's offset"""
    d = _blank(rows, nc)
    r = iter(rng.permutation(rows)[:40].tolist())
    confs = iter(np.linspace(0.9, 0.5, 40).astype(F32).tolist())
    for cls, box in ((0, (0, 0, 9000, 100)), (1, (-4000, 0, 5000, 100)), (2, (-8000, 0, 1000, 100)), (1, (10, 10, 60, 60)),
                     (nc - 1, (0, 0, 9000, 100)), (nc - 1, (10, 10, 60, 60)), (nc - 2, (4000, 0, 13000, 100)), (nc - 1, (12, 12, 62, 62))):
        c = np.zeros(nc, F32); c[cls] = 1.0
        _put(d, next(r), box, next(confs), c)
    return d


def _random_rows(rows, nc, rng):
    """160 rows that are candidates at conf_thres -1 (obj in (-0.5, 1)), scores of both signs, a NaN score in one row of five,
    clustered boxes"""
    d = _blank(rows, nc)
    n = 160
    r = rng.permutation(rows)[:n]
    k = 12
    cx, cy = rng.uniform(20, 330, k), rng.uniform(20, 330, k)
    which = rng.integers(0, k, n)
    d[r, 0] = (cx[which] + rng.normal(0, 8, n)).astype(F32)
    d[r, 1] = (cy[which] + rng.normal(0, 8, n)).astype(F32)
    d[r, 2:4] = rng.uniform(5, 80, (n, 2)).astype(F32)
    d[r, 4] = rng.uniform(-0.5, 1.0, n).astype(F32)
    sc = rng.uniform(-0.2, 1.0, (n, nc)).astype(F32)
    sc[:, 6:] = np.minimum(sc[:, 6:], 0.3)        # a few dominant classes, so that the class filter keeps some rows
    bad = np.flatnonzero(rng.random(n) < 0.2)
    sc[bad, rng.integers(0, nc, bad.size)] = np.nan
    d[r, 5:] = sc
    return d


DECODED_CASES = (("nan_and_signs", _nan_and_signs), ("thresholds", _thresholds), ("chain", _chain), ("tie_cut", _tie_cut),
                 ("wide_classes", _wide_classes), ("random_rows", _random_rows))


def decoded_batch(rows, nc, seed=0):
    """(len(DECODED_CASES), rows, 5 + nc) fp32: one image per crafted case"""
    out = []
    for k, (_, fn) in enumerate(DECODED_CASES):
        out.append(fn(rows, nc, np.random.default_rng([seed, rows, nc, k])))
    return np.stack(out).astype(F32)


def same_bits(x, y):
    """bit-equal fp32 arrays, any NaN equal to any NaN (NaN payload and sign are specified by neither side)"""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    if x.shape != y.shape:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    return bool(np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint32), y[~ny].view(np.uint32)))


def golden_result(z, c, a, i, f, b):
    """(rows, idx) golden_post_adversarial.npz holds for config c, conf_thres a, iou_thres i, class filter f, image b"""
    k = int(z["result"][c, a, i, f, b])
    off = np.concatenate(([0], np.cumsum(z["nms_count"])))
    return z["nms_rows"][off[k]:off[k + 1]], z["nms_idx"][off[k]:off[k + 1]]


def probe(a):
    """input checksum: a strided sample of the bits plus a 64-bit sum of all words (NaN payloads included)"""
    u = np.ascontiguousarray(a).view(np.uint32).reshape(-1)
    return np.concatenate((u[::9973], [np.uint32(u.astype(np.uint64).sum() & 0xFFFFFFFF)])).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# logits (reg (B,12,h,w), obj (B,3,h,w), cls (B,nc,h,w) at stride 16, then stride 32)
# ---------------------------------------------------------------------------------------------------------------------------
LOGIT_CASES = ("random_sigma8", "equal_classes", "exact_ties", "near_ties", "saturated", "tiny_obj", "anchor_patterns", "nonfinite")
NONFINITE_CASE = "nonfinite"


def _maps(nc, h, w):
    return [(12, h // 16, w // 16), (3, h // 16, w // 16), (nc, h // 16, w // 16), (12, h // 32, w // 32), (3, h // 32, w // 32),
            (nc, h // 32, w // 32)]


def _cells(c):
    """class map (nc, fh, fw) -> (cells, nc) view on a copy; put back with _uncells"""
    return c.reshape(c.shape[0], -1).T.copy()


def _uncells(v, shape):
    return np.ascontiguousarray(v.T.reshape(shape)).astype(F32)


def logit_image(case, nc, h, w, rng):
    """the six logit maps of ONE image of a crafted case (fp32)"""
    m = [rng.normal(0, 8, s).astype(F32) for s in _maps(nc, h, w)]
    if case == "random_sigma8":
        return m
    per = (nc + 3) // 4                                   # classes per lane of the row decode's 4-lane softmax
    for sc in (0, 1):
        cls, obj = m[3 * sc + 2], m[3 * sc + 1]
        v = _cells(cls)
        n = v.shape[0]
        top = rng.normal(0, 4, n).astype(F32)
        if case == "equal_classes":
            v[:] = top[:, None]
        elif case == "exact_ties":
            v = (top[:, None] - 12 - np.abs(v)).astype(F32)   # the two tied classes hold nearly all the probability
            a = rng.integers(0, nc, n)
            same = (a // per) * per + (a % per + 1 + rng.integers(0, max(1, per - 1), n)) % max(1, per)   # same 4-lane slice
            other = (a + per * rng.integers(1, 4, n)) % nc                                                # another slice
            b = np.where(np.arange(n) % 2 == 0, np.minimum(same, nc - 1), other)
            v[np.arange(n), a] = top
            v[np.arange(n), b] = top
        elif case == "near_ties":
            # the maximum at 0 (at 1.0 for the 1-ulp kind) and a second class 1 ulp below it, exp(d) just inside, just outside
            # and exactly at the 1 - 2^-20 bound of the row decode's near-maximum test, or 17 * 2^-24 below (outside it)
            v = (F32(-12) - np.abs(v)).astype(F32)
            a = rng.integers(0, nc, n)
            b = (a + 1 + rng.integers(0, max(1, nc - 1), n)) % nc
            kind = np.arange(n) % 5
            d = np.select([kind == 1, kind == 2, kind == 3], [-(2.0 ** -20 - 2.0 ** -25), -(2.0 ** -20 + 2.0 ** -24), -(2.0 ** -20)],
                          -17 * 2.0 ** -24)
            base = np.where(kind == 0, F32(1), F32(0)).astype(F32)
            v[np.arange(n), a] = base
            v[np.arange(n), b] = np.where(kind == 0, np.nextafter(base, F32(0)), base + d).astype(F32)
        elif case == "saturated":
            v[:] = F32(-80)
            a = rng.integers(0, nc, n)
            v[np.arange(n), a] = F32(80)
            # a few classes 87 .. 104 below the maximum: denormal probabilities and ones that underflow to 0
            for k, dd in enumerate((88, 95, 103, 104, 149)):
                j = (a + 1 + k) % nc
                v[np.arange(n), j] = np.where(j != a, F32(80 - dd), F32(80))
        elif case == "tiny_obj":
            o = _cells(obj)
            o[:] = rng.uniform(-110, -60, o.shape).astype(F32)   # sigmoid 1e-48 .. 1e-26: conf below 2^-100, denormal, 0
            m[3 * sc + 1] = _uncells(o, obj.shape)
        elif case == "anchor_patterns":
            o = _cells(obj)
            pat = (np.arange(o.shape[0]) * 5 + rng.integers(0, 8)) % 8  # 0, 1, 2 or 3 anchors above 0.3, varying inside a wave
            o[:] = np.where((pat[:, None] >> np.arange(3)[None, :]) & 1, F32(3.0), F32(-3.0)) + rng.normal(0, 0.2, o.shape).astype(F32)
            m[3 * sc + 1] = _uncells(o, obj.shape)
        elif case == "nonfinite":
            pick = rng.random(v.shape) < 0.01
            v[pick] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], F32), int(pick.sum()))
            o = _cells(obj)
            po = rng.random(o.shape) < 0.03
            o[po] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], F32), int(po.sum()))
            m[3 * sc + 1] = _uncells(o, obj.shape)
            reg = m[3 * sc]
            pr = rng.random(reg.shape) < 0.01
            reg[pr] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], F32), int(pr.sum()))
        else:
            raise ValueError(case)
        m[3 * sc + 2] = _uncells(v, cls.shape)
    return m


def logit_batch(case, nc, h, w, B=2, seed=0):
    """B images of one crafted case: six fp32 arrays (B, C, fh, fw) in detector.py:47's order"""
    rng = np.random.default_rng([seed, LOGIT_CASES.index(case), nc, h, w])
    imgs = [logit_image(case, nc, h, w, rng) for _ in range(B)]
    return [np.ascontiguousarray(np.stack([im[k] for im in imgs])).astype(F32) for k in range(6)]
