"""Host model (numpy fp32) of the conf / class rule of the row decode behind the fused decode + NMS launch and decode_kernel<true>
(yfv2_compact_row, yolo_fastestv2_amd/csrc/yfv2_post.hip), against the exact sweep it replaces.

The reference's rule (utils/utils.py:261,267): conf = max_j fl(fl(e_j / sum) * obj), class = the FIRST maximal j, with the
exponentials e_j = exp(x_j - max) (the largest is exactly 1) and sum = their fp32 sum.  The kernel's shortcut: when exactly one
exponential is >= 1 - 2^-20 and fl(fl(1 / sum) * obj) > 2^-100, conf = fl(fl(1 / sum) * obj) and class = that exponential's index;
otherwise it runs the exact sweep.  The sum is formed in the kernel's order: each of a cell's four lanes adds its slice of
ceil(nc / 4) classes in index order, then (s0 + s1) + (s2 + s3).  Inputs: the maximum exactly 1 and a second class at
1 - k 2^-24 (k = 1..40: inside, at and beyond the 2^-20 window), the rest random below; obj in every binade down to 2^-126;
1 .. 96 classes.  CPU only."""
import numpy as np
import pytest

F32 = np.float32
NEAR = F32(1.0 - 2.0 ** -20)
TINY = F32(2.0 ** -100)


def lane_sum(e):
    """(n, nc) exponentials -> (n,) fp32 sum in the kernel's 4-lane order"""
    nc = e.shape[1]
    per = (nc + 3) // 4
    s = np.zeros((e.shape[0], 4), F32)
    for p in range(4):
        for c in range(p * per, min(nc, (p + 1) * per)):
            s[:, p] = (s[:, p] + e[:, c]).astype(F32)
    return ((s[:, 0] + s[:, 1]).astype(F32) + (s[:, 2] + s[:, 3]).astype(F32)).astype(F32)


def exact_sweep(e, total, obj):
    prod = ((e / total[:, None]).astype(F32) * obj[:, None]).astype(F32)
    j = prod.argmax(1)                                                    # first maximal index
    return prod[np.arange(len(j)), j], j


def shortcut(e, total, obj):
    """-> (taken, conf, class) of the kernel's fast path"""
    near = e >= NEAR
    conf = ((F32(1) / total).astype(F32) * obj).astype(F32)
    taken = (near.sum(1) == 1) & (conf > TINY)
    return taken, conf, near.argmax(1)


@pytest.mark.parametrize("nc", list(range(1, 97)))
def test_shortcut_equals_exact_sweep(nc):
    rng = np.random.default_rng(nc)
    ks = np.arange(1, 41)
    binades = np.arange(0, 127)
    n = len(ks) * len(binades)
    e = rng.uniform(0.0, 1.0 - 2.0 ** -19, (n, nc)).astype(F32)
    e[rng.random((n, nc)) < 0.1] = F32(0)                                 # underflowed exponentials
    p = rng.integers(0, nc, n)
    q = (p + 1 + rng.integers(0, max(1, nc - 1), n)) % nc                 # the second class, before or after the maximum
    k = np.repeat(ks, len(binades))
    e[np.arange(n), q] = (1.0 - k * 2.0 ** -24).astype(F32)
    e[np.arange(n), p] = F32(1)
    obj = np.ldexp(rng.uniform(1.0, 2.0, n), -np.tile(binades, len(ks))).astype(F32)
    total = lane_sum(e)
    conf, j = exact_sweep(e, total, obj)
    taken, f_conf, f_j = shortcut(e, total, obj)
    assert np.array_equal(f_conf[taken].view(np.uint32), conf[taken].view(np.uint32))
    assert np.array_equal(f_j[taken], j[taken]), np.flatnonzero(taken & (f_j != j))[:5]
    if nc > 1:
        # the window: a second class within 2^-20 of the maximum never takes the shortcut; one beyond it does, while conf > 2^-100
        inside = e[np.arange(n), q] >= NEAR
        assert not taken[inside].any()
        assert taken[~inside & (f_conf > TINY)].all()
        assert (k[~inside] >= 17).all() and (k[inside] <= 16).all()
    assert taken.sum() > n // 3                                           # (the shortcut is the common case)


def test_denormal_products_tie_where_the_shortcut_is_not_taken():
    """why the 2^-100 guard: with obj near 2^-126 two distinct exponentials give the same product, and the first index wins"""
    e = np.asarray([[F32(1.0 - 40 * 2.0 ** -24), F32(1)]], F32)
    obj = np.asarray([F32(2.0 ** -140)], F32)
    total = lane_sum(e)
    conf, j = exact_sweep(e, total, obj)
    taken, _, f_j = shortcut(e, total, obj)
    assert j[0] == 0 and f_j[0] == 1 and not taken[0]
