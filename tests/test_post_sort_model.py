"""Host model of the NMS launch's sort (bitonic_sort in yfv2_post.hip): the compare-exchange network the kernel runs (one
key per thread up to 1024 keys, more per thread beyond), on 64-bit keys conf_bits << 32 | ~row, against np.lexsort (conf
descending, ties by lower row)."""
import numpy as np
import pytest


def bitonic_sort(keys, threads=1024):
    """the kernel's network: next power of two np2, zero padding, descending; one key per thread when np2 <= 1024"""
    n = len(keys)
    np2 = 1
    while np2 < n:
        np2 <<= 1
    kpt = 1 if np2 <= threads else -(-np2 // threads)
    k = np.zeros(kpt * threads, np.uint64)
    k[:n] = keys
    i = np.arange(kpt * threads)
    kk = 2
    while kk <= np2:
        j = kk >> 1
        while j > 0:
            y = k[i ^ j]
            take_max = ((i & j) == 0) == ((i & kk) == 0)
            k = np.where(take_max == (k > y), k, y)
            j >>= 1
        kk <<= 1
    return k[:n]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2048, 3840])
def test_sort_model_matches_lexsort(n):
    rng = np.random.default_rng(n)
    conf = rng.uniform(0.3, 1.0, n).astype(np.float32)
    conf[rng.integers(0, n, n // 3)] = np.float32(0.5)   # ties: decided by the row
    rows = rng.permutation(4096)[:n].astype(np.uint64)
    keys = (conf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rows)
    got = bitonic_sort(keys)
    order = np.lexsort((rows, -conf.astype(np.float64)))
    np.testing.assert_array_equal(got, keys[order])
