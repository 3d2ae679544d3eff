"""Anchor k-means: the golden cases and the numpy model of the kernels' arithmetic (yolo_fastestv2_amd/csrc/yfv2_anchors.hip).

The model is the executable specification of the device results: the same four-case similarity, the same first-minimum
assignment and - what makes it bit-exact rather than merely close - the same summation tree over fixed chunks of 1024 points.
tests/test_anchors_host.py holds it against the reference's goldens, tests/test_gpu_anchors.py holds the device against it bit
for bit, tools/anchors_probe.py times it as the vectorised CPU baseline.
"""
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_anchors.npz")

CH = 1024      # YFV2_KM_CH: points per chunk
LANES = 256    # threads of a workgroup

# (N, k, seed): the sizes that cross a wave, a workgroup, a chunk boundary and a multi-chunk finalise, k = 1, and CH -+ 1
CASES = [(7, 3, 1), (255, 6, 2), (257, 6, 3), (4099, 6, 4), (20011, 6, 5), (20011, 10, 6), (4099, 1, 7), (1023, 6, 8), (1025, 6, 9)]


def make_x(seed, N):
    return np.round(np.clip(np.exp(np.random.RandomState(seed).normal(-2.2, 0.9, (N, 2))), 0.004, 1.0), 6)


def initial_indices(seed, N, k):
    random.seed(seed)
    return [random.randrange(N) for _ in range(k)]


def load_case(z, i):
    """(X, initial centroids, golden dict) of case i, X regenerated from the seed and checked against the stored probe"""
    g = {key[len("c%d_" % i):]: z[key] for key in z if key.startswith("c%d_" % i)}
    N, k, seed = int(g["N"]), int(g["k"]), int(g["seed"])
    X = make_x(seed, N)
    assert np.array_equal(X.ravel()[::997], g["x_probe"]), "the generated label sizes differ from the generating machine's"
    idx = initial_indices(seed, N, k)
    assert idx == [int(v) for v in g["init_idx"]]
    return X, X[idx].copy(), g


def write_label_tree(root, X, per_image=5):
    """a VOC-style tree: JPEGImages/*.jpg|*.png listed in train.txt, labels/*.txt rows 'class cx cy w h'; returns the train.txt path"""
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "labels"))
    names = []
    for n, start in enumerate(range(0, len(X), per_image)):
        ext = ".jpg" if n % 2 == 0 else ".png"
        names.append(os.path.join(root, "JPEGImages", "img%04d%s" % (n, ext)))
        with open(os.path.join(root, "labels", "img%04d.txt" % n), "w") as f:
            for w, h in X[start:start + per_image]:
                f.write("%d 0.5 0.5 %r %r\n" % (n % 3, float(w), float(h)))
    traintxt = os.path.join(root, "train.txt")
    with open(traintxt, "w") as f:
        f.write("\n".join(names) + "\n")
    return traintxt


def tree_sum(v):
    """The kernels' one summation tree over the last axis: pad with +0.0 to a multiple of 256; lane t adds v[t], v[t + 256], ...
    in ascending order; each wave folds its 64 lane values in halves (a[l] += a[l + 32], 16, 8, 4, 2, 1); the four wave values
    are added in ascending order."""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    rows = max(1, -(-n // LANES))
    if rows * LANES != n:
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (rows * LANES - n,))], axis=-1)
    v = v.reshape(v.shape[:-1] + (rows, LANES))
    lane = v[..., 0, :]
    for r in range(1, rows):
        lane = lane + v[..., r, :]
    a = lane.reshape(lane.shape[:-1] + (4, 64))
    half = 32
    while half >= 1:
        a = a[..., :half] + a[..., half:2 * half]
        half //= 2
    w = a[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def similarity(X, C):
    """(N, k) IoU of every label size with every centroid: four cases tested in the reference's order, each with its own formula"""
    w, h = X[:, 0:1], X[:, 1:2]
    cw, ch = C[None, :, 0], C[None, :, 1]
    with np.errstate(all="ignore"):
        inside = w * h / (cw * ch)
        tall = w * ch / (w * h + (cw - w) * ch)
        wide = cw * h / (w * h + cw * (ch - h))
        outside = (cw * ch) / (w * h)
    return np.where((cw >= w) & (ch >= h), inside, np.where((cw >= w) & (ch <= h), tall, np.where((cw <= w) & (ch >= h), wide, outside)))


def chunk_sums(values, nch):
    """values (..., N) -> (..., nch): the tree over each chunk of CH values"""
    N = values.shape[-1]
    pad = nch * CH - N
    if pad:
        values = np.concatenate([values, np.zeros(values.shape[:-1] + (pad,))], axis=-1)
    return tree_sum(values.reshape(values.shape[:-1] + (nch, CH)))


def kmeans(X, C0, max_iter=1000):
    """The device loop.  Returns dict(centroids, assign, avg_iou, iterations, converged, empty_cluster, updates) where updates[i]
    = the centroids after update i + 1."""
    X = np.asarray(X, np.float64)
    C = np.array(C0, np.float64)
    N, k = X.shape[0], C.shape[0]
    nch = -(-N // CH)
    prev = np.full(N, -1)
    updates = []
    for it in range(1, max_iter + 1):
        S = similarity(X, C)
        assign = np.argmin(1.0 - S, axis=1)
        avg_iou = tree_sum(chunk_sums(S.max(axis=1), nch)) / float(N)
        onehot = assign[None, :] == np.arange(k)[:, None]
        count = onehot.sum(axis=1)
        out = dict(centroids=C, assign=assign, avg_iou=avg_iou, iterations=it, converged=0, empty_cluster=-1, updates=updates)
        if (assign == prev).all():
            out["converged"] = 1
            return out
        if (count == 0).any():
            out["empty_cluster"] = int(np.argmax(count == 0))
            return out
        if it == max_iter:
            return out
        sw = tree_sum(chunk_sums(np.where(onehot, X[None, :, 0], 0.0), nch))
        sh = tree_sum(chunk_sums(np.where(onehot, X[None, :, 1], 0.0), nch))
        C = np.stack([sw / count.astype(np.float64), sh / count.astype(np.float64)], axis=1)
        updates.append(C)
        prev = assign
