"""Generates tests/golden/golden_anchors.npz from the REFERENCE's genanchors.py (run where a reference checkout exists:
``python tests/golden/make_golden_anchors.py /path/to/Yolo-FastestV2``).  make_golden.py is left alone.

Per case (N, k, seed) of tests/anchors_model.CASES the reference's own kmeans / avg_IOU / write_anchors_to_file run on
label sizes regenerated from the seed; X itself is not stored (a probe of it is).  The reference's script needs `np.float`,
which this numpy no longer has: it is set before the import.  Its prints are silenced; the iteration count is the number of
its "iter N:" lines.

Gap condition: for every point and pass the two smallest distances differ by at least 1e-9 (asserted here).  A different
summation order moves a centroid by a few 1e-15, so no assignment can legitimately differ and the tests exempt no point.
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import anchors_model as am  # noqa: E402

WIDTH = HEIGHT = 352


def load_reference(root):
    np.float = float  # genanchors.py:95
    spec = importlib.util.spec_from_file_location("ref_genanchors", os.path.join(root, "genanchors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv):
    if len(argv) < 2:
        raise SystemExit("usage: make_golden_anchors.py /path/to/Yolo-FastestV2")
    ref = load_reference(argv[1])
    ref_iou = ref.IOU
    gap = [np.inf]

    def watched_iou(x, centroids):
        s = ref_iou(x, centroids)
        if len(s) > 1:
            d = np.sort(1 - s)
            gap[0] = min(gap[0], d[1] - d[0])
        return s

    out = {"cases": np.array(am.CASES, np.int64), "width": np.int64(WIDTH), "height": np.int64(HEIGHT)}
    for i, (N, k, seed) in enumerate(am.CASES):
        X = am.make_x(seed, N)
        idx = am.initial_indices(seed, N, k)
        centroids = X[idx].copy()
        gap[0] = np.inf
        ref.IOU = watched_iou
        log = io.StringIO()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "anchors%d.txt" % k)
            with contextlib.redirect_stdout(log):
                ref.kmeans(X, centroids, 0.005, path, WIDTH, HEIGHT)
            with open(path, "rb") as f:
                file_bytes = f.read()
        min_gap = gap[0]   # (the avg_IOU walk inside write_anchors_to_file sees the last pass's distances again: same minimum)
        ref.IOU = ref_iou
        iterations = sum(1 for line in log.getvalue().splitlines() if line.startswith("iter "))
        with contextlib.redirect_stdout(io.StringIO()):
            avg_iou = ref.avg_IOU(X, centroids)
        assign = np.array([np.argmin(1 - ref.IOU(X[j], centroids)) for j in range(N)])   # the terminating pass's (centroids unchanged by it)
        assert np.isfinite(centroids).all() and len(np.unique(assign)) == k, "case %d: empty cluster - change the seed" % i
        assert k == 1 or min_gap >= 1e-9, "case %d: top-two gap %g below 1e-9 - change the seed" % (i, min_gap)
        p = "c%d_" % i
        out.update({p + "seed": np.int64(seed), p + "N": np.int64(N), p + "k": np.int64(k), p + "x_probe": X.ravel()[::997].copy(),
                    p + "init_idx": np.array(idx, np.int64), p + "centroids": centroids, p + "assign": assign.astype(np.uint8),
                    p + "iterations": np.int64(iterations), p + "avg_iou": np.float64(avg_iou),
                    p + "file": np.frombuffer(file_bytes, dtype="S1"), p + "min_gap": np.float64(min_gap)})
        print("case %d (N %d, k %d, seed %d): %d iterations, smallest gap %.3g, avg IoU %.6f" % (i, N, k, seed, iterations, min_gap, avg_iou))
    np.savez_compressed(os.path.join(HERE, "golden_anchors.npz"), **out)


if __name__ == "__main__":
    main(sys.argv)
