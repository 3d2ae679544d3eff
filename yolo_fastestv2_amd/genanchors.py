"""genanchors.py of the reference on the MI355X: the six anchor pairs of a label set, the first step a user takes on their own data.

    kmeans(X, centroids, eps, anchor_file, width_in_cfg_file, height_in_cfg_file)   genanchors.py:67   (the loop runs on the device)
    write_anchors_to_file(centroids, X, anchor_file, width, height)                 genanchors.py:42   (byte for byte the same file)
    read_label_dims(traintxt)                                                       genanchors.py:124-147
    main(argv) / python -m yolo_fastestv2_amd.genanchors                            genanchors.py:104

The reference evaluates N k IoUs per pass in interpreted Python (and needs ``np.float``, which numpy dropped); here a pass is
two kernel launches (include/yfv2.h yfv2_anchor_kmeans).  There is no CPU path: k-means needs the built library and an MI355X.
"""
import argparse
import os
import random
import sys
import warnings

import numpy as np

MODEL_CLUSTERS = 6   # anchor_num 3 x 2 scales: what yfv2_set_anchors, handel_preds and the loss consume


def _sorted_scaled(centroids, width, height):
    anchors = np.array(centroids, dtype=np.float64, copy=True)
    anchors[:, 0] *= width
    anchors[:, 1] *= height
    return anchors[np.argsort(anchors[:, 0])]


def _host_avg_iou(X, centroids):
    """avg_IOU (genanchors.py:34-40) for callers that hold no k-means result: four-case IoU, running sum in point order"""
    w, h = X[:, 0:1], X[:, 1:2]
    cw, ch = centroids[None, :, 0], centroids[None, :, 1]
    with np.errstate(all="ignore"):
        s = np.where((cw >= w) & (ch >= h), w * h / (cw * ch),
                     np.where((cw >= w) & (ch <= h), w * ch / (w * h + (cw - w) * ch),
                              np.where((cw <= w) & (ch >= h), cw * h / (w * h + cw * (ch - h)), (cw * ch) / (w * h))))
    return float(np.cumsum(s.max(axis=1))[-1] / X.shape[0])


def write_anchors_to_file(centroids, X, anchor_file, width_in_cfg_file, height_in_cfg_file, avg_iou=None):
    """The reference's anchor file: the centroids times the configured size, sorted by width, '%0.2f,%0.2f' pairs joined by
    ', ', a newline, then '%f' of the average IoU.  ``avg_iou``: the k-means call's own result (kmeans passes it); None
    recomputes it on the host from X."""
    centroids = np.asarray(centroids, np.float64)
    if avg_iou is None:
        avg_iou = _host_avg_iou(np.asarray(X, np.float64), centroids)
    anchors = _sorted_scaled(centroids, width_in_cfg_file, height_in_cfg_file)
    with open(anchor_file, "w") as f:
        for a in anchors[:-1]:
            f.write("%0.2f,%0.2f, " % (a[0], a[1]))
        f.write("%0.2f,%0.2f\n" % (anchors[-1, 0], anchors[-1, 1]))
        f.write("%f\n" % float(avg_iou))


def anchors_for_cfg(centroids, width, height):
    """The flat anchor list (12 floats for 6 clusters) as the anchor file holds it - scaled, sorted by width, rounded to two
    decimals - ready for cfg["anchors"], Engine.set_anchors and load_datafile-style dicts."""
    return [float("%0.2f" % v) for v in _sorted_scaled(centroids, width, height).ravel()]


def read_label_dims(traintxt):
    """(N, 2) float64 w, h of every label of every image listed in ``traintxt``: the label file of an image path is the path with
    'JPEGImages' -> 'labels' and '.jpg' / '.png' -> '.txt'; w and h are the fields after the third blank of a line."""
    dims = []
    with open(traintxt) as f:
        lines = [line.rstrip("\n") for line in f.readlines()]
    for line in lines:
        line = line.replace("JPEGImages", "labels").replace(".jpg", ".txt").replace(".png", ".txt")
        with open(line) as f2:
            for row in f2.readlines():
                w, h = row.rstrip("\n").split(" ")[3:]
                dims.append((float(w), float(h)))
    return np.array(dims, dtype=np.float64).reshape(-1, 2)


def kmeans(X, centroids, eps, anchor_file, width_in_cfg_file, height_in_cfg_file, device=None, max_iter=1000):
    """The reference's signature plus ``device`` and ``max_iter``.  X (N, 2) and centroids (k, 2) are numpy float64; centroids
    is overwritten with the result, as the reference does, and the anchor file is written.  Returns (centroids, assignments,
    avg_iou, iterations).  ``eps`` is unused, as in the reference.  Raises ValueError on a label size that is not a finite
    number > 0 and on a cluster that received no point (naming it; the reference would go on with NaN centroids), RuntimeError
    if the assignments have not repeated within max_iter passes."""
    import torch

    from .engine import get_engine
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != 2 or centroids.shape[1:] != (2,):
        raise ValueError("X must be (N, 2) and centroids (k, 2)")
    eng = get_engine(device if device is not None else "cuda", 352, 352)
    cent, assign, avg, info = eng.anchor_kmeans(torch.from_numpy(X).to(eng.device), torch.from_numpy(np.ascontiguousarray(centroids, dtype=np.float64)).to(eng.device),
                                                max_iter=max_iter)
    if info["bad_input"]:
        raise ValueError("anchor k-means: a label width or height is not a finite number > 0")
    if info["empty_cluster"] >= 0:
        raise ValueError("anchor k-means: cluster %d received no point in pass %d (duplicate initial centroids?); draw other initial centroids"
                         % (info["empty_cluster"], info["iterations"]))
    if not info["converged"]:
        raise RuntimeError("anchor k-means: assignments still changing after max_iter = %d passes" % max_iter)
    centroids[...] = cent.cpu().numpy()
    avg_iou = float(avg.cpu())
    write_anchors_to_file(centroids, X, anchor_file, width_in_cfg_file, height_in_cfg_file, avg_iou=avg_iou)
    return centroids, assign.cpu().numpy(), avg_iou, info["iterations"]


def main(argv):
    """argv as sys.argv (program name first); the reference's flags."""
    parser = argparse.ArgumentParser(prog="yolo_fastestv2_amd.genanchors")
    parser.add_argument("--traintxt", default="", help="path to traintxt")
    parser.add_argument("--output_dir", default="./", type=str, help="Output anchor directory")
    parser.add_argument("--num_clusters", default=6, type=int, help="number of clusters (0: one run for each of 1..10)")
    parser.add_argument("--input_width", default=352, type=int, help="model input width")
    parser.add_argument("--input_height", default=352, type=int, help="model input height")
    args = parser.parse_args(argv[1:])
    if not os.path.exists(args.output_dir):
        os.mkdir(args.output_dir)
    dims = read_label_dims(args.traintxt)
    results = []
    for k in (range(1, 11) if args.num_clusters == 0 else [args.num_clusters]):
        if k != MODEL_CLUSTERS:
            warnings.warn("this model takes %d anchor pairs (anchor_num 3 x 2 scales); anchors%d.txt is not usable as its cfg anchors" % (MODEL_CLUSTERS, k))
        anchor_file = os.path.join(args.output_dir, "anchors%d.txt" % k)
        indices = [random.randrange(dims.shape[0]) for _ in range(k)]   # the reference's draw, in its order
        centroids = dims[indices]
        _, _, avg_iou, iterations = kmeans(dims, centroids, 0.005, anchor_file, args.input_width, args.input_height)
        print("%s: %d passes, avg IoU %f, anchors %s" % (anchor_file, iterations, avg_iou, anchors_for_cfg(centroids, args.input_width, args.input_height)))
        results.append((k, centroids, avg_iou, iterations))
    return results


if __name__ == "__main__":
    main(sys.argv)
