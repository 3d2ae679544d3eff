"""A numpy statement of the rule yfv2_batch_statistics_multi implements (csrc/yfv2_post.hip stats_multi_kernel): matching at K IoU
thresholds in two phases.

  phase 1, once per detection, no threshold in sight: ``best`` (the largest IoU with any of the image's targets, fp32, the
           reference's "+1 pixel" bbox_iou), ``bidx`` (its first index) and ``has`` (the detection's label occurs among the
           image's target labels);
  phase 2, per threshold: walk the detections in order; detection i is a true positive at threshold k when
           has_i and best_i >= thr_k (fp32) and target bidx_i is still free at threshold k, and then takes it.

The claim this pins (tests/test_stats_multi_host.py): that is the reference's get_batch_statistics (utils/utils.py:194-230) at every
threshold - the best target does not depend on the threshold, and "stop once every target is matched" needs no code of its own.
Finite boxes are assumed (an IoU that is not a number never becomes ``best`` on the device; numpy's argmax would pick it)."""
import numpy as np

from oracle import yfv2_oracle as oracle

COCO_THRESHOLDS = np.linspace(0.5, 0.95, 10).astype(np.float32)


def phase1(dets, ann):
    """dets (n, 6) rows x1, y1, x2, y2, conf, label; ann (nt, 5) rows label, x1, y1, x2, y2 -> best (n) fp32, bidx (n), has (n)"""
    n = dets.shape[0]
    best, bidx, has = np.full(n, -1, np.float32), np.full(n, -1, np.int64), np.zeros(n, bool)
    if len(ann) == 0:
        return best, bidx, has
    for i in range(n):
        has[i] = dets[i, 5] in ann[:, 0]
        iou = oracle.bbox_iou_plus1(dets[i, :4], ann[:, 1:])
        bidx[i] = int(iou.argmax())            # the first maximum
        best[i] = iou[bidx[i]]
    return best, bidx, has


def walk(best, bidx, has, thresholds, nt):
    """-> (n) uint32, bit k = true positive at thresholds[k]"""
    thr = np.asarray(thresholds, np.float32).reshape(-1)
    assert 1 <= len(thr) <= 32
    mask = np.zeros(len(best), np.uint32)
    for k in range(len(thr)):
        free = np.ones(nt, bool)
        for i in range(len(best)):
            if has[i] and best[i] >= thr[k] and free[bidx[i]]:     # a NaN threshold: the comparison is False
                mask[i] |= np.uint32(1 << k)
                free[bidx[i]] = False
    return mask


def batch_statistics_multi(outputs, targets, thresholds):
    """outputs: list of (n_i, 6) arrays; targets (T, 6) rows image, label, x1, y1, x2, y2 -> list of (n_i) uint32 masks"""
    targets = np.asarray(targets, np.float32).reshape(-1, 6)
    masks = []
    for b, o in enumerate(outputs):
        o = np.asarray(o, np.float32).reshape(-1, 6)
        ann = targets[targets[:, 0] == b][:, 1:]
        best, bidx, has = phase1(o, ann)
        masks.append(walk(best, bidx, has, thresholds, len(ann)))
    return masks


def reference_masks(outputs, targets, thresholds):
    """the same masks from K runs of the oracle's get_batch_statistics, one per threshold"""
    masks = [np.zeros(np.asarray(o).reshape(-1, 6).shape[0], np.uint32) for o in outputs]
    for k, t in enumerate(np.asarray(thresholds, np.float32).reshape(-1)):
        for m, (tp, _, _) in zip(masks, oracle.get_batch_statistics(outputs, targets, t)):
            m |= (tp != 0).astype(np.uint32) << np.uint32(k)
    return masks


def det(x1, y1, x2, y2, conf, label):
    return [x1, y1, x2, y2, conf, label]


def hand_cases():
    """name -> (outputs, targets, thresholds).  Boxes are chosen so that every IoU is a ratio of small integers, exact in fp32:
    with the "+1 pixel" convention box (0, 0, 99, 99) has area 10000 and (0, 0, 99, h - 1) lies inside it with IoU h / 100."""
    f32 = lambda a: np.asarray(a, np.float32)
    cases = {}
    # the best IoU equals the threshold: 0.5 and 0.25 are exact, >= must hit at the value and miss one ulp above
    up, down = np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0))
    cases["threshold equals the iou"] = (
        [f32([det(0, 0, 99, 49, 0.9, 1), det(200, 200, 299, 224, 0.8, 1)])],
        f32([[0, 1, 0, 0, 99, 99], [0, 1, 200, 200, 299, 299]]),
        f32([0.5, up, down, 0.25, np.nextafter(np.float32(0.25), np.float32(1))]))
    # two detections of one class share their best target: the higher-ranked at IoU 0.6, the lower-ranked at 0.9.  Up to 0.6 the
    # first takes the target and the second misses; from 0.65 the first fails and the second hits; at 0.95 both miss.
    cases["non-monotone tp"] = (
        [f32([det(0, 0, 99, 59, 0.9, 3), det(0, 0, 99, 89, 0.8, 3)])],
        f32([[0, 3, 0, 0, 99, 99], [0, 3, 500, 500, 520, 520]]),
        COCO_THRESHOLDS)
    cases["unsorted thresholds, a repeat, a NaN, out of range"] = (
        cases["non-monotone tp"][0], cases["non-monotone tp"][1], f32([0.75, 0.5, np.nan, 0.5, 0.9, -1.0, 2.0, 0.6]))
    # a label no target carries is skipped and takes nothing; the next detection of a present label still gets the target.  The
    # third detection's best target carries ANOTHER label than its own: the reference matches across labels, and so does this.
    # Image 1's detection covers its only target exactly, but its label occurs in image 0 alone.
    cases["label not among the targets"] = (
        [f32([det(0, 0, 99, 99, 0.9, 7), det(0, 0, 99, 79, 0.8, 3), det(300, 300, 399, 389, 0.7, 3)]), f32([det(0, 0, 9, 9, 0.5, 4)])],
        f32([[0, 3, 0, 0, 99, 99], [0, 5, 300, 300, 399, 399], [1, 3, 0, 0, 9, 9]]),
        COCO_THRESHOLDS)
    return cases
