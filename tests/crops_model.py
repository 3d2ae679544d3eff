"""The numpy / Python statement of the second-stage crop rule (include/yfv2.h "second-stage crops"; the library's one
__host__ __device__ function is yfv2_crop_axis, yfv2_internal.h).  Python floats are IEEE doubles and every operation below is
rounded on its own, which is the whole specification of the arithmetic."""
import math

import numpy as np


def _axis(a1, a2, pad, n):
    """one axis: the box edges (doubles), the pad factor, the frame's length -> (origin, length) or None (skipped)"""
    b = a2 - a1
    if not b > 0.0:
        return None
    m = pad * b
    lo, hi = a1 - m, a2 + m
    c1 = lo if lo > 0.0 else 0.0            # max(ax1, 0)
    c2 = hi if hi < float(n) else float(n)  # min(ax2, n)
    if not c2 > c1:
        return None
    o, e = int(math.floor(c1)), int(math.ceil(c2))
    return o, e - o


def crop_rect(box, frame_h, frame_w, pad_x=0.0, pad_y=0.0):
    """box: x1, y1, x2, y2 (taken as fp32); pads taken as fp32 -> (X0, Y0, width, height) or None when the row is skipped"""
    x1, y1, x2, y2 = (float(np.float32(v)) for v in box)
    if not all(math.isfinite(v) for v in (x1, y1, x2, y2)):
        return None
    if not (x2 - x1 > 0.0 and y2 - y1 > 0.0):
        return None
    ax = _axis(x1, x2, float(np.float32(pad_x)), int(frame_w))
    ay = _axis(y1, y2, float(np.float32(pad_y)), int(frame_h))
    if ax is None or ay is None:
        return None
    return ax[0], ay[0], ax[1], ay[1]


def class_passes(cls, classes):
    """cls: the row's fp32 class column; classes: None (all) or ints in 0..254"""
    c = float(np.float32(cls))
    if not math.isfinite(c) or c != math.floor(c) or not 0.0 <= c <= 254.0:
        return False
    return classes is None or int(c) in set(int(k) for k in classes)


def plan(dets, count, sizes, pad_x=0.0, pad_y=0.0, max_per_frame=300, classes=None, cap=None):
    """dets (B, R, 6) fp32, count (B) ints, sizes: B pairs (h, w).  Returns a dict: src, rect (the crops that are written, k <
    min(total, cap)), offset (B + 1; offset[B] = the untruncated total), skipped (B) and frame (the frame of each written crop)."""
    dets = np.asarray(dets, np.float32)
    B, R = dets.shape[0], dets.shape[1]
    src, rect, frame, offset, skipped = [], [], [], [0], []
    for b in range(B):
        n = min(max(int(count[b]), 0), R)
        h, w = sizes[b]
        taken, skip = 0, 0
        for r in range(n):
            if not class_passes(dets[b, r, 5], classes):
                continue
            rc = crop_rect(dets[b, r, :4], h, w, pad_x, pad_y)
            if rc is None:
                skip += 1               # every skipped candidate of the frame counts, before or after the cut
                continue
            if taken < max_per_frame:
                src.append(b * R + r); rect.append(rc); frame.append(b)
                taken += 1
        offset.append(offset[-1] + taken)
        skipped.append(skip)
    live = len(src) if cap is None else min(len(src), int(cap))
    return {"src": np.asarray(src[:live], np.int32), "rect": np.asarray(rect[:live], np.int32).reshape(-1, 4),
            "frame": np.asarray(frame[:live], np.int32), "offset": np.asarray(offset, np.int32), "skipped": np.asarray(skipped, np.int32)}
