"""The numpy statement of the 8-bit YUV formats of include/yfv2.h beyond 4:2:0 (yfv2_frame_yuv: YFV2_YUV_I422, _I440, _I444, _YUYV,
_UYVY, _GREY), together with the three 4:2:0 ones: where pixel (R, C) of the planes reads its luma, U and V, then
the colour rule of tests/yuv_model.py (imported, not restated).  Shared by tests/test_yuv_any_host.py (CPU) and
tests/test_gpu_yuv_any.py (GPU).  Also the general launch's LDS bytes and width limit, restated from the layout.
"""
import numpy as np

import rows_model as rm
from yuv_model import BT601_FULL, BT601_LIMITED, BT709_FULL, BT709_LIMITED, COEF, COLOURS, POISON, convert, pad_plane  # noqa: F401

NV12, NV21, I420, I422, I440, I444, YUYV, UYVY, GREY = range(9)
FORMATS = (NV12, NV21, I420, I422, I440, I444, YUYV, UYVY, GREY)
NEW_FORMATS = (I422, I440, I444, YUYV, UYVY, GREY)
NAMES = {NV12: "nv12", NV21: "nv21", I420: "i420", I422: "i422", I440: "i440", I444: "i444", YUYV: "yuyv", UYVY: "uyvy", GREY: "grey"}
PLANAR = (I420, I422, I440, I444)
PACKED = (YUYV, UYVY)
# format -> (sx, sy): pixel (R, C) takes the chroma sample (R >> sy, C >> sx)
SHIFTS = {NV12: (1, 1), NV21: (1, 1), I420: (1, 1), I422: (1, 0), I440: (0, 1), I444: (0, 0), YUYV: (1, 0), UYVY: (1, 0), GREY: (0, 0)}


def offsets(fmt, R, C):
    """((plane index, row, byte) of luma, of U, of V) for pixel (R, C) - include/yfv2.h's table; GREY: U and V are None (the value 128)"""
    sx, sy = SHIFTS[fmt]
    if fmt == GREY:
        return (0, R, C), None, None
    if fmt == YUYV:
        return (0, R, 2 * C), (0, R, 4 * (C >> 1) + 1), (0, R, 4 * (C >> 1) + 3)
    if fmt == UYVY:
        return (0, R, 2 * C + 1), (0, R, 4 * (C >> 1)), (0, R, 4 * (C >> 1) + 2)
    if fmt in PLANAR:
        return (0, R, C), (1, R >> sy, C >> sx), (2, R >> sy, C >> sx)
    a, b = (1, R >> 1, 2 * (C >> 1)), (1, R >> 1, 2 * (C >> 1) + 1)
    return ((0, R, C), a, b) if fmt == NV12 else ((0, R, C), b, a)


def yuv_to_bgr(planes, fmt, colour, x0, y0, w, h):
    """planes: 2-D uint8 arrays (a row is a row of the array; a packed plane is rows x bytes) -> (h, w, 3) uint8 B, G, R of the
    frame whose top-left pixel is (x0, y0) of the planes"""
    R = (y0 + np.arange(h))[:, None]
    C = (x0 + np.arange(w))[None, :]
    ly, lu, lv = offsets(fmt, R, C)
    Y = planes[ly[0]][ly[1], ly[2]]
    if lu is None:
        return convert(Y, 128, 128, colour)
    return convert(Y, planes[lu[0]][lu[1], lu[2]], planes[lv[0]][lv[1], lv[2]], colour)


def plane_shapes(rows, cols, fmt):
    """the (rows, bytes) of each plane of a picture of rows x cols pixels, tight"""
    sx, sy = SHIFTS[fmt]
    cr, cc = ((rows - 1) >> sy) + 1, ((cols - 1) >> sx) + 1
    if fmt == GREY:
        return [(rows, cols)]
    if fmt in PACKED:
        return [(rows, 4 * cc)]
    if fmt in PLANAR:
        return [(rows, cols), (cr, cc), (cr, cc)]
    return [(rows, cols), (cr, 2 * cc)]


def random_planes(rng, rows, cols, fmt):
    """full-range random planes, tight pitch: every byte over 0..255, so the clamps fire"""
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in plane_shapes(rows, cols, fmt))


def from_i444(planes, fmt):
    """the picture of I444 `planes` in another format, subsampled by TAKING the chroma sample at the even positions (no averaging):
    the formats then agree wherever they must.  A packed row of an odd width ends with a macropixel whose second luma byte is 0."""
    y, u, v = planes
    rows, cols = y.shape
    sx, sy = SHIFTS[fmt]
    us, vs = u[::1 << sy, ::1 << sx], v[::1 << sy, ::1 << sx]
    if fmt == GREY:
        return (y.copy(),)
    if fmt in PLANAR:
        return y.copy(), np.ascontiguousarray(us), np.ascontiguousarray(vs)
    if fmt in PACKED:
        cc = us.shape[1]
        ypad = np.zeros((rows, 2 * cc), np.uint8)
        ypad[:, :cols] = y
        out = np.zeros((rows, 4 * cc), np.uint8)
        yo, uo = (0, 1) if fmt == YUYV else (1, 0)
        out[:, yo::2] = ypad
        out[:, uo::4] = us
        out[:, uo + 2::4] = vs
        return (out,)
    uv = np.zeros((us.shape[0], 2 * us.shape[1]), np.uint8)
    uv[:, (0 if fmt == NV12 else 1)::2] = us
    uv[:, (1 if fmt == NV12 else 0)::2] = vs
    return y.copy(), uv


# ---- the general launch's LDS: six slots of slot(w), a group of three per blended source row ([luma][U][V]; an interleaved row
# lies over U and V, a packed row over all three), then the row kind's own bytes (tests/rows_model.py) ----
def lds_bytes(kind, w, W):
    return 6 * rm.slot(w, rm.align(kind)) + rm.own_bytes(kind, W)


def max_width(kind, W):
    """the exact maximum, by bisection (the function never falls)"""
    lo, hi = 1, rm.LDS_FULL
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lds_bytes(kind, mid, W) <= rm.LDS_FULL:
            lo = mid
        else:
            hi = mid - 1
    return lo


def bgr_to_i444(bgr):
    """a full-range BT.601 (JPEG) B, G, R picture -> I444 planes of no particular pedigree: test pictures only"""
    b, g, r = (bgr[..., k].astype(np.float64) for k in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    u = 128 - 0.168736 * r - 0.331264 * g + 0.5 * b
    v = 128 + 0.5 * r - 0.418688 * g - 0.081312 * b
    return tuple(np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in (y, u, v))
