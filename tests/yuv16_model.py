"""The numpy statement of the 10-bit YUV 4:2:0 -> B, G, R rule of include/yfv2.h (YFV2_YUV_P010 / YFV2_YUV_I010),
written from the rule and not from the library, shared by tests/test_yuv16_host.py (CPU) and tests/test_gpu_yuv16.py (GPU): the
value of a 16-bit word in either format, the colour formula, the chroma addressing, planes with junk in the ignored bits and with
poison words between rows, and the LDS / width limit of the row kernels' two-byte instantiations (the slot, the rows' own bytes
and their alignment come from tests/rows_model.py).  cv2 has no P010 conversion: the literals are the formulas below, rounded.
"""
import numpy as np

from rows_model import LDS_FULL, align, own_bytes, slot

P010, I010 = 16, 17
FORMATS = (P010, I010)
BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL = 0, 1, 2, 3
COLOURS = (BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL)
SHIFT = 20
# colour: (off, CY, CVR, CVG, CUG, CUB), each rint(k * 2^20) of the real coefficient per 10-bit code (coefficients() below)
COEF = {
    BT601_LIMITED: (64, 305236, 418389, -213115, -102698, 528805),
    BT709_LIMITED: (64, 305236, 469956, -139699, -55902, 553753),
    BT601_FULL: (0, 261375, 366448, -186658, -89949, 463157),
    BT709_FULL: (0, 261375, 411614, -122356, -48962, 485008),
}
KR_KB = {BT601_LIMITED: (0.299, 0.114), BT601_FULL: (0.299, 0.114), BT709_LIMITED: (0.2126, 0.0722), BT709_FULL: (0.2126, 0.0722)}
POISON = 0xA5A5


def coefficients(colour):
    """the table row from the formulas, in float64: limited range maps 219 * 4 luma codes and 224 * 4 chroma codes to 255, full
    range 1023 codes of either"""
    kr, kb = KR_KB[colour]
    kg = 1.0 - kr - kb
    limited = colour in (BT601_LIMITED, BT709_LIMITED)
    sy, sc = (255.0 / (219 * 4), 255.0 / (224 * 4)) if limited else (255.0 / 1023, 255.0 / 1023)
    real = (sy, sc * 2 * (1 - kr), sc * -2 * kr * (1 - kr) / kg, sc * -2 * kb * (1 - kb) / kg, sc * 2 * (1 - kb))
    return (64 if limited else 0,) + tuple(int(np.rint(k * (1 << SHIFT))) for k in real)


def sample_values(words, fmt):
    """the 10-bit values of little-endian 16-bit words: P010 in the high 10 bits, I010 in the low 10; the other 6 are ignored"""
    w = np.asarray(words).astype(np.uint16).astype(np.int64)
    return w >> 6 if fmt == P010 else w & 1023


def pack(values, fmt, junk=0):
    """words that carry `values` (0..1023) in format fmt, with the 6 bits of `junk` (0..63) in the ignored bits"""
    v, j = np.asarray(values).astype(np.int64), np.asarray(junk).astype(np.int64)
    return ((v << 6 | j) if fmt == P010 else (j << 10 | v)).astype(np.uint16)


def accumulators(Y, U, V, colour):
    """the three int64 accumulators (R, G, B) before the shift, of 10-bit values - int64 so that a range sweep SEES an int32 overflow"""
    off, cy, cvr, cvg, cug, cub = COEF[colour]
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(Y - off, 0) * cy + (1 << (SHIFT - 1))
    u, v = U - 512, V - 512
    return yy + cvr * v, yy + cvg * v + cug * u, yy + cub * u


def convert(Y, U, V, colour):
    """(..., 3) uint8 B, G, R of broadcastable 10-bit Y, U, V: rounded once from 10-bit precision"""
    r, g, b = accumulators(Y, U, V, colour)
    bgr = [np.clip(a >> SHIFT, 0, 255).astype(np.uint8) for a in (b, g, r)]                       # >> of a negative int: floor
    return np.stack(np.broadcast_arrays(*bgr), axis=-1)


def chroma_of(planes, fmt, R, C):
    """the U, V WORDS at plane coordinates R (column vector) x C (row vector): the sample at (R >> 1, C >> 1), replicated; P010 has
    U first in the interleaved plane"""
    if fmt == I010:
        return planes[1][R >> 1, C >> 1], planes[2][R >> 1, C >> 1]
    return planes[1][R >> 1, 2 * (C >> 1)], planes[1][R >> 1, 2 * (C >> 1) + 1]


def yuv_to_bgr(planes, fmt, colour, x0, y0, w, h):
    """planes: (y, uv) / (y, u, v) as 2-D uint16 arrays of words (a row is a row of the array) -> (h, w, 3) uint8 B, G, R of the
    frame whose top-left pixel is sample (x0, y0) of the planes"""
    R = (y0 + np.arange(h))[:, None]
    C = (x0 + np.arange(w))[None, :]
    U, V = chroma_of(planes, fmt, R, C)
    return convert(sample_values(planes[0][R, C], fmt), sample_values(U, fmt), sample_values(V, fmt), colour)


def chroma_shape(rows, cols, fmt):
    """(rows, words per row) of a chroma plane under a luma plane of rows x cols"""
    return (rows + 1) // 2, ((cols + 1) // 2) * (1 if fmt == I010 else 2)


def random_planes(rng, rows, cols, fmt, junk=True):
    """random planes of words for a rows x cols luma plane, tight pitch: values over all of 0..1023, so the clamps fire, and
    random junk in the ignored bits (junk=False: zeros there, what a decoder writes)"""
    shapes = [(rows, cols)] + [chroma_shape(rows, cols, fmt)] * (2 if fmt == I010 else 1)
    return tuple(pack(rng.integers(0, 1024, s), fmt, rng.integers(0, 64, s) if junk else 0) for s in shapes)


def to_format(planes_p010, fmt):
    """the same values as P010 `planes` (zeros in the ignored bits) in format fmt: I010 de-interleaves and moves the value down"""
    y, uv = planes_p010
    if fmt == P010:
        return y, uv
    return tuple(pack(sample_values(np.ascontiguousarray(p), P010), I010) for p in (y, uv[:, 0::2], uv[:, 1::2]))


def pad_plane(plane, pitch, poison=POISON):
    """the flat WORDS of `plane` at a row pitch of `pitch` words >= its width, allocated EXACTLY: (rows - 1) * pitch + width words, the
    padding between rows filled with the poison word"""
    rows, width = plane.shape
    assert pitch >= width
    flat = np.full((rows - 1) * pitch + width, poison, np.uint16)
    for r in range(rows):
        flat[r * pitch:r * pitch + width] = plane[r]
    return flat


def bgr_to_p010(bgr):
    """an 8-bit B, G, R picture -> BT.601 limited-range P010 planes of no particular pedigree (10-bit codes = 4 x the 8-bit real
    values, rounded at 10 bits; 2 x 2 box-averaged chroma): test pictures only"""
    b, g, r = (bgr[..., k].astype(np.float64) for k in range(3))
    h, w = b.shape
    y = np.clip(np.rint(4 * (16 + 0.257 * r + 0.504 * g + 0.098 * b)), 0, 1023)
    u = 4 * (128 - 0.148 * r - 0.291 * g + 0.439 * b)
    v = 4 * (128 + 0.439 * r - 0.368 * g - 0.071 * b)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    uv = np.zeros((ch, 2 * cw))
    for k, p in enumerate((u, v)):
        q = np.pad(p, ((0, 2 * ch - h), (0, 2 * cw - w)), mode="edge").reshape(ch, 2, cw, 2).mean(axis=(1, 3))
        uv[:, k::2] = np.clip(np.rint(q), 0, 1023)
    return pack(y, P010), pack(uv, P010)


# ---- the LDS of a workgroup of the two-byte instantiations and the exact width limit (the kernel: yfv2_pre.hip) -----------------
def lds_bytes(kind, w, W):
    """two luma rows of 2 w bytes and two chroma rows, each either one interleaved row of 2 * 2 * (w // 2 + 1) bytes or two planar
    rows of 2 * (w // 2 + 1) in a half-slot each, then the row's own bytes"""
    a = align(kind)
    half = slot(2 * (w // 2 + 1), a)
    assert 2 * half >= slot(2 * 2 * (w // 2 + 1), a)
    return 2 * slot(2 * w, a) + 2 * 2 * half + own_bytes(kind, W)


def max_width(kind, W):
    """the widest frame with lds_bytes <= a CU's LDS, by bisection on a function that never falls (1 if none fits)"""
    lo, hi = 1, LDS_FULL
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lds_bytes(kind, mid, W) <= LDS_FULL:
            lo = mid
        else:
            hi = mid - 1
    return lo
