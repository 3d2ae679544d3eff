"""The numpy statement of the YUV -> B, G, R rule of include/yfv2.h (yfv2_frame_yuv) for all eleven
formats, written from the rule and not from the library or the package: ONE format table, where pixel (R, C) of the planes reads
its luma, U and V, the value of a 16-bit word, the colour formula at 8 and at 10 bits, planes with pitch padding and poison around
a frame, and the converters that make one picture in several formats.  Shared by the tests/test_yuv*_host.py files (CPU) and
the tests/test_gpu_yuv*.py files (GPU).  (The row kernels' LDS and width limits: tests/rows_model.py.)  OpenCV is on neither
machine: the 8-bit rule is the published integer arithmetic written out, cv2 has no P010 conversion, and parity with cv2 proper is
unpinned, exactly as for the resize.
"""
import collections

import numpy as np

Format = collections.namedtuple("Format", "name bits planes shifts layout lsb")
# the header's YFV2_YUV_* value: name, bits of a sample, number of planes, (sx, sy) - pixel (R, C) takes the chroma sample
# (R >> sy, C >> sx) - how U and V lie ("interleaved": one plane of pairs; "planar": a plane each; "packed": 4-byte macropixels
# with the luma; "grey": none), and for two-byte samples the lowest bit of the value in its little-endian word (P010: the high 10
# bits, I010: the low 10; the other 6 are ignored)
TABLE = {
    0: Format("nv12", 8, 2, (1, 1), "interleaved", None),
    1: Format("nv21", 8, 2, (1, 1), "interleaved", None),
    2: Format("i420", 8, 3, (1, 1), "planar", None),
    3: Format("i422", 8, 3, (1, 0), "planar", None),
    4: Format("i440", 8, 3, (0, 1), "planar", None),
    5: Format("i444", 8, 3, (0, 0), "planar", None),
    6: Format("yuyv", 8, 1, (1, 0), "packed", None),
    7: Format("uyvy", 8, 1, (1, 0), "packed", None),
    8: Format("grey", 8, 1, (0, 0), "grey", None),
    16: Format("p010", 10, 2, (1, 1), "interleaved", 6),
    17: Format("i010", 10, 3, (1, 1), "planar", 0),
}
NV12, NV21, I420, I422, I440, I444, YUYV, UYVY, GREY, P010, I010 = TABLE
FORMATS = tuple(TABLE)
NAMES = {f: t.name for f, t in TABLE.items()}
SHIFTS = {f: t.shifts for f, t in TABLE.items()}
PLANAR = tuple(f for f, t in TABLE.items() if t.layout == "planar")
PACKED = tuple(f for f, t in TABLE.items() if t.layout == "packed")
FORMATS8 = tuple(f for f, t in TABLE.items() if t.bits == 8)
FORMATS16 = tuple(f for f, t in TABLE.items() if t.bits == 10)
FORMATS420 = tuple(f for f in FORMATS8 if SHIFTS[f] == (1, 1))                 # the three a video decoder writes
NEW_FORMATS = tuple(f for f in FORMATS8 if f not in FORMATS420)               # the 8-bit samplings beyond 4:2:0

BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL = 0, 1, 2, 3
COLOURS = (BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL)
SHIFT = 20
# bits: colour: (off, CY, CVR, CVG, CUG, CUB)
COEF = {
    8: {
        BT601_LIMITED: (16, 1220542, 1673527, -852492, -409993, 2116026),   # OpenCV's COLOR_YUV2BGR_NV12 / _I420 literals
        BT709_LIMITED: (16, 1220945, 1879825, -558796, -223607, 2215014),
        BT601_FULL: (0, 1048576, 1470104, -748826, -360853, 1858077),       # JPEG
        BT709_FULL: (0, 1048576, 1651297, -490864, -196424, 1945738),
    },
    10: {   # each rint(k * 2^20) of the real coefficient per 10-bit code (coefficients() below)
        BT601_LIMITED: (64, 305236, 418389, -213115, -102698, 528805),
        BT709_LIMITED: (64, 305236, 469956, -139699, -55902, 553753),
        BT601_FULL: (0, 261375, 366448, -186658, -89949, 463157),
        BT709_FULL: (0, 261375, 411614, -122356, -48962, 485008),
    },
}
KR_KB = {BT601_LIMITED: (0.299, 0.114), BT601_FULL: (0.299, 0.114), BT709_LIMITED: (0.2126, 0.0722), BT709_FULL: (0.2126, 0.0722)}
POISON, POISON16 = 0xA5, 0xA5A5


def coefficients(colour):
    """the 10-bit table row from the formulas, in float64: limited range maps 219 * 4 luma codes and 224 * 4 chroma codes to 255,
    full range 1023 codes of either"""
    kr, kb = KR_KB[colour]
    kg = 1.0 - kr - kb
    limited = colour in (BT601_LIMITED, BT709_LIMITED)
    sy, sc = (255.0 / (219 * 4), 255.0 / (224 * 4)) if limited else (255.0 / 1023, 255.0 / 1023)
    real = (sy, sc * 2 * (1 - kr), sc * -2 * kr * (1 - kr) / kg, sc * -2 * kb * (1 - kb) / kg, sc * 2 * (1 - kb))
    return (64 if limited else 0,) + tuple(int(np.rint(k * (1 << SHIFT))) for k in real)


# ---- the colour rule ---------------------------------------------------------------------------------------------------------
def accumulators(Y, U, V, colour, bits=8):
    """the three int64 accumulators (R, G, B) before the shift - int64 here so that a range sweep can SEE an int32 overflow"""
    off, cy, cvr, cvg, cug, cub = COEF[bits][colour]
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(Y - off, 0) * cy + (1 << (SHIFT - 1))
    u, v = U - (1 << (bits - 1)), V - (1 << (bits - 1))
    return yy + cvr * v, yy + cvg * v + cug * u, yy + cub * u


def convert(Y, U, V, colour, bits=8):
    """(..., 3) uint8 B, G, R of broadcastable Y, U, V arrays of `bits`-bit values: at 10 bits rounded once from 10-bit precision"""
    r, g, b = accumulators(Y, U, V, colour, bits)
    bgr = [np.clip(a >> SHIFT, 0, 255).astype(np.uint8) for a in (b, g, r)]                       # >> of a negative int: floor
    return np.stack(np.broadcast_arrays(*bgr), axis=-1)


# ---- two-byte samples ----------------------------------------------------------------------------------------------------------
def sample_values(words, fmt):
    """the 10-bit values of little-endian 16-bit words of format fmt; the other 6 bits are ignored"""
    return (np.asarray(words).astype(np.uint16).astype(np.int64) >> TABLE[fmt].lsb) & 1023


def pack(values, fmt, junk=0):
    """words that carry `values` (0..1023) in format fmt, with the 6 bits of `junk` (0..63) in the ignored bits"""
    v, j = np.asarray(values).astype(np.int64), np.asarray(junk).astype(np.int64)
    lsb = TABLE[fmt].lsb
    return (v << lsb | j << (0 if lsb else 10)).astype(np.uint16)


# ---- addressing ------------------------------------------------------------------------------------------------------------------
def offsets(fmt, R, C):
    """((plane index, row, sample) of luma, of U, of V) for pixel (R, C) - include/yfv2.h's table; GREY: U and V are None (the
    midpoint).  P010 addresses like NV12 and I010 like I420, in samples."""
    layout, (sx, sy) = TABLE[fmt].layout, SHIFTS[fmt]
    if layout == "grey":
        return (0, R, C), None, None
    if layout == "packed":
        yo, uo = (0, 1) if fmt == YUYV else (1, 0)
        return (0, R, 2 * C + yo), (0, R, 4 * (C >> 1) + uo), (0, R, 4 * (C >> 1) + uo + 2)
    if layout == "planar":
        return (0, R, C), (1, R >> sy, C >> sx), (2, R >> sy, C >> sx)
    a, b = (1, R >> 1, 2 * (C >> 1)), (1, R >> 1, 2 * (C >> 1) + 1)
    return ((0, R, C), b, a) if fmt == NV21 else ((0, R, C), a, b)


def yuv_to_bgr(planes, fmt, colour, x0, y0, w, h):
    """planes: 2-D arrays of samples - uint8, or uint16 words for the two-byte formats (a row is a row of the array, so any pitch;
    a packed plane is rows x bytes) -> (h, w, 3) uint8 B, G, R of the frame whose top-left pixel is sample (x0, y0) of the planes"""
    bits = TABLE[fmt].bits
    R = (y0 + np.arange(h))[:, None]
    C = (x0 + np.arange(w))[None, :]

    def read(loc):
        if loc is None:
            return 1 << (bits - 1)
        a = planes[loc[0]][loc[1], loc[2]]
        return sample_values(a, fmt) if bits == 10 else a
    return convert(*(read(loc) for loc in offsets(fmt, R, C)), colour, bits)


def plane_shapes(rows, cols, fmt):
    """the (rows, samples) of each plane of a picture of rows x cols pixels, tight (a packed plane: bytes)"""
    layout, (sx, sy) = TABLE[fmt].layout, SHIFTS[fmt]
    cr, cc = ((rows - 1) >> sy) + 1, ((cols - 1) >> sx) + 1
    return {"grey": [(rows, cols)], "packed": [(rows, 4 * cc)], "planar": [(rows, cols), (cr, cc), (cr, cc)], "interleaved": [(rows, cols), (cr, 2 * cc)]}[layout]


def random_planes(rng, rows, cols, fmt, junk=True):
    """random planes for a rows x cols picture, tight pitch: every sample over its full range (0..255 / 0..1023), so the clamps
    fire; at 10 bits with random junk in the ignored bits (junk=False: zeros there, what a decoder writes)"""
    shapes = plane_shapes(rows, cols, fmt)
    if TABLE[fmt].bits == 8:
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)
    return tuple(pack(rng.integers(0, 1024, s), fmt, rng.integers(0, 64, s) if junk else 0) for s in shapes)


def pad_plane(plane, pitch, poison=None):
    """the flat samples of `plane` at a row pitch of `pitch` samples >= its width, allocated EXACTLY: (rows - 1) * pitch + width, the
    padding between rows filled with `poison` (default: the poison byte or word of the plane's dtype)"""
    rows, width = plane.shape
    assert pitch >= width
    flat = np.full((rows - 1) * pitch + width, (POISON if plane.dtype.itemsize == 1 else POISON16) if poison is None else poison, plane.dtype)
    for r in range(rows):
        flat[r * pitch:r * pitch + width] = plane[r]
    return flat


# ---- one picture in several formats, and test pictures ----------------------------------------------------------------------------
def nv12_to(planes, fmt):
    """the same picture as NV12 `planes` in another format: NV21 swaps the byte pairs, I420 de-interleaves"""
    y, uv = planes
    if fmt == NV12:
        return y, uv
    if fmt == NV21:
        return y, np.ascontiguousarray(uv.reshape(uv.shape[0], -1, 2)[:, :, ::-1]).reshape(uv.shape)
    return y, np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])


def to_format(planes_p010, fmt):
    """the same values as P010 `planes` (zeros in the ignored bits) in format fmt: I010 de-interleaves and moves the value down"""
    y, uv = planes_p010
    if fmt == P010:
        return y, uv
    return tuple(pack(sample_values(np.ascontiguousarray(p), P010), I010) for p in (y, uv[:, 0::2], uv[:, 1::2]))


def from_i444(planes, fmt):
    """the picture of I444 `planes` in another 8-bit format, subsampled by TAKING the chroma sample at the even positions (no
    averaging): the formats then agree wherever they must.  A packed row of an odd width ends with a macropixel whose second luma
    byte is 0."""
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


def bgr_to_nv12(bgr):
    """a BT.601 limited-range B, G, R -> NV12 of no particular pedigree (2 x 2 box-averaged chroma): test pictures only"""
    b, g, r = (bgr[..., k].astype(np.float64) for k in range(3))
    h, w = b.shape
    y = np.clip(np.rint(16 + 0.257 * r + 0.504 * g + 0.098 * b), 0, 255).astype(np.uint8)
    u = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    ch, cw = (h + 1) // 2, (w + 1) // 2
    uv = np.zeros((ch, 2 * cw), np.uint8)
    for k, p in enumerate((u, v)):
        q = np.pad(p, ((0, 2 * ch - h), (0, 2 * cw - w)), mode="edge").reshape(ch, 2, cw, 2).mean(axis=(1, 3))
        uv[:, k::2] = np.clip(np.rint(q), 0, 255).astype(np.uint8)
    return y, uv


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


def bgr_to_i444(bgr):
    """a full-range BT.601 (JPEG) B, G, R picture -> I444 planes of no particular pedigree: test pictures only"""
    b, g, r = (bgr[..., k].astype(np.float64) for k in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    u = 128 - 0.168736 * r - 0.331264 * g + 0.5 * b
    v = 128 + 0.5 * r - 0.418688 * g - 0.081312 * b
    return tuple(np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in (y, u, v))
