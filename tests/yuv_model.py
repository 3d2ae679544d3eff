"""The numpy statement of the YUV 4:2:0 -> B, G, R rule of include/yfv2.h (yfv2_frame_yuv), shared by
tests/test_yuv_host.py (CPU) and tests/test_gpu_yuv.py (GPU), plus helpers that build planes with pitch padding and poison
bytes around a frame.  (The resize's LDS and width limit: tests/rows_model.py.)  OpenCV is on neither machine: this is the published integer arithmetic written out, and parity with cv2
proper is unpinned, exactly as for the resize.
"""
import numpy as np

NV12, NV21, I420 = 0, 1, 2
BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL = 0, 1, 2, 3
FORMATS = (NV12, NV21, I420)
COLOURS = (BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL)
SHIFT = 20
# colour: (off, CY, CVR, CVG, CUG, CUB)
COEF = {
    BT601_LIMITED: (16, 1220542, 1673527, -852492, -409993, 2116026),   # OpenCV's COLOR_YUV2BGR_NV12 / _I420 literals
    BT709_LIMITED: (16, 1220945, 1879825, -558796, -223607, 2215014),
    BT601_FULL: (0, 1048576, 1470104, -748826, -360853, 1858077),       # JPEG
    BT709_FULL: (0, 1048576, 1651297, -490864, -196424, 1945738),
}
POISON = 0xA5


def accumulators(Y, U, V, colour):
    """the three int64 accumulators (R, G, B) before the shift - int64 here so that the range sweep can SEE an int32 overflow"""
    off, cy, cvr, cvg, cug, cub = COEF[colour]
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(Y - off, 0) * cy + (1 << (SHIFT - 1))
    u, v = U - 128, V - 128
    return yy + cvr * v, yy + cvg * v + cug * u, yy + cub * u


def convert(Y, U, V, colour):
    """(..., 3) uint8 B, G, R of broadcastable Y, U, V arrays"""
    r, g, b = accumulators(Y, U, V, colour)
    return np.stack([np.clip(a >> SHIFT, 0, 255) for a in (b, g, r)], axis=-1).astype(np.uint8)   # >> of a negative int: floor


def chroma_of(planes, fmt, R, C):
    """U, V at plane coordinates R (column vector) x C (row vector): the sample at (R >> 1, C >> 1), replicated"""
    if fmt == I420:
        return planes[1][R >> 1, C >> 1], planes[2][R >> 1, C >> 1]
    a, b = planes[1][R >> 1, 2 * (C >> 1)], planes[1][R >> 1, 2 * (C >> 1) + 1]
    return (a, b) if fmt == NV12 else (b, a)


def yuv_to_bgr(planes, fmt, colour, x0, y0, w, h):
    """planes: (y, uv) / (y, u, v) as 2-D uint8 arrays (any pitch: a row is a row of the array) -> (h, w, 3) uint8 B, G, R of the
    frame whose top-left pixel is (x0, y0) of the planes"""
    R = (y0 + np.arange(h))[:, None]
    C = (x0 + np.arange(w))[None, :]
    U, V = chroma_of(planes, fmt, R, C)
    return convert(planes[0][R, C], U, V, colour)


def chroma_shape(rows, cols, fmt):
    """(rows, bytes per row) of a chroma plane under a luma plane of rows x cols"""
    return (rows + 1) // 2, ((cols + 1) // 2) * (1 if fmt == I420 else 2)


def random_planes(rng, rows, cols, fmt):
    """full-range random planes for a rows x cols luma plane, tight pitch: U and V over 0..255, so the clamps fire"""
    cr, cb = chroma_shape(rows, cols, fmt)
    planes = [rng.integers(0, 256, (rows, cols), dtype=np.uint8)]
    for _ in range(2 if fmt == I420 else 1):
        planes.append(rng.integers(0, 256, (cr, cb), dtype=np.uint8))
    return tuple(planes)


def nv12_to(planes, fmt):
    """the same picture as NV12 `planes` in another format: NV21 swaps the byte pairs, I420 de-interleaves"""
    y, uv = planes
    if fmt == NV12:
        return y, uv
    if fmt == NV21:
        return y, np.ascontiguousarray(uv.reshape(uv.shape[0], -1, 2)[:, :, ::-1]).reshape(uv.shape)
    return y, np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])


def pad_plane(plane, pitch, poison=POISON):
    """the flat bytes of `plane` at row pitch `pitch` >= its width, allocated EXACTLY: (rows - 1) * pitch + width bytes, the
    padding between rows filled with `poison`"""
    rows, width = plane.shape
    assert pitch >= width
    flat = np.full((rows - 1) * pitch + width, poison, np.uint8)
    for r in range(rows):
        flat[r * pitch:r * pitch + width] = plane[r]
    return flat


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

