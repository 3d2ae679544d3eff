"""CPU-only checks of the YUV 4:2:0 front door (include/yfv2.h yfv2_frame_yuv): the colour rule's known
points and its int32 range, the chroma indexing at every parity, the format relations, the staging guard per plane and the
LDS / width limit.  The device side is tests/test_gpu_yuv.py."""
import numpy as np
import pytest

import rows_model as rm
import yuv_model as ym
from frames_ref import stage_row

FORMATS = ym.FORMATS420


# ---- 1. the colour rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", ym.COLOURS)
def test_known_triplets_and_clamps(colour):
    limited = colour in (ym.BT601_LIMITED, ym.BT709_LIMITED)
    black, white = (16, 235) if limited else (0, 255)
    assert ym.convert(black, 128, 128, colour).tolist() == [0, 0, 0]
    assert ym.convert(white, 128, 128, colour).tolist() == [255, 255, 255]
    # grey stays grey: no chroma, three equal channels
    g = ym.convert(np.arange(256), 128, 128, colour)
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 1], g[:, 2]) and np.all(np.diff(g[:, 0].astype(int)) >= 0)
    if limited:   # below black and above white: the luma floor and the upper clamp
        assert ym.convert(0, 128, 128, colour).tolist() == [0, 0, 0] and ym.convert(255, 128, 128, colour).tolist() == [255, 255, 255]
    # both clamps of every channel: V drives R (and G the other way), U drives B (and G the other way)
    assert ym.convert(white, 128, 255, colour)[2] == 255 and ym.convert(black, 128, 0, colour)[2] == 0
    assert ym.convert(white, 255, 128, colour)[0] == 255 and ym.convert(black, 0, 128, colour)[0] == 0
    assert ym.convert(white, 0, 0, colour)[1] == 255 and ym.convert(black, 255, 255, colour)[1] == 0
    # the clamps really fire: the unclamped values leave [0, 255]
    r, _, b = ym.accumulators(white, 255, 255, colour)
    assert (r >> ym.SHIFT) > 255 and (b >> ym.SHIFT) > 255
    r, _, b = ym.accumulators(black, 0, 0, colour)
    assert (r >> ym.SHIFT) < 0 and (b >> ym.SHIFT) < 0


def test_bt601_limited_midpoints_by_hand():
    """(81, 90, 240) is BT.601 limited-range pure red, (145, 54, 34) pure green, (41, 240, 110) pure blue - to a unit"""
    for yuv, bgr in (((81, 90, 240), (0, 0, 255)), ((145, 54, 34), (0, 255, 0)), ((41, 240, 110), (255, 0, 0))):
        got = ym.convert(*yuv, ym.BT601_LIMITED).astype(int)
        assert np.abs(got - np.array(bgr)).max() <= 2, (yuv, got)
    # one value by hand: Y 100, U 100, V 200 -> yy = 84 * 1220542 + 524288 = 103049816
    assert ym.convert(100, 100, 200, ym.BT601_LIMITED).tolist() == [
        (103049816 + 2116026 * -28) >> 20, (103049816 + -852492 * 72 + -409993 * -28) >> 20, (103049816 + 1673527 * 72) >> 20]


@pytest.mark.parametrize("colour", ym.COLOURS)
def test_accumulators_fit_int32_over_all_triples(colour):
    """all 2^24 (Y, U, V): every accumulator, and the luma product alone, stays inside int32 - the kernel computes in int"""
    Y = np.arange(256)[:, None, None]
    U = np.arange(256)[None, :, None]
    V = np.arange(256)[None, None, :]
    worst = 0
    for a in ym.accumulators(Y, U, V, colour):
        worst = max(worst, int(np.abs(a).max()))
    assert worst < 2 ** 31 - 1, worst
    assert 5.0e8 < worst < 6.0e8, worst      # the largest |accumulator| is about 5.7e8 for each standard
    off, cy = ym.COEF[8][colour][:2]
    assert (255 - off) * cy + (1 << 19) < 2 ** 31


# ---- 2. chroma indexing --------------------------------------------------------------------------------------------------------
def _folded(planes, fmt, colour, x0, y0, w, h):
    """the kernel's view (ResizeFrameYuv): the origin folded into the plane pointers, the parities kept - pixel (r, c) reads luma
    y[r, c] and chroma row (r + py) >> 1, sample (c + px) >> 1 from the folded bases"""
    px, py = x0 & 1, y0 & 1
    step = 1 if fmt == ym.I420 else 2
    y = planes[0][y0:, x0:]
    ca = planes[1][y0 >> 1:, (x0 >> 1) * step:]
    cb = planes[2][y0 >> 1:, x0 >> 1:] if fmt == ym.I420 else None
    cw, ch = ((w - 1 + px) >> 1) + 1, ((h - 1 + py) >> 1) + 1
    assert ca.shape[0] >= ch and ca.shape[1] >= cw * step     # the chroma rectangle the kernel stages lies inside the plane
    r = np.arange(h)[:, None]
    c = np.arange(w)[None, :]
    j = ((c + px) >> 1) * step
    cr = (r + py) >> 1
    assert j.max() + step <= cw * step and cr.max() < ch
    if fmt == ym.I420:
        U, V = ca[cr, j], cb[cr, j]
    else:
        U, V = (ca[cr, j], ca[cr, j + 1]) if fmt == ym.NV12 else (ca[cr, j + 1], ca[cr, j])
    return ym.convert(y[r, c], U, V, colour)


@pytest.mark.parametrize("fmt", FORMATS)
def test_chroma_indexing_every_parity(fmt):
    """the kernel's folded view reads what the model reads (the model against offsets by hand, every format:
    tests/test_yuv_any_host.py test_chroma_addressing_every_parity)"""
    rng = np.random.default_rng(5 + fmt)
    planes = ym.random_planes(rng, 11, 13, fmt)
    cases = [(x0, y0, w, h) for x0 in (0, 1, 2, 3) for y0 in (0, 1, 2) for w, h in ((1, 1), (2, 2), (3, 5), (4, 3), (7, 6))]
    cases += [(0, 0, 13, 11), (12, 10, 1, 1), (5, 4, 8, 7), (6, 5, 7, 6)]          # the whole plane; its last pixel; ending on the last row and column
    for x0, y0, w, h in cases:
        assert np.array_equal(_folded(planes, fmt, ym.BT709_LIMITED, x0, y0, w, h), ym.yuv_to_bgr(planes, fmt, ym.BT709_LIMITED, x0, y0, w, h)), (x0, y0, w, h)
    # 2 x 2 blocks share their chroma: an even-origin 2 x 2 frame with constant luma is one colour, an odd-origin one is four
    flat = (np.full_like(planes[0], 128),) + planes[1:]
    assert len(np.unique(ym.yuv_to_bgr(flat, fmt, 0, 2, 2, 2, 2).reshape(-1, 3), axis=0)) == 1
    assert len(np.unique(ym.yuv_to_bgr(flat, fmt, 0, 1, 1, 2, 2).reshape(-1, 3), axis=0)) == 4


def test_formats_are_one_picture():
    rng = np.random.default_rng(9)
    nv12 = ym.random_planes(rng, 9, 7, ym.NV12)
    want = ym.yuv_to_bgr(nv12, ym.NV12, ym.BT601_FULL, 1, 2, 6, 7)
    nv21 = ym.nv12_to(nv12, ym.NV21)
    assert np.array_equal(nv21[1][:, 0::2], nv12[1][:, 1::2]) and np.array_equal(nv21[1][:, 1::2], nv12[1][:, 0::2])
    assert np.array_equal(ym.yuv_to_bgr(nv21, ym.NV21, ym.BT601_FULL, 1, 2, 6, 7), want)
    i420 = ym.nv12_to(nv12, ym.I420)
    assert i420[1].shape == (5, 4) and np.array_equal(i420[1], nv12[1][:, 0::2]) and np.array_equal(i420[2], nv12[1][:, 1::2])
    assert np.array_equal(ym.yuv_to_bgr(i420, ym.I420, ym.BT601_FULL, 1, 2, 6, 7), want)
    # YV12 = I420 with the planes swapped = NV21 read as NV12
    assert np.array_equal(ym.yuv_to_bgr((i420[0], i420[2], i420[1]), ym.I420, ym.BT601_FULL, 1, 2, 6, 7),
                          ym.yuv_to_bgr(nv21, ym.NV12, ym.BT601_FULL, 1, 2, 6, 7))


# ---- 3. the staging guard, per plane --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("fmt", [ym.NV12, ym.I420])
def test_plane_extent_guard_for_chroma_rows(base, fmt):
    """A chroma plane that starts at any byte address inside memory it does not own: every row of it is staged complete, whole
    dwords are loaded only inside the plane's own extent, and no byte outside the extent is touched at all."""
    rng = np.random.default_rng(base)
    rows, cbytes, pitch = 5, (7 if fmt == ym.I420 else 14), 23
    plane = rng.integers(0, 256, (rows, cbytes), dtype=np.uint8)
    flat = ym.pad_plane(plane, pitch)
    extent = (rows - 1) * pitch + cbytes
    assert len(flat) == extent
    mem = np.full(base + extent + 8, 0xEE, np.uint8)
    mem[base:base + extent] = flat
    own = set(range(base, base + extent))
    straddled = 0
    for r in range(rows):
        staged, mis, whole, single = stage_row(mem, base, extent, r * pitch, cbytes)
        assert mis == (base + r * pitch) & 3
        assert np.array_equal(staged[mis:mis + cbytes], plane[r]), r
        assert whole <= own and single <= own and not (whole & single)
        assert (whole | single) >= set(range(base + r * pitch, base + r * pitch + cbytes))
        straddled += bool(single)
    assert straddled >= (1 if base % 4 else 0)       # an odd base makes the first row's first dword straddle the extent's start
    # a sub-rectangle of the plane (a crop: folded base inside the plane, shorter rows, same pitch) owns only ITS extent
    cbase, crows, cb2 = base + pitch + 3, 3, 6
    cext = (crows - 1) * pitch + cb2
    for r in range(crows):
        staged, mis, whole, single = stage_row(mem, cbase, cext, r * pitch, cb2)
        assert np.array_equal(staged[mis:mis + cb2], mem[cbase + r * pitch:cbase + r * pitch + cb2])
        assert (whole | single) <= set(range(cbase, cbase + cext))


# ---- 4. the LDS function and the width limit ----------------------------------------------------------------------------------
def test_lds_bytes_and_width_limit_against_the_restatement():
    from yolo_fastestv2_amd import yuv
    for W in (352, 64, 96, 640):
        for w in list(range(1, 70)) + [351, 352, 353, 1279, 1280, 1919, 1920, 1921, 3840, 27128, 40000]:
            assert yuv.resize_lds_bytes(w, W) == rm.lds_bytes(rm.U8, rm.YUV8, w, W), (w, W)
            if w > 1:
                assert yuv.resize_lds_bytes(w, W) >= yuv.resize_lds_bytes(w - 1, W)
        m = yuv.max_width(W)
        assert m == rm.max_width(rm.U8, rm.YUV8, W)
        assert rm.lds_bytes(rm.U8, rm.YUV8, m, W) <= rm.LDS_FULL < rm.lds_bytes(rm.U8, rm.YUV8, m + 1, W)
    assert yuv.max_width(352) == 40689
    assert yuv.resize_lds_bytes(1920, 352) == 8760                      # 18 workgroups of a 1080p batch per CU by LDS
    assert rm.lds_bytes(rm.U8, rm.BGR, 1920, 352) == 12584               # ... where the B, G, R kernel's rows take 12 584 bytes
    # what the slots must hold, for every width and misalignment: a luma row, an interleaved row in two half-slots, a planar row in one
    for w in range(1, 200):
        half = rm.slot((w >> 1) + 1, 4)
        for px in (0, 1):
            cw = ((w - 1 + px) >> 1) + 1
            for mis in range(4):
                assert ((mis + w + 3) >> 2) * 4 <= rm.slot(w, 4)
                assert ((mis + cw + 3) >> 2) * 4 <= half
                assert ((mis + 2 * cw + 3) >> 2) * 4 <= 2 * half


def test_binding_matches_the_header():
    """yfv2_frame_yuv's ctypes layout is the C struct's: 3 pointers, 2 int64, 6 int32 = 64 bytes, fields at the C offsets"""
    import ctypes as C
    from yolo_fastestv2_amd import _lib
    F = _lib.FrameYuv
    assert C.sizeof(F) == 64
    assert [getattr(F, n).offset for n in ("y", "u", "v", "pitch_y", "pitch_c", "x0", "y0", "width", "height", "format", "colour")] == [
        0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]
    from yolo_fastestv2_amd import yuv
    assert (yuv.FORMATS["nv12"], yuv.FORMATS["nv21"], yuv.FORMATS["i420"]) == (ym.NV12, ym.NV21, ym.I420)
    assert [yuv.COLOURS[k] for k in ("bt601", "bt709", "bt601_full", "bt709_full")] == list(ym.COLOURS)
