"""CPU-only checks of the 10-bit YUV front door (include/yfv2.h YFV2_YUV_P010 / YFV2_YUV_I010): the colour table
against its formulas, the int32 range, known triplets, the distance to the 8-bit rule, the ignored bits, the LDS / width limit of
the two-byte row kernels (yfv2_debug_rows16) against tests/rows_model.py, and yuv.frame_table on 16-bit and byte planes.
The device side is tests/test_gpu_yuv16.py."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import rows_model as rm
import yuv_model as ym
from conftest import REPO
from rows_checks import _rows, check_export, check_lds_bytes_and_limit

FULL = rm.LDS_FULL
LIMITED = (ym.BT601_LIMITED, ym.BT709_LIMITED)
FORMATS = ym.FORMATS16


def _rows16(kind, w, W):
    return _rows(kind, rm.YUV16, w, W)


def _convert(Y, U, V, colour):
    return ym.convert(Y, U, V, colour, bits=10)


# ---- 1. the colour rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", ym.COLOURS)
def test_table_literals_are_the_formulas(colour):
    assert ym.COEF[10][colour] == ym.coefficients(colour)
    header = open(os.path.join(REPO, "include", "yfv2.h")).read()
    name = ("YFV2_BT601_LIMITED", "YFV2_BT709_LIMITED", "YFV2_BT601_FULL", "YFV2_BT709_FULL")[colour]
    assert re.search(name + r"\s+" + r"\s+".join(str(k) for k in ym.COEF[10][colour]) + r"\b", header), "the header states another row for " + name


@pytest.mark.parametrize("colour", ym.COLOURS)
def test_accumulators_fit_int32(colour):
    """each accumulator is affine in max(Y - off, 0), U and V, so its extremes over the 10-bit cube are at the 8 corners; 2^22 random
    triples must lie inside them.  Every factor is below 2^24 (the kernel multiplies with 24-bit multiplies)."""
    corners = np.array(list(itertools.product((0, 1023), repeat=3)))
    acc = np.stack(ym.accumulators(corners[:, 0], corners[:, 1], corners[:, 2], colour, bits=10))
    lo, hi = int(acc.min()), int(acc.max())
    assert -2.83e8 <= lo and hi <= 5.77e8 and hi < 2 ** 31 - 1 and lo > -2 ** 31, (lo, hi)
    rng = np.random.default_rng(40 + colour)
    Y, U, V = rng.integers(0, 1024, (3, 1 << 22))
    rnd = np.stack(ym.accumulators(Y, U, V, colour, bits=10))
    assert lo <= int(rnd.min()) and int(rnd.max()) <= hi
    assert all(abs(k) < 1 << 24 for k in ym.COEF[10][colour][1:]) and 1023 < 1 << 24


@pytest.mark.parametrize("colour", ym.COLOURS)
def test_known_triplets_and_clamps(colour):
    limited = colour in LIMITED
    black, white = (64, 940) if limited else (0, 1023)
    assert _convert(black, 512, 512, colour).tolist() == [0, 0, 0]
    assert _convert(white, 512, 512, colour).tolist() == [255, 255, 255]
    # mid-grey by hand: limited (502 - 64) * 255 / 876 = 127.5 exactly in the reals, 127 with this CY (a hair below the real
    # coefficient); full 512 * 255 / 1023 = 127.62...
    want = (((502 - 64) * 305236 + (1 << 19)) >> 20) if limited else ((512 * 261375 + (1 << 19)) >> 20)
    assert want in (127, 128) and _convert(502 if limited else 512, 512, 512, colour).tolist() == [want] * 3
    g = _convert(np.arange(1024), 512, 512, colour)
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 1], g[:, 2]) and np.all(np.diff(g[:, 0].astype(int)) >= 0)
    assert set(np.unique(g[:, 0])) == set(range(256))                  # every 8-bit level is reached
    if limited:   # below black and above white: the luma floor and the upper clamp
        assert _convert(0, 512, 512, colour).tolist() == [0, 0, 0] and _convert(1023, 512, 512, colour).tolist() == [255, 255, 255]
    assert _convert(white, 512, 1023, colour)[2] == 255 and _convert(black, 512, 0, colour)[2] == 0
    assert _convert(white, 1023, 512, colour)[0] == 255 and _convert(black, 0, 512, colour)[0] == 0
    assert _convert(white, 0, 0, colour)[1] == 255 and _convert(black, 1023, 1023, colour)[1] == 0
    r, _, b = ym.accumulators(white, 1023, 1023, colour, bits=10)
    assert (r >> ym.SHIFT) > 255 and (b >> ym.SHIFT) > 255
    r, _, b = ym.accumulators(black, 0, 0, colour, bits=10)
    assert (r >> ym.SHIFT) < 0 and (b >> ym.SHIFT) < 0


def test_one_value_by_hand():
    """Y 400, U 400, V 800 under BT.601 limited: yy = 336 * 305236 + 524288 = 103083584, u = -112, v = 288"""
    yy = 336 * 305236 + 524288
    assert yy == 103083584
    assert _convert(400, 400, 800, ym.BT601_LIMITED).tolist() == [
        (yy + 528805 * -112) >> 20, (yy + -213115 * 288 + -102698 * -112) >> 20, (yy + 418389 * 288) >> 20]
    # rounded once from 10-bit precision: two 10-bit greys inside one 8-bit code give different outputs somewhere
    g = _convert(np.arange(1024), 512, 512, ym.BT601_FULL)[:, 0].astype(int)
    assert any(g[4 * k] != g[4 * k + 3] for k in range(256))


@pytest.mark.parametrize("colour", LIMITED)
def test_ten_bit_rule_on_four_times_the_samples_is_within_one_of_the_eight_bit_rule(colour):
    """all 2^24 8-bit (Y, U, V): the 10-bit rule on 4 Y, 4 U, 4 V against the 8-bit rule of tests/yuv_model.py - at most 1 apart in
    any channel, and 1 somewhere (BT.601: the 8-bit row is cv2's rounded decimals, 3.4 % of the outputs differ; BT.709: 0.007 %)."""
    U = np.arange(256)[None, :, None]
    V = np.arange(256)[None, None, :]
    worst, differ = 0, 0
    for y in range(0, 256, 8):
        Y = np.arange(y, y + 8)[:, None, None]
        Yb, Ub, Vb = np.broadcast_arrays(Y, U, V)
        d = np.abs(_convert(4 * Yb, 4 * Ub, 4 * Vb, colour).astype(np.int16) - ym.convert(Yb, Ub, Vb, colour).astype(np.int16))
        worst, differ = max(worst, int(d.max())), differ + int(np.count_nonzero(d))
    share = differ / (3 * 2.0 ** 24)
    print("colour %d: max |difference| %d, %.4f %% of the outputs differ" % (colour, worst, 100 * share))
    assert worst == 1
    assert (0.03 < share < 0.04) if colour == ym.BT601_LIMITED else (0 < share < 0.001)


# ---- 2. the ignored bits, and the two formats ---------------------------------------------------------------------------------
def test_ignored_bits_do_not_matter_and_the_formats_are_one_picture():
    rng = np.random.default_rng(17)
    clean = ym.random_planes(rng, 9, 7, ym.P010, junk=False)
    want = ym.yuv_to_bgr(clean, ym.P010, ym.BT709_LIMITED, 1, 2, 6, 7)
    assert len(np.unique(want)) > 50
    values = [ym.sample_values(p, ym.P010) for p in clean]
    for fmt in FORMATS:
        base = ym.to_format(clean, fmt)
        assert np.array_equal(ym.yuv_to_bgr(base, fmt, ym.BT709_LIMITED, 1, 2, 6, 7), want), fmt
        for junk in (63, 21, None):
            dirty = tuple(ym.pack(ym.sample_values(p, fmt), fmt, rng.integers(0, 64, p.shape) if junk is None else junk) for p in base)
            assert any(np.any(d != b) for d, b in zip(dirty, base))
            assert all(np.array_equal(ym.sample_values(d, fmt), ym.sample_values(b, fmt)) for d, b in zip(dirty, base))
            assert np.array_equal(ym.yuv_to_bgr(dirty, fmt, ym.BT709_LIMITED, 1, 2, 6, 7), want), (fmt, junk)
    i010 = ym.to_format(clean, ym.I010)
    assert i010[1].shape == (5, 4) and np.array_equal(ym.sample_values(i010[1], ym.I010), values[1][:, 0::2])
    assert np.array_equal(ym.sample_values(i010[2], ym.I010), values[1][:, 1::2])
    # the value of a word: the high 10 bits of P010, the low 10 of I010
    assert ym.sample_values(np.array([0xFFC0, 0x003F, 0x8000 | 63], np.uint16), ym.P010).tolist() == [1023, 0, 512]
    assert ym.sample_values(np.array([0x03FF, 0xFC00, 0xFC00 | 512], np.uint16), ym.I010).tolist() == [1023, 0, 512]


# ---- 3. the LDS function and the width limit --------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_checks_its_arguments():
    from yolo_fastestv2_amd import yuv
    check_export("yfv2_debug_rows16", (), yuv.rows_lds16)
    assert re.search(r"YFV2_YUV_P010 = 16, YFV2_YUV_I010 = 17", open(os.path.join(REPO, "include", "yfv2.h")).read())
    with pytest.raises(ValueError):
        yuv.max_width(352, bits=12)


@pytest.mark.parametrize("kind", rm.KINDS, ids=rm.KIND_IDS)
def test_lds_bytes_and_limit_equal_the_model(kind):
    check_lds_bytes_and_limit(kind, rm.YUV16)


def test_pinned_values_and_package_functions():
    from yolo_fastestv2_amd import datasets as ds, yuv
    assert yuv.max_width(352, bits=10) == _rows16(rm.U8, 1, 352)[1] == rm.max_width(rm.U8, rm.YUV16, 352) == 20343
    assert yuv.max_width(352) == yuv.max_width(352, 8) == 40689                # about twice
    assert _rows16(rm.U8, 1920, 352)[0] == 2 * 3844 + 4 * 1928 + 1056 == 16456   # 9 workgroups of a 1080p batch per CU by LDS
    assert FULL // 16456 == 9
    for W in (32, 64, 352, 640):
        assert ds.max_frame_width(W, True, bits=10) == _rows16(rm.TRAIN, 1, W)[1] <= ds.max_frame_width(W, True)
        assert ds.train_batch_lds_bytes(1920, W, True, bits=10) == _rows16(rm.TRAIN, 1920, W)[0]
        assert yuv.rows_lds16(yuv.ROWS_TENSOR_F16, 351, W) == _rows16(rm.TENSOR_F16, 351, W)
    with pytest.raises(ValueError):
        ds.max_frame_width(352, False, bits=10)


def test_slots_hold_what_the_staging_writes():
    """for every width 1..199, misalignment 0 or 2 (the planes are 2-byte aligned, the pitches even) and origin parity: the dwords a
    row's staging writes fit its slot, at either alignment - a luma row, an interleaved row in two half-slots, a planar row in one"""
    for a in (4, 16):
        for w in range(1, 200):
            half = rm.slot(2 * (w // 2 + 1), a)
            for mis in (0, 2):
                assert ((mis + 2 * w + 3) >> 2) * 4 <= rm.slot(2 * w, a)
                for px in (0, 1):
                    cw = ((w - 1 + px) >> 1) + 1
                    assert ((mis + 2 * cw + 3) >> 2) * 4 <= half and ((mis + 4 * cw + 3) >> 2) * 4 <= 2 * half


# ---- 4. yuv.frame_table ---------------------------------------------------------------------------------------------------------
def _t16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16))


def test_frame_table_takes_word_and_byte_planes():
    from yolo_fastestv2_amd import yuv
    cpu = torch.device("cpu")
    rng = np.random.default_rng(31)
    assert yuv.FORMATS["p010"] == yuv.FORMATS[16] == ym.P010 and yuv.FORMATS["i010"] == yuv.FORMATS["yuv420p10le"] == yuv.FORMATS["yuv420p10"] == yuv.FORMATS[17] == ym.I010
    y, uv = (_t16(p) for p in ym.random_planes(rng, 10, 14, ym.P010))
    arr, frames = yuv.frame_table([yuv.YuvFrame((y, uv), "p010", "bt709")], cpu)
    a = arr[0]
    assert (a.format, a.colour, a.width, a.height, a.pitch_y, a.pitch_c) == (16, 1, 14, 10, 28, 28) and a.y == y.data_ptr() and a.u == uv.data_ptr()
    # uv as (rows, samples, 2); a padded luma plane; a crop
    big = torch.zeros((10, 20), dtype=torch.int16)
    a = yuv.frame_table([yuv.YuvFrame((big[:, :15], uv.view(5, 7, 2)), "p010", x0=1, y0=2, width=13, height=8)], cpu)[0][0]
    assert (a.pitch_y, a.pitch_c, a.x0, a.y0, a.width, a.height) == (40, 28, 1, 2, 13, 8)
    if hasattr(torch, "uint16"):
        a = yuv.frame_table([yuv.YuvFrame((y.view(torch.uint16), uv.view(torch.uint16)), 16)], cpu)[0][0]
        assert (a.pitch_y, a.pitch_c, a.width) == (28, 28, 14)
    # the bytes: pitch = stride(0); the rectangle must be stated
    yb, uvb = y.view(torch.uint8), uv.view(torch.uint8)
    assert tuple(yb.shape) == (10, 28)
    a = yuv.frame_table([yuv.YuvFrame((yb, uvb), "p010", width=14, height=10)], cpu)[0][0]
    assert (a.pitch_y, a.pitch_c, a.width, a.height, a.y) == (28, 28, 14, 10, y.data_ptr())
    with pytest.raises(ValueError, match="width and height"):
        yuv.YuvFrame((yb, uvb), "p010")
    # I010: three planes, one chroma pitch
    yi, ui, vi = (_t16(p) for p in ym.random_planes(rng, 9, 7, ym.I010))
    a = yuv.frame_table([yuv.YuvFrame((yi, ui, vi), "yuv420p10le", "jpeg")], cpu)[0][0]
    assert (a.format, a.colour, a.pitch_y, a.pitch_c, a.v) == (17, 2, 14, 8, vi.data_ptr())
    # refused: short planes (rows and samples count twice the bytes), wrong plane counts and types, a mix of sample widths
    y8, uv8 = torch.zeros((10, 14), dtype=torch.uint8), torch.zeros((5, 14), dtype=torch.uint8)
    for bad in (yuv.YuvFrame((y, uv), "p010", width=15), yuv.YuvFrame((y, uv), "p010", y0=1, height=10), yuv.YuvFrame((y, uv[:, :13]), "p010"),
                yuv.YuvFrame((y, uv[:4]), "p010"), yuv.YuvFrame((yb, uvb), "p010", width=15, height=10), yuv.YuvFrame((yb[:, :27], uvb), "p010", width=14, height=10),
                yuv.YuvFrame((y, uv), "i010"), yuv.YuvFrame((yi, ui), "i010"), yuv.YuvFrame((yi, ui, vi[:, :3]), "i010"), yuv.YuvFrame((y, uv.float()), "p010"),
                yuv.YuvFrame((y, uv.int()), "p010"), yuv.YuvFrame((y, uv), "nv12"), yuv.YuvFrame((y[:, ::2], uv), "p010")):
        with pytest.raises(ValueError):
            yuv.frame_table([bad], cpu)
    with pytest.raises(ValueError, match="frame 1"):
        yuv.frame_table([yuv.YuvFrame((y, uv), "p010"), yuv.YuvFrame((y8, uv8), "nv12")], cpu)
    with pytest.raises(ValueError, match="frame 2"):
        yuv.frame_table([yuv.YuvFrame((y8, uv8), "nv12"), yuv.YuvFrame((y8, uv8), "nv21"), yuv.YuvFrame((yi, ui, vi), "i010")], cpu)
    assert len(yuv.frame_table([yuv.YuvFrame((y, uv), "p010"), yuv.YuvFrame((yi, ui, vi), "i010")], cpu)[0]) == 2      # one width: accepted
