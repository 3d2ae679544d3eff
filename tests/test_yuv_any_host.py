"""CPU-only checks of the 8-bit YUV samplings beyond 4:2:0 (include/yfv2.h YFV2_YUV_I422 .. YFV2_YUV_GREY): the
model's addressing against offsets worked out by hand (all eleven formats of tests/yuv_model.py, from one body), grey, the three
forms of one 4:2:2 picture, the model against bytes recorded before its three predecessors were folded, the general launch's LDS and width limit (yfv2_debug_rows_any) against tests/rows_model.py, yuv.frame_table
on the new plane shapes and on mixed lists, and the host-side sanitizer program tests/cpp/yfv2_yuv_any_san.cpp.
The argument checks of the C ABI need a handle, and a handle needs a device: they are in tests/test_gpu_yuv_any.py
(test_argument_errors_launch_nothing).  The device side is that file."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rows_model as rm
import yuv_model as ym
from conftest import REPO
from rows_checks import _rows, check_export, check_lds_bytes_and_limit

FULL = rm.LDS_FULL
FORMATS = ym.FORMATS8


def _rows_any(kind, w, W):
    return _rows(kind, rm.YUV8_ANY, w, W)


# ---- 1. the addressing -----------------------------------------------------------------------------------------------------------
def _by_hand(fmt, R, C):
    """(luma, U, V) sample positions of pixel (R, C) as (plane, row, sample), written out per format from include/yfv2.h's table"""
    if fmt in (ym.NV12, ym.P010):
        return (0, R, C), (1, R // 2, 2 * (C // 2)), (1, R // 2, 2 * (C // 2) + 1)
    if fmt == ym.NV21:
        return (0, R, C), (1, R // 2, 2 * (C // 2) + 1), (1, R // 2, 2 * (C // 2))
    if fmt in (ym.I420, ym.I010):
        return (0, R, C), (1, R // 2, C // 2), (2, R // 2, C // 2)
    if fmt == ym.I422:
        return (0, R, C), (1, R, C // 2), (2, R, C // 2)
    if fmt == ym.I440:
        return (0, R, C), (1, R // 2, C), (2, R // 2, C)
    if fmt == ym.I444:
        return (0, R, C), (1, R, C), (2, R, C)
    if fmt == ym.YUYV:
        return (0, R, 2 * C), (0, R, 4 * (C // 2) + 1), (0, R, 4 * (C // 2) + 3)
    if fmt == ym.UYVY:
        return (0, R, 2 * C + 1), (0, R, 4 * (C // 2)), (0, R, 4 * (C // 2) + 2)
    return (0, R, C), None, None


@pytest.mark.parametrize("fmt", ym.FORMATS, ids=[ym.NAMES[f] for f in ym.FORMATS])
def test_chroma_addressing_every_parity(fmt):
    """frames at every origin parity inside 11 x 13 planes - one pixel up to the whole plane, its last pixel, ending on its last row
    and column - each pixel is the conversion of the three samples at the hand-computed offsets; the planes hold random samples, so
    a wrong offset shows"""
    bits, mid = ym.TABLE[fmt].bits, 1 << (ym.TABLE[fmt].bits - 1)
    rng = np.random.default_rng(7 + fmt)
    assert ym.plane_shapes(6, 7, fmt) == {ym.NV12: [(6, 7), (3, 8)], ym.NV21: [(6, 7), (3, 8)], ym.I420: [(6, 7), (3, 4), (3, 4)], ym.I422: [(6, 7), (6, 4), (6, 4)],
                                          ym.I440: [(6, 7), (3, 7), (3, 7)], ym.I444: [(6, 7), (6, 7), (6, 7)], ym.YUYV: [(6, 16)], ym.UYVY: [(6, 16)], ym.GREY: [(6, 7)],
                                          ym.P010: [(6, 7), (3, 8)], ym.I010: [(6, 7), (3, 4), (3, 4)]}[fmt]
    planes = ym.random_planes(rng, 11, 13, fmt)
    assert [p.shape for p in planes] == ym.plane_shapes(11, 13, fmt) and all(p.dtype == (np.uint8 if bits == 8 else np.uint16) for p in planes)
    val = [ym.sample_values(p, fmt) for p in planes] if bits == 10 else planes
    cases = [(x0, y0, w, h) for x0 in (0, 1, 2, 3) for y0 in (0, 1, 2) for w, h in ((1, 1), (2, 2), (3, 5), (4, 3), (5, 4), (7, 6))]
    cases += [(0, 0, 13, 11), (12, 10, 1, 1), (5, 4, 8, 7), (6, 5, 7, 6)]          # the whole plane; its last pixel; ending on the last row and column
    for x0, y0, w, h in cases:
        got = ym.yuv_to_bgr(planes, fmt, ym.BT601_FULL, x0, y0, w, h)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        for r in range(h):
            for c in range(w):
                ly, lu, lv = _by_hand(fmt, y0 + r, x0 + c)
                u, v = (mid, mid) if lu is None else (val[lu[0]][lu[1], lu[2]], val[lv[0]][lv[1], lv[2]])
                assert got[r, c].tolist() == ym.convert(val[ly[0]][ly[1], ly[2]], u, v, ym.BT601_FULL, bits).tolist(), (x0, y0, r, c)
    # two offsets by hand, numbers only: pixel (3, 3) of a YUYV row is luma byte 6, U byte 5, V byte 7; of a UYVY row 7, 4, 6
    assert ym.offsets(ym.YUYV, 3, 3) == ((0, 3, 6), (0, 3, 5), (0, 3, 7)) and ym.offsets(ym.UYVY, 3, 3) == ((0, 3, 7), (0, 3, 4), (0, 3, 6))
    assert ym.offsets(ym.I440, 3, 3) == ((0, 3, 3), (1, 1, 3), (2, 1, 3)) and ym.offsets(ym.I422, 3, 3) == ((0, 3, 3), (1, 3, 1), (2, 3, 1))


def test_grey_is_i444_with_neutral_chroma_and_full_range_grey_is_identity():
    rng = np.random.default_rng(11)
    y = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    neutral = np.full_like(y, 128)
    for colour in ym.COLOURS:
        for x0, y0, w, h in ((0, 0, 13, 9), (1, 2, 11, 6), (12, 8, 1, 1)):
            assert np.array_equal(ym.yuv_to_bgr((y,), ym.GREY, colour, x0, y0, w, h), ym.yuv_to_bgr((y, neutral, neutral), ym.I444, colour, x0, y0, w, h))
    ramp = np.arange(256, dtype=np.uint8)[None, :]
    got = ym.yuv_to_bgr((ramp,), ym.GREY, ym.BT601_FULL, 0, 0, 256, 1)
    assert np.array_equal(got, np.repeat(ramp[0][:, None], 3, axis=1)[None])             # B = G = R = Y for all 256 values
    assert np.array_equal(ym.yuv_to_bgr((ramp,), ym.GREY, ym.BT709_FULL, 0, 0, 256, 1), got)


def test_one_picture_in_three_422_forms_and_the_other_subsamplings():
    """an I444 picture subsampled by taking the even samples: YUYV, UYVY and I422 of it are ONE picture; every format agrees with
    the I444 picture at the pixels whose own chroma sample was taken (even column / row on the subsampled axes)"""
    rng = np.random.default_rng(13)
    for rows, cols in ((8, 10), (7, 9)):
        src = ym.random_planes(rng, rows, cols, ym.I444)
        full = ym.yuv_to_bgr(src, ym.I444, ym.BT601_FULL, 0, 0, cols, rows)
        want = ym.yuv_to_bgr(ym.from_i444(src, ym.I422), ym.I422, ym.BT601_FULL, 0, 0, cols, rows)
        for fmt in (ym.YUYV, ym.UYVY):
            for x0, y0, w, h in ((0, 0, cols, rows), (1, 1, cols - 1, rows - 1), (3, 2, 4, 3)):
                got = ym.yuv_to_bgr(ym.from_i444(src, fmt), fmt, ym.BT601_FULL, x0, y0, w, h)
                assert np.array_equal(got, want[y0:y0 + h, x0:x0 + w]), (fmt, x0, y0)
        for fmt in FORMATS:
            if fmt == ym.GREY:
                continue
            sx, sy = ym.SHIFTS[fmt]
            got = ym.yuv_to_bgr(ym.from_i444(src, fmt), fmt, ym.BT601_FULL, 0, 0, cols, rows)
            assert np.array_equal(got[::1 << sy, ::1 << sx], full[::1 << sy, ::1 << sx]), fmt
            assert (fmt == ym.I444) == np.array_equal(got, full)
        assert np.array_equal(ym.from_i444(src, ym.GREY)[0], src[0])


@pytest.mark.parametrize("fmt", ym.FORMATS, ids=[ym.NAMES[f] for f in ym.FORMATS])
def test_the_model_reproduces_the_recorded_bytes(fmt):
    """tests/golden/yuv_model_bgr.npz: yuv_to_bgr of one seeded 9 x 7 picture per format, the 5 x 5 frame at the odd origin (3, 1),
    under each colour - recorded with the three per-family models this file replaced (the 4:2:0 formats: two of them agreed).
    The one model returns those bytes."""
    gold = np.load(os.path.join(REPO, "tests", "golden", "yuv_model_bgr.npz"))
    x0, y0, w, h = (int(v) for v in gold["rect"])
    assert (x0, y0, w, h) == (3, 1, 5, 5)
    planes = tuple(gold["f%d_plane%d" % (fmt, k)] for k in range(ym.TABLE[fmt].planes))
    assert [p.shape for p in planes] == ym.plane_shapes(7, 9, fmt)
    for colour in ym.COLOURS:
        got = ym.yuv_to_bgr(planes, fmt, colour, x0, y0, w, h)
        assert got.dtype == np.uint8 and np.array_equal(got, gold["f%d_c%d" % (fmt, colour)]), (fmt, colour)


# ---- 2. the general launch's LDS and width limit --------------------------------------------------------------------------------
def test_export_is_declared_bound_and_checks_its_arguments():
    from yolo_fastestv2_amd import yuv
    check_export("yfv2_debug_rows_any", (), yuv.rows_lds_any)
    header = open(os.path.join(REPO, "include", "yfv2.h")).read()
    assert re.search(r"YFV2_YUV_I422 = 3, YFV2_YUV_I440 = 4, YFV2_YUV_I444 = 5, YFV2_YUV_YUYV = 6, YFV2_YUV_UYVY = 7, YFV2_YUV_GREY = 8", header)
    with pytest.raises(ValueError):
        yuv.max_width(352, bits=10, general=True)


@pytest.mark.parametrize("kind", rm.KINDS, ids=rm.KIND_IDS)
def test_lds_bytes_and_limit_equal_the_model(kind):
    check_lds_bytes_and_limit(kind, rm.YUV8_ANY)


def test_layout_holds_a_packed_row_and_a_full_width_chroma_row():
    """what the staging writes - the dwords that cover a row at head misalignment 0..3 - fits where the layout puts it: a luma or a
    4:4:4 chroma row of w bytes in ONE slot, an interleaved row of at most w + 2 bytes in two, a packed row of 2 w + 4 in three"""
    for a in (4, 16):
        for w in range(1, 600):
            s = rm.slot(w, a)
            for mis in range(4):
                assert ((mis + w + 3) >> 2) * 4 <= s
                assert ((mis + 2 * w + 4 + 3) >> 2) * 4 <= 3 * s
                for px in (0, 1):
                    cw = ((w - 1 + px) >> 1) + 1
                    assert 4 * cw <= 2 * w + 4 and ((mis + 2 * cw + 3) >> 2) * 4 <= 2 * s


def test_pinned_values_and_package_functions():
    from yolo_fastestv2_amd import datasets as ds, yuv
    general = yuv.max_width(352, general=True)
    assert general == _rows_any(rm.U8, 1, 352)[1] == rm.max_width(rm.U8, rm.YUV8_ANY, 352) == 27125 < yuv.max_width(352) == 40689
    assert _rows_any(rm.U8, 1920, 352)[0] == 6 * 1924 + 1056 == 12600 and FULL // 12600 == 13      # workgroups of a 1080p batch per CU by LDS
    assert ds.max_frame_width(352, True, general=True) == _rows_any(rm.TRAIN, 1, 352)[1] == 26429
    for W in (32, 64, 352, 640):
        assert ds.max_frame_width(W, True, general=True) == _rows_any(rm.TRAIN, 1, W)[1] <= ds.max_frame_width(W, True)
        assert ds.train_batch_lds_bytes(1920, W, True, general=True) == _rows_any(rm.TRAIN, 1920, W)[0]
        assert yuv.rows_lds_any(yuv.ROWS_TENSOR_F16, 351, W) == _rows_any(rm.TENSOR_F16, 351, W)
    with pytest.raises(ValueError):
        ds.max_frame_width(352, False, general=True)
    header = open(os.path.join(REPO, "include", "yfv2.h")).read()
    assert "27 125 pixels at cfg.width 352" in header and "26 429 against 39 641" in header       # the figures the code computes


# ---- 3. yuv.frame_table -----------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_frame_table_takes_the_new_formats():
    from yolo_fastestv2_amd import yuv
    cpu = torch.device("cpu")
    rng = np.random.default_rng(31)
    for name, value in (("i444", 5), ("yuv444p", 5), ("i422", 3), ("yuv422p", 3), ("i440", 4), ("yuv440p", 4), ("yuyv", 6), ("yuy2", 6), ("yuyv422", 6),
                        ("uyvy", 7), ("uyvy422", 7), ("grey", 8), ("gray", 8), ("y800", 8)):
        assert yuv.FORMATS[name] == yuv.FORMATS[value] == value
    # planar: three planes, one chroma pitch, default size from the luma plane
    for fmt in (ym.I422, ym.I440, ym.I444):
        y, u, v = (_t(p) for p in ym.random_planes(rng, 9, 13, fmt))
        a = yuv.frame_table([yuv.YuvFrame((y, u, v), ym.NAMES[fmt], "jpeg")], cpu)[0][0]
        assert (a.format, a.colour, a.width, a.height, a.pitch_y, a.pitch_c) == (fmt, 2, 13, 9, 13, u.shape[1])
        assert (a.y, a.u, a.v) == (y.data_ptr(), u.data_ptr(), v.data_ptr())
        for bad in (yuv.YuvFrame((y, u), ym.NAMES[fmt]), yuv.YuvFrame((y, u, v[:, :-1]), ym.NAMES[fmt]), yuv.YuvFrame((y, u[:-1], v), ym.NAMES[fmt]),
                    yuv.YuvFrame((y[:, :-1], u, v), ym.NAMES[fmt], width=13)):
            with pytest.raises(ValueError, match="frame 0"):
                yuv.frame_table([bad], cpu)
    # packed: ONE plane, 2-D bytes or (rows, pixels, 2); width = bytes // 2 - x0 or pixels - x0
    for fmt in (ym.YUYV, ym.UYVY):
        p = _t(ym.random_planes(rng, 9, 14, fmt)[0])
        assert tuple(p.shape) == (9, 28)
        for planes in ((p,), p, (p.view(9, 14, 2),)):
            f = yuv.YuvFrame(planes, ym.NAMES[fmt], "bt709")
            a = yuv.frame_table([f], cpu)[0][0]
            assert (f.width, f.height) == (14, 9) and (a.format, a.width, a.height, a.pitch_y, a.y) == (fmt, 14, 9, 28, p.data_ptr()) and not a.u and not a.v
        f = yuv.YuvFrame(p.view(9, 14, 2), ym.NAMES[fmt], x0=3, y0=2)
        assert (f.width, f.height) == (11, 7) and yuv.YuvFrame(p, ym.NAMES[fmt], x0=3, y0=2).width == 11
        c = yuv.YuvFrame(p, ym.NAMES[fmt]).crop(3, 1, 5, 4)          # an odd origin: the middle of a macropixel
        a = yuv.frame_table([c], cpu)[0][0]
        assert (a.x0, a.y0, a.width, a.height) == (3, 1, 5, 4)
        # an odd last pixel reads its whole macropixel: 13 pixels need 28 bytes, and a plane one byte short of that is refused
        odd = yuv.YuvFrame(p, ym.NAMES[fmt], width=13)
        assert yuv.frame_table([odd], cpu)[0][0].width == 13
        with pytest.raises(ValueError, match=r"frame 1: plane packed"):
            yuv.frame_table([odd, yuv.YuvFrame(p[:, :27], ym.NAMES[fmt], width=13)], cpu)
        with pytest.raises(ValueError, match="frame 0"):
            yuv.frame_table([yuv.YuvFrame(p[:8], ym.NAMES[fmt], height=9)], cpu)
        with pytest.raises(ValueError, match="1 plane"):
            yuv.frame_table([yuv.YuvFrame((p, p), ym.NAMES[fmt])], cpu)
    # grey: one plane
    g = _t(ym.random_planes(rng, 9, 13, ym.GREY)[0])
    a = yuv.frame_table([yuv.YuvFrame(g, "gray", "jpeg", x0=1)], cpu)[0][0]
    assert (a.format, a.width, a.height, a.pitch_y, a.y, a.x0) == (8, 12, 9, 13, g.data_ptr(), 1) and not a.u
    with pytest.raises(ValueError, match=r"frame 0: plane y"):
        yuv.frame_table([yuv.YuvFrame((g[:, :12],), "grey", width=13)], cpu)
    with pytest.raises(ValueError):
        yuv.YuvFrame((g,), "yuv411p")


def test_frame_table_takes_mixed_8_bit_lists_and_refuses_10_bit_among_them():
    from yolo_fastestv2_amd import yuv
    cpu = torch.device("cpu")
    rng = np.random.default_rng(37)
    mk = lambda fmt, rows, cols: yuv.YuvFrame(tuple(_t(p) for p in ym.random_planes(rng, rows, cols, fmt)), ym.NAMES[fmt], "jpeg")
    frames = [mk(ym.NV12, 10, 14), mk(ym.I444, 9, 13), mk(ym.YUYV, 7, 6), mk(ym.GREY, 3, 4)]
    arr, out = yuv.frame_table(frames, cpu)
    assert [a.format for a in arr] == [0, 5, 6, 8] and [(a.width, a.height) for a in arr] == [(14, 10), (13, 9), (6, 7), (4, 3)] and len(out) == 4
    p010 = yuv.YuvFrame((torch.zeros((4, 6), dtype=torch.int16), torch.zeros((2, 6), dtype=torch.int16)), "p010")
    with pytest.raises(ValueError, match="frame 1"):
        yuv.frame_table([frames[1], p010], cpu)
    with pytest.raises(ValueError, match="frame 1"):
        yuv.frame_table([p010, frames[1]], cpu)


# ---- 4. the sanitizer program -----------------------------------------------------------------------------------------------------
def test_rows_and_fold_under_sanitizers():
    """tests/cpp/yfv2_yuv_any_san.cpp: its own main, the API units and the host instance of yfv2_yuv_move built with AddressSanitizer
    and UBSan (host side only), run as a program with nothing preloaded.  It sweeps yfv2_debug_rows_any and folds origins 0..3 x
    0..3 for every format, comparing the moved pointers and parities with the offsets of include/yfv2.h's table.  Sanitized code
    belongs on CPU machines: where a device is visible the test has nothing to do."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: not built or run where a GPU is visible")
    from yolo_fastestv2_amd import _lib
    _lib.lib()      # (the kernel objects the program links come from the library's build)
    csrc = os.path.join(REPO, "yolo_fastestv2_amd", "csrc")
    made = subprocess.run(["make", "-C", csrc, "yuv_any_san", "-j8"], capture_output=True, text=True)
    assert made.returncode == 0, made.stdout[-3000:] + made.stderr[-3000:]
    run = subprocess.run([os.path.join(REPO, "tests", "cpp", "yfv2_yuv_any_san")], capture_output=True, text=True)
    assert run.returncode == 0 and "yuv_any_san ok" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-6000:]
