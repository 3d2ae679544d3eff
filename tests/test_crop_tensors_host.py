"""CPU-only checks of crops as network input (include/yfv2.h yfv2_crop_letterbox, yfv2_crop_tensor_value, yfv2_crop_tensors_u8 /
_yuv):
  * yfv2_crop_tensor_value - the host entry point over the very function the kernels' epilogue calls - equals the numpy statement
    (tests/crop_tensors_model.py) bit for bit over all 256 bytes, fp32 and binary16, overflow and subnormal results included
  * yfv2_crop_letterbox likewise over every small rectangle at four output sizes and on the extreme aspect ratios
  * argument errors that need no device, and the binding
"""
import ctypes as C
import os

import numpy as np
import pytest

import crop_tensors_model as model

INF, NAN = float("inf"), float("nan")


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _c_value(m, a, mean, std):
    f, u = C.c_float(-77.0), C.c_uint16(0x7777)
    assert m.lib().yfv2_crop_tensor_value(a, mean, std, C.byref(f), C.byref(u)) == 0, m.last_error()
    return np.float32(f.value), np.uint16(u.value)


def _c_letterbox(m, cw, ch, H, W, lb):
    r = (C.c_int32 * 4)(-77, -77, -77, -77)
    assert m.lib().yfv2_crop_letterbox(cw, ch, H, W, lb, r) == 0, m.last_error()
    return tuple(r)


IMAGENET = [(0.485, 0.229), (0.456, 0.224), (0.406, 0.225)]
# (mean, std): plain / 255; ImageNet's three; (0.5, 0.5); a std so small that binary16 overflows (255 / 255 / 1e-6 = 1e6 > 65504);
# a mean next to 1 / 255 and a std that bring byte 1 to about 4e-6, a binary16 subnormal, and byte 0 to a negative normal
PAIRS = [(0.0, 1.0)] + IMAGENET + [(0.5, 0.5), (0.0, 1e-6), (0.0039, 5.0), (0.0, 3e38)]


@pytest.mark.parametrize("mean,std", PAIRS)
def test_value_equals_the_numpy_model_over_all_bytes(mean, std):
    m = _lib()
    a = np.arange(256)
    want32 = model.value(a, np.float32(mean), np.float32(std))
    want16 = model.to_dtype(want32, True)
    got = [_c_value(m, int(k), mean, std) for k in a]
    got32 = np.array([g[0] for g in got], np.float32)
    got16 = np.array([g[1] for g in got], np.uint16)
    assert np.array_equal(model.bits(got32), model.bits(want32)), (mean, std)
    assert np.array_equal(got16, model.bits(want16)), (mean, std)


def test_value_special_results_are_what_the_cases_claim():
    """the overflow pair gives binary16 infinities, the subnormal pairs subnormals - in binary16 and in fp32 - and plain / 255
    is torch's .float() / 255"""
    m = _lib()
    f, u = _c_value(m, 255, 0.0, 1e-6)
    assert np.isfinite(f) and u == 0x7C00
    f, u = _c_value(m, 1, 0.0039, 5.0)
    assert 0 < abs(float(f)) < 2.0 ** -14 and (u & 0x7C00) == 0 and (u & 0x3FF) != 0          # a binary16 subnormal
    f, u = _c_value(m, 1, 0.0, 3e38)
    assert 0 < float(f) < 2.0 ** -126 and u == 0                                              # an fp32 subnormal; binary16 zero
    assert float(_c_value(m, 255, 0.0, 1.0)[0]) == 1.0 and _c_value(m, 255, 0.0, 1.0)[1] == 0x3C00
    assert _c_value(m, 0, 0.0, 1.0) == (np.float32(0.0), np.uint16(0))
    import torch
    want = (torch.arange(256, dtype=torch.uint8).float() / 255.0).numpy()
    got = np.array([_c_value(m, k, 0.0, 1.0)[0] for k in range(256)], np.float32)
    assert np.array_equal(model.bits(got), model.bits(want))


def test_value_writes_only_what_is_asked_for():
    m = _lib()
    f, u = C.c_float(-77.0), C.c_uint16(0x7777)
    assert m.lib().yfv2_crop_tensor_value(7, 0.5, 0.5, C.byref(f), None) == 0 and f.value != -77.0
    assert m.lib().yfv2_crop_tensor_value(7, 0.5, 0.5, None, C.byref(u)) == 0 and u.value != 0x7777
    assert m.lib().yfv2_crop_tensor_value(7, 0.5, 0.5, None, None) == 0


@pytest.mark.parametrize("out_size", [(32, 32), (20, 12), (1, 4), (64, 24)])
def test_letterbox_equals_the_model_on_every_small_rectangle(out_size):
    m = _lib()
    H, W = out_size
    seen = set()
    for cw in range(1, 41):
        for ch in range(1, 41):
            got = _c_letterbox(m, cw, ch, H, W, 1)
            assert got == model.letterbox(cw, ch, H, W, True), (cw, ch, out_size)
            ox0, oy0, iw, ih = got
            assert 1 <= iw <= W and 1 <= ih <= H and (iw == W or ih == H), (cw, ch, got)
            assert ox0 == (W - iw) // 2 and oy0 == (H - ih) // 2 and ox0 + iw <= W and oy0 + ih <= H
            seen.add((iw == W, ih == H))
            assert _c_letterbox(m, cw, ch, H, W, 0) == (0, 0, W, H) == model.letterbox(cw, ch, H, W, False)
    assert (True, True) in seen and ((True, False) in seen or H == 1) and (False, True) in seen


def test_letterbox_extreme_equal_and_odd_cases():
    m = _lib()
    for H, W in ((32, 32), (20, 12), (1, 4), (64, 24)):
        for cw, ch in ((40000, 1), (1, 40000)):
            got = _c_letterbox(m, cw, ch, H, W, 1)
            assert got == model.letterbox(cw, ch, H, W, True)
            assert 1 <= got[2] <= W and 1 <= got[3] <= H
    assert _c_letterbox(m, 40000, 1, 32, 32, 1) == (0, 15, 32, 1)          # the inner height never falls to 0 ...
    assert _c_letterbox(m, 1, 40000, 32, 32, 1) == (15, 0, 1, 32)          # ... nor the inner width
    assert _c_letterbox(m, 2 ** 31 - 1, 1, 2 ** 15, 2 ** 15, 1) == (0, 2 ** 14 - 1, 2 ** 15, 1) == model.letterbox(2 ** 31 - 1, 1, 2 ** 15, 2 ** 15, True)
    # equal aspect: the whole output, no margin
    assert _c_letterbox(m, 24, 40, 20, 12, 1) == (0, 0, 12, 20) and _c_letterbox(m, 7, 7, 32, 32, 1) == (0, 0, 32, 32)
    # an odd margin: W - iw = 32 - 21 = 11 -> 5 on the left, 6 on the right; iw = (2 * 21 * 32 + 32) // 64 = 21
    assert _c_letterbox(m, 21, 32, 32, 32, 1) == (5, 0, 21, 32)
    assert _c_letterbox(m, 32, 21, 32, 32, 1) == (0, 5, 32, 21)
    # round half up: 3 x 2 into 32 wide -> ih = 21.33 -> 21; 2 x 1 into (32, 5) -> ih = 2.5 -> 3
    assert _c_letterbox(m, 3, 2, 32, 32, 1) == (0, 5, 32, 21)
    assert _c_letterbox(m, 2, 1, 32, 5, 1) == (0, 14, 5, 3)


def test_argument_errors_without_a_device():
    m = _lib()
    L = m.lib()
    r = (C.c_int32 * 4)(-77, -77, -77, -77)
    for args in ((0, 5, 8, 8, 1, r), (5, 0, 8, 8, 1, r), (5, 5, 0, 8, 1, r), (5, 5, 8, 0, 1, r), (5, 5, 8, 8, 2, r), (5, 5, 8, 8, -1, r), (5, 5, 8, 8, 1, None)):
        assert L.yfv2_crop_letterbox(*args) == m.ERR_ARG, args[:5]
        assert "yfv2_crop_letterbox" in m.last_error()
    assert list(r) == [-77] * 4
    f, u = C.c_float(-77.0), C.c_uint16(0x7777)
    for a, mean, std in ((-1, 0.0, 1.0), (256, 0.0, 1.0), (3, NAN, 1.0), (3, INF, 1.0), (3, 0.0, 0.0), (3, 0.0, -1.0), (3, 0.0, NAN), (3, 0.0, INF)):
        assert L.yfv2_crop_tensor_value(a, mean, std, C.byref(f), C.byref(u)) == m.ERR_ARG, (a, mean, std)
        assert "yfv2_crop_tensor_value" in m.last_error()
    assert f.value == -77.0 and u.value == 0x7777
    # the device entry points refuse a null handle before they look at anything else
    for name in ("yfv2_crop_tensors_u8", "yfv2_crop_tensors_yuv"):
        assert getattr(L, name)(None, None, 1, None, None, 1, None, None, None, None, None, None, None, 1, None) == m.ERR_ARG
        assert "null handle" in m.last_error()


def test_entry_points_are_bound_and_the_struct_has_the_c_layout():
    m = _lib()
    for name in ("yfv2_crop_letterbox", "yfv2_crop_tensor_value", "yfv2_crop_tensors_u8", "yfv2_crop_tensors_yuv"):
        assert name in m._PROTOTYPES and hasattr(m.lib(), name)
    assert C.sizeof(m.CropTensor) == 40 and m.CropTensor.mean.offset == 8 and m.CropTensor.std.offset == 20
    assert m.CropTensor.letterbox.offset == 32 and m.CropTensor.fill.offset == 36
    assert len(m._PROTOTYPES["yfv2_crop_tensors_u8"][1]) == len(m._PROTOTYPES["yfv2_crop_detections_u8"][1]) + 1
    assert m.lib().yfv2_abi_version() == 7          # additive symbols only


def test_the_model_composes_bytes_planes_and_fill():
    """a hand-made case: a 2 x 4 view into (4, 4) with letterbox lands in rows 1..3; rgb flips the planes, mean / std follow the plane"""
    view = np.arange(24, dtype=np.uint8).reshape(2, 4, 3) * 10
    img = model.byte_image(view, 4, 4, True, (1, 2, 3))
    assert model.letterbox(4, 2, 4, 4, True) == (0, 1, 4, 2)
    assert np.array_equal(img[1:3], view) and (img[0] == [1, 2, 3]).all() and (img[3] == [1, 2, 3]).all()
    t = model.from_bytes(img, (0.0, 0.5, 0.25), (1.0, 2.0, 4.0), True, False)
    assert t.shape == (3, 4, 4) and t.dtype == np.float32
    assert t[0, 0, 0] == np.float32(3) / np.float32(255)                                   # plane 0 of rgb is byte channel 2 (R)
    assert t[2, 1, 1] == (np.float32(30) / np.float32(255) - np.float32(0.25)) / np.float32(4.0)   # plane 2 is B of pixel (0, 1) of the view
    assert model.from_bytes(img, (0, 0, 0), (1, 1, 1), False, True).dtype == np.float16
