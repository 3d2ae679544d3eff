"""CPU-only: the library's one description of the row kernels - the LDS a launch asks for and the width limit an entry point
enforces, for every row kind and both frame kinds (include/yfv2.h yfv2_debug_rows; yfv2_pre.hip FrameRows) - against the one
restatement, tests/rows_model.py.  A launch that asked for less LDS than its kernel uses would write outside its allocation on the
device; this sweep is what holds the host's arithmetic to the kernels' layout without a device."""
import ctypes as C
import os
import re

import pytest

import rows_model as rm
from conftest import REPO

FULL = rm.LDS_FULL


def _rows(kind, is_yuv, w, W):
    from yolo_fastestv2_amd import _lib
    lds, limit = C.c_int64(-1), C.c_int32(-1)
    assert _lib.lib().yfv2_debug_rows(kind, int(is_yuv), w, W, C.byref(lds), C.byref(limit)) == _lib.OK, (kind, is_yuv, w, W)
    return lds.value, limit.value


def test_export_is_declared_bound_and_checks_its_arguments():
    from yolo_fastestv2_amd import _lib, yuv
    L = _lib.lib()
    assert L.yfv2_abi_version() == _lib.ABI_VERSION == 7                      # additive: the ABI number stays
    res, args = _lib._PROTOTYPES["yfv2_debug_rows"]
    assert res is C.c_int and args == [C.c_int32] * 4 + [C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    header = open(os.path.join(REPO, "include", "yfv2.h")).read()
    assert re.search(r"YFV2_API int yfv2_debug_rows\(int32_t row_kind, int32_t yuv, int32_t w, int32_t W, int64_t\* lds_bytes, int32_t\* max_width\);", header)
    assert (yuv.ROWS_U8, yuv.ROWS_COUNTED_U8, yuv.ROWS_TRAIN, yuv.ROWS_TENSOR_F32, yuv.ROWS_TENSOR_F16) == rm.KINDS
    assert L.yfv2_debug_rows(0, 0, 1920, 352, None, None) == _lib.OK          # either output may be NULL
    for bad in ((-1, 0, 8, 8), (5, 0, 8, 8), (0, 2, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, (1 << 26) + 1, 8), (0, 0, 8, 0), (0, 0, 8, (1 << 20) + 1)):
        assert L.yfv2_debug_rows(*bad, None, None) == _lib.ERR_ARG, bad
    with pytest.raises(ValueError):
        yuv.rows_lds(9, False, 8, 8)


@pytest.mark.parametrize("is_yuv", [False, True], ids=["bgr", "yuv"])
@pytest.mark.parametrize("kind", rm.KINDS, ids=["u8", "counted_u8", "train", "tensor_f32", "tensor_f16"])
def test_lds_bytes_and_limit_equal_the_restatement(kind, is_yuv):
    """every W % 4 == 0 up to 4096: the limit, and the bytes at the widths where a rule could break - the smallest frames, around
    the limit, a 1080p row, around the exact maximum"""
    for W in range(4, 4097, 4):
        limit = _rows(kind, is_yuv, 1, W)[1]
        assert limit == rm.max_width(kind, is_yuv, W), W
        exact = rm.exact_max_width(kind, is_yuv, W)
        for w in {1, 2, 3, limit - 1, limit, limit + 1, 1920, exact - 1, exact + 1, limit + 6}:
            assert _rows(kind, is_yuv, w, W)[0] == rm.lds_bytes(kind, is_yuv, w, W), (w, W)
        assert rm.lds_bytes(kind, is_yuv, limit, W) <= FULL, W                 # what is admitted fits ...
        if is_yuv:
            assert limit == exact and rm.lds_bytes(kind, True, limit + 1, W) > FULL, W       # ... and nothing wider would
        else:
            assert limit <= exact and rm.lds_bytes(kind, False, limit + 6, W) > FULL, W      # ... no more than a slot's rounding below


def test_pinned_values():
    assert _rows(rm.U8, False, 1, 352)[1] == 27128 and _rows(rm.COUNTED_U8, False, 1, 352)[1] == 27128
    assert rm.exact_max_width(rm.U8, False, 352) == 27129                      # yfv2_resize_u8 tests the bytes: one pixel more
    assert _rows(rm.U8, True, 1, 352)[1] == 40689
    assert _rows(rm.TRAIN, False, 26426, 352) == (FULL, 26426)                 # the widest training row fills the LDS to the byte
    assert _rows(rm.TRAIN, True, 1, 352)[1] == 39641
    assert _rows(rm.TENSOR_F32, False, 1, 64)[1] == 27172 and _rows(rm.TENSOR_F16, False, 1, 64)[1] == 27236
    assert _rows(rm.U8, True, 1920, 352)[0] == 8760                            # 18 workgroups of a 1080p batch per CU by LDS
    assert _rows(rm.U8, False, 1920, 352)[0] == 12584                          # ... where the B, G, R kernel's rows take 12 584 bytes
    assert _rows(rm.TRAIN, False, 1920, 352)[0] == 16800 and _rows(rm.TRAIN, True, 1920, 352)[0] == 13024


@pytest.mark.parametrize("is_yuv", [False, True], ids=["bgr", "yuv"])
def test_a_wider_row_format_never_admits_more(is_yuv):
    """what the tensor entry points take, the crops' take at the same out_w; what the training entry points take, the resize's take"""
    for W in range(4, 4097, 4):
        crops, resize = _rows(rm.COUNTED_U8, is_yuv, 1, W)[1], _rows(rm.U8, is_yuv, 1, W)[1]
        assert crops == resize
        f32, f16, train = (_rows(k, is_yuv, 1, W)[1] for k in (rm.TENSOR_F32, rm.TENSOR_F16, rm.TRAIN))
        assert f32 <= f16 <= crops and train <= resize and train <= f32, W


def test_package_functions_take_their_values_from_the_library():
    from yolo_fastestv2_amd import datasets as ds, yuv
    for W in (32, 64, 352, 640):
        assert yuv.max_width(W) == _rows(rm.U8, True, 1, W)[1]
        for is_yuv in (False, True):
            assert ds.max_frame_width(W, is_yuv) == _rows(rm.TRAIN, is_yuv, 1, W)[1]
            for w in (1, 351, 1920, 27128):
                assert ds.train_batch_lds_bytes(w, W, is_yuv) == _rows(rm.TRAIN, is_yuv, w, W)[0]
                assert yuv.resize_lds_bytes(w, W) == _rows(rm.U8, True, w, W)[0]


def test_slots_hold_what_the_staging_writes():
    """for every width, misalignment and origin parity: the dwords a row's staging writes fit its slot, at either alignment"""
    for a in (4, 16):
        for w in range(1, 200):
            for mis in range(4):
                assert ((mis + 3 * w + 3) >> 2) * 4 <= rm.slot(3 * w, a)
                assert ((mis + w + 3) >> 2) * 4 <= rm.slot(w, a)
                for px in (0, 1):
                    cw = ((w - 1 + px) >> 1) + 1
                    half = rm.slot(w // 2 + 1, a)
                    assert ((mis + cw + 3) >> 2) * 4 <= half and ((mis + 2 * cw + 3) >> 2) * 4 <= 2 * half
