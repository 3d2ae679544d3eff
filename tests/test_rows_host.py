"""CPU-only: the library's one description of the row kernels - the LDS a launch asks for and the width limit an entry point
enforces, for every row kind and frame kind (include/yfv2.h yfv2_debug_rows, _rows16, _rows_any; yfv2_pre.hip FrameRows) - against the one
restatement, tests/rows_model.py.  A launch that asked for less LDS than its kernel uses would write outside its allocation on the
device; this sweep is what holds the host's arithmetic to the kernels' layout without a device."""

import pytest

import rows_model as rm
from rows_checks import _rows, check_export, check_lds_bytes_and_limit

FULL = rm.LDS_FULL


def test_export_is_declared_bound_and_checks_its_arguments():
    from yolo_fastestv2_amd import _lib, yuv
    check_export("yfv2_debug_rows", ("yuv",), yuv.rows_lds)
    assert (yuv.ROWS_U8, yuv.ROWS_COUNTED_U8, yuv.ROWS_TRAIN, yuv.ROWS_TENSOR_F32, yuv.ROWS_TENSOR_F16) == rm.KINDS
    for bad in ((0, 2, 8, 8), (0, -1, 8, 8)):                                  # yuv is 0 or 1
        assert _lib.lib().yfv2_debug_rows(*bad, None, None) == _lib.ERR_ARG, bad


@pytest.mark.parametrize("is_yuv", [False, True], ids=["bgr", "yuv"])
@pytest.mark.parametrize("kind", rm.KINDS, ids=rm.KIND_IDS)
def test_lds_bytes_and_limit_equal_the_restatement(kind, is_yuv):
    check_lds_bytes_and_limit(kind, rm.YUV8 if is_yuv else rm.BGR)


def test_pinned_values():
    assert _rows(rm.U8, False, 1, 352)[1] == 27128 and _rows(rm.COUNTED_U8, False, 1, 352)[1] == 27128
    assert rm.exact_max_width(rm.U8, rm.BGR, 352) == 27129                      # yfv2_resize_u8 tests the bytes: one pixel more
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
