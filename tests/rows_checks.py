"""What the CPU tests of the row kernels' LDS and width limits share (test_rows_host.py: B, G, R and 4:2:0 bytes; test_yuv16_host.py:
two-byte samples; test_yuv_any_host.py: the general one-byte launch): the call of the frame kind's debug hook and the bodies of the
two checks every frame kind gets - the hook is declared, bound and checks its arguments; its bytes and limit equal tests/rows_model.py."""
import ctypes as C
import os
import re

import pytest

import rows_model as rm
from conftest import REPO

FULL = rm.LDS_FULL


def _rows(kind, frames, w, W):
    """(LDS bytes, width limit) from the debug hook of the frame kind (a bool: B, G, R / 4:2:0 bytes, as yfv2_debug_rows takes it)"""
    from yolo_fastestv2_amd import _lib
    L, lds, limit = _lib.lib(), C.c_int64(-1), C.c_int32(-1)
    hook, lead = {rm.BGR: (L.yfv2_debug_rows, (0,)), rm.YUV8: (L.yfv2_debug_rows, (1,)), rm.YUV16: (L.yfv2_debug_rows16, ()), rm.YUV8_ANY: (L.yfv2_debug_rows_any, ())}[int(frames)]
    assert hook(kind, *lead, w, W, C.byref(lds), C.byref(limit)) == _lib.OK, (kind, frames, w, W)
    return lds.value, limit.value


def check_export(hook, lead, package_function):
    """one of the three yfv2_debug_rows* hooks is declared, bound and checks its arguments; lead: what it takes between row_kind and w"""
    from yolo_fastestv2_amd import _lib
    L = _lib.lib()
    assert L.yfv2_abi_version() == _lib.ABI_VERSION == 7                      # additive: the ABI number stays
    res, args = _lib._PROTOTYPES[hook]
    assert res is C.c_int and args == [C.c_int32] * (3 + len(lead)) + [C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    header = open(os.path.join(REPO, "include", "yfv2.h")).read()
    params = "".join(r"int32_t %s, " % name for name in ("row_kind",) + lead + ("w", "W"))
    assert re.search(r"YFV2_API int %s\(%sint64_t\* lds_bytes, int32_t\* max_width\);" % (hook, params), header)
    call, zeros = getattr(L, hook), (0,) * len(lead)
    assert call(0, *zeros, 1920, 352, None, None) == _lib.OK                  # either output may be NULL
    for kind, w, W in ((-1, 8, 8), (5, 8, 8), (0, 0, 8), (0, (1 << 26) + 1, 8), (0, 8, 0), (0, 8, (1 << 20) + 1)):
        assert call(kind, *zeros, w, W, None, None) == _lib.ERR_ARG, (kind, w, W)
    with pytest.raises(ValueError):
        package_function(9, *zeros, 8, 8)


def check_lds_bytes_and_limit(kind, frames):
    """every W % 4 == 0 up to 4096: the limit, and the bytes at the widths where a rule could break - the smallest frames, around
    the limit, a 1080p row, around the exact maximum; then w in 1..4100 and at the limit +- 2 for W in {32, 352, 4096}.  A YUV limit
    is the exact maximum; no other YUV kind admits a frame the 4:2:0 byte kind refuses at the same W, and the general launch never
    takes less LDS than the 4:2:0 one."""
    for W in range(4, 4097, 4):
        limit = _rows(kind, frames, 1, W)[1]
        assert limit == rm.max_width(kind, frames, W), W
        exact = rm.exact_max_width(kind, frames, W)
        for w in {1, 2, 3, limit - 1, limit, limit + 1, 1920, exact - 1, exact + 1, limit + 6}:
            assert _rows(kind, frames, max(w, 1), W)[0] == rm.lds_bytes(kind, frames, max(w, 1), W), (w, W)
        assert rm.lds_bytes(kind, frames, limit, W) <= FULL, W                 # what is admitted fits ...
        if frames != rm.BGR:
            assert limit == exact and rm.lds_bytes(kind, frames, limit + 1, W) > FULL, W     # ... and nothing wider would
            assert limit <= rm.max_width(kind, rm.YUV8, W), W
        else:
            assert limit <= exact and rm.lds_bytes(kind, frames, limit + 6, W) > FULL, W     # ... no more than a slot's rounding below
    for W in (32, 352, 4096):
        limit = _rows(kind, frames, 1, W)[1]
        for w in list(range(1, 4101)) + [limit + d for d in (-2, -1, 0, 1, 2)]:
            assert _rows(kind, frames, w, W) == (rm.lds_bytes(kind, frames, w, W), limit), (w, W)
        assert _rows(kind, frames, limit, W)[0] <= FULL, W
        if frames != rm.BGR:
            assert FULL < _rows(kind, frames, limit + 1, W)[0], W
        if frames == rm.YUV8_ANY:
            for w in (1, 2, 3, 640, 1920, limit):
                assert rm.lds_bytes(kind, frames, w, W) >= rm.lds_bytes(kind, rm.YUV8, w, W), (w, W)
