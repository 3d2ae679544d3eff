"""The LDS of a workgroup of the row kernels (yfv2_pre.hip: resize_frames_u8_kernel / resize_frames_yuv_kernel) and the width
limits the frame entry points derive from it, restated once for all five row kinds and all four frame kinds - what the kernels'
staging needs, written from that need and not from the library's expressions.  tests/test_rows_host.py sweeps the library
(yfv2_debug_rows, yfv2_debug_rows16, yfv2_debug_rows_any) against this file; the GPU tests take their at-the-limit widths from here.
"""
LDS_FULL = 160 * 1024
U8, COUNTED_U8, TRAIN, TENSOR_F32, TENSOR_F16 = range(5)     # yfv2_debug_rows' row_kind
KINDS = (U8, COUNTED_U8, TRAIN, TENSOR_F32, TENSOR_F16)
KIND_IDS = ["u8", "counted_u8", "train", "tensor_f32", "tensor_f16"]
BGR, YUV8, YUV16, YUV8_ANY = range(4)                          # the frame kinds: B, G, R; YUV 4:2:0 of 1-byte and of 2-byte samples; any 8-bit YUV
TABLE_BYTES = 256 * 4                                          # the training rows' augmentation table


def align(kind):
    """what the row behind the staging slots needs its LDS aligned to: dword stores for the uint8 rows, 16-byte stores otherwise"""
    return 4 if kind in (U8, COUNTED_U8) else 16


def own_bytes(kind, W):
    """the row's own LDS for an output row of W pixels: 3 W bytes; the table and three fp32 planes; three fp32 / fp16 planes"""
    return {U8: 3 * W, COUNTED_U8: 3 * W, TRAIN: TABLE_BYTES + 3 * W * 4, TENSOR_F32: 3 * W * 4, TENSOR_F16: 3 * W * 2}[kind]


def slot(n, a):
    """a staged row of n bytes: up to 3 bytes of head misalignment in front of it, rounded up to the row's alignment"""
    return (n + 3 + a - 1) // a * a


def lds_bytes(kind, frames, w, W):
    """B, G, R: two source rows of 3 w bytes.  YUV 4:2:0 of sb-byte samples: two luma rows of sb w bytes and two chroma rows, each
    either one interleaved row of 2 sb (w // 2 + 1) bytes or two planar rows of sb (w // 2 + 1) in a half-slot each (two half-slots
    hold the interleaved row).  The general launch: six slots of w bytes, a group of three per blended source row ([luma][U][V]; an
    interleaved row lies over U and V, a packed row over all three).  Then the row kind's own bytes."""
    a = align(kind)
    if frames == BGR:
        return 2 * slot(3 * w, a) + own_bytes(kind, W)
    if frames == YUV8_ANY:
        return 6 * slot(w, a) + own_bytes(kind, W)
    sb = 2 if frames == YUV16 else 1
    half = slot(sb * (w // 2 + 1), a)
    assert 2 * half >= slot(2 * sb * (w // 2 + 1), a)
    return 2 * slot(sb * w, a) + 2 * 2 * half + own_bytes(kind, W)


def exact_max_width(kind, frames, W):
    """the widest frame with lds_bytes <= a CU's LDS, by bisection on a function that never falls (1 if none fits)"""
    lo, hi = 1, LDS_FULL
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lds_bytes(kind, frames, mid, W) <= LDS_FULL:
            lo = mid
        else:
            hi = mid - 1
    return lo


def max_width(kind, frames, W):
    """the limit the entry points enforce (include/yfv2.h).  YUV: the exact maximum.  B, G, R: a closed form - a slot is at most
    3 w + align + 2 bytes - which lies a few pixels below the exact maximum."""
    if frames != BGR:
        return exact_max_width(kind, frames, W)
    return (LDS_FULL - own_bytes(kind, W)) // 6 - (align(kind) + 2) // 3
