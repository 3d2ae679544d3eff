"""Host models for the ragged-batch entry points (yfv2_resize_frames_u8 / yfv2_detect_frames_u8), shared by
tests/test_frames_host.py (CPU) and tests/test_gpu_frames.py (GPU).

* stage_row: the per-frame staging guard of resize_frames_u8_kernel (yfv2_pre.hip), restated dword by dword.
* to_frame_coords: the frame-coordinate epilogue (frame_boxes_kernel, yfv2_post.hip) in numpy float64.
"""
import numpy as np

MAX_DET = 300


def stage_row(mem, base, extent, g, row_bytes):
    """What one workgroup stages for the source row at byte offset g of a frame that starts at mem[base] and owns the bytes
    [base, base + extent).  The kernel loads aligned dwords covering [base + g, base + g + row_bytes); a dword is loaded whole
    only if its four bytes lie inside the extent, otherwise byte by byte from those that do.  Returns (staged bytes, the
    offset of the row's first byte in them, the set of absolute addresses a whole-dword load touched, the set of absolute
    addresses a byte load touched)."""
    mis = (base + g) & 3
    nd = (mis + row_bytes + 3) >> 2
    first = g - mis
    staged = np.zeros(4 * nd, np.uint8)
    whole, single = set(), set()
    for i in range(nd):
        lo = first + 4 * i
        if lo >= 0 and lo + 4 <= extent:
            assert (base + lo) % 4 == 0
            staged[4 * i:4 * i + 4] = mem[base + lo:base + lo + 4]
            whole.update(range(base + lo, base + lo + 4))
        else:
            for k in range(4):
                if 0 <= lo + k < extent:
                    staged[4 * i + k] = mem[base + lo + k]
                    single.add(base + lo + k)
    return staged, mis, whole, single


def to_frame_coords(dets, count, sizes, width, height):
    """dets (B,300,6) fp32 in network coordinates -> frame coordinates: columns 0-3 of the first count[b] rows times
    w_b / width (x) and h_b / height (y) in float64, rounded to fp32 (test.py:58,65-66).  sizes: [(h_b, w_b)]."""
    out = np.array(dets, np.float32, copy=True)
    for b, (h, w) in enumerate(sizes):
        n = int(count[b])
        sx, sy = np.float64(w) / np.float64(width), np.float64(h) / np.float64(height)
        r = out[b, :n, :4].astype(np.float64)
        r[:, 0::2] *= sx
        r[:, 1::2] *= sy
        out[b, :n, :4] = r.astype(np.float32)
    return out
