"""CPU-only checks of the ragged-batch entry points (yfv2_resize_frames_u8 / yfv2_detect_frames_u8):
  * both are exported and bound, and refuse a NULL handle with YFV2_ERR_ARG (no GPU involved)
  * the per-frame staging guard of resize_frames_u8_kernel never loads a whole dword that leaves the frame's extent, and
    still stages every byte of the row
  * the frame-coordinate formula agrees with test.py's arithmetic
"""
import ctypes as C
import os

import numpy as np

from frames_ref import stage_row, to_frame_coords


def _lib():
    from yolo_fastestv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_frame_entry_points_are_exported_and_refuse_a_null_handle():
    m = _lib()
    L = m.lib()
    raw = C.CDLL(m.LIB_PATH)
    for name in ("yfv2_resize_frames_u8", "yfv2_detect_frames_u8"):
        assert name in m._PROTOTYPES and hasattr(raw, name)
    assert C.sizeof(m.Frame) == 24      # pointer, two int32, int64: the layout of yfv2_frame
    fr = (m.Frame * 1)()
    fr[0].data, fr[0].height, fr[0].width, fr[0].row_pitch = 64, 4, 4, 12
    assert L.yfv2_resize_frames_u8(None, fr, 1, C.c_void_p(64), None) == m.ERR_ARG
    assert "null handle" in m.last_error()
    assert L.yfv2_detect_frames_u8(None, fr, 1, 0.3, 0.4, C.c_void_p(64), C.c_void_p(64), C.c_void_p(64), None) == m.ERR_ARG
    assert "null handle" in m.last_error()


def _check_frame(base_align, h, w, pitch, rng):
    """A frame of h rows of 3w bytes with row pitch `pitch` placed at an address with base % 4 == base_align inside a larger
    memory whose other bytes belong to nobody: every row staged through the guard equals the frame's row, every whole-dword
    load stays inside the extent, and the byte loads do too."""
    extent = (h - 1) * pitch + 3 * w
    pad = 16
    base = pad + base_align
    mem = rng.integers(0, 256, base + extent + pad, dtype=np.uint8)
    inside = set(range(base, base + extent))
    for r in range(h):
        g = r * pitch
        staged, mis, whole, single = stage_row(mem, base, extent, g, 3 * w)
        assert np.array_equal(staged[mis:mis + 3 * w], mem[base + g:base + g + 3 * w]), (base_align, h, w, pitch, r)
        assert whole <= inside, (base_align, h, w, pitch, r, sorted(whole - inside))
        assert single <= inside
        # every byte of the row came from one of the two kinds of load
        assert set(range(base + g, base + g + 3 * w)) <= whole | single


def test_staging_guard_stays_inside_each_frame():
    rng = np.random.default_rng(0)
    n = 0
    for align in range(4):
        for w in range(1, 8):
            for extra in (0, 1, 2, 3, 5, 8):          # pitch == 3w, and crops of wider frames
                for h in (1, 2, 3, 5):
                    _check_frame(align, h, w, 3 * w + extra, rng)
                    n += 1
        _check_frame(align, 1, 1, 3, rng)               # the 1x1 frame: three bytes, never a whole dword
    assert n == 4 * 7 * 6 * 4


def test_single_pixel_frame_is_read_byte_by_byte():
    rng = np.random.default_rng(1)
    for align in range(4):
        mem = rng.integers(0, 256, 32, dtype=np.uint8)
        staged, mis, whole, single = stage_row(mem, 8 + align, 3, 0, 3)
        assert not whole and single == {8 + align, 9 + align, 10 + align}
        assert np.array_equal(staged[mis:mis + 3], mem[8 + align:11 + align])


def test_frame_coordinates_match_test_py_arithmetic():
    """test.py:58,65-66: scale_w = w / cfg["width"]; x1 = box[0] * scale_w with box a list of Python floats (the fp32 values
    exactly); the device keeps the product in fp32 (rounded to nearest)."""
    rng = np.random.default_rng(2)
    sizes = [(1080, 1920), (720, 1280), (480, 640), (352, 352), (1, 1), (353, 351), (2, 20000), (7, 3)]
    B = len(sizes)
    dets = (rng.random((B, 300, 6)) * 400 - 24).astype(np.float32)
    dets[:, :, 5] = rng.integers(0, 80, (B, 300))
    count = rng.integers(0, 301, B).astype(np.int32)
    count[0], count[1] = 300, 0
    got = to_frame_coords(dets, count, sizes, 352, 352)
    for b, (h, w) in enumerate(sizes):
        scale_h, scale_w = h / 352, w / 352                      # Python floats, as test.py computes them
        for i in range(300):
            box = dets[b, i].tolist()
            if i < count[b]:
                want = [box[0] * scale_w, box[1] * scale_h, box[2] * scale_w, box[3] * scale_h]
                assert [np.float32(v) for v in want] == list(got[b, i, :4]), (b, i)
            else:
                assert np.array_equal(got[b, i, :4].view(np.uint32), dets[b, i, :4].view(np.uint32))
        assert np.array_equal(got[b, :, 4:].view(np.uint32), dets[b, :, 4:].view(np.uint32))
    # scale 1 (a 352x352 frame) is an exact copy
    assert np.array_equal(got[3].view(np.uint32), dets[3].view(np.uint32))
