"""CPU-only checks of the training-batch front door (include/yfv2.h yfv2_train_batch_frames_u8 / _yuv, yolo_fastestv2_amd/datasets.py;
DESIGN.md 4.16): the symbols and their binding, the numpy statement's roundings (tests/train_batch_model.py), and the host half of
utils/datasets.py - the draws, the label files and collate_fn's label numbering - against restatements of the reference's lines."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import rows_model as rm
import train_batch_model as tm
from conftest import REPO

F32 = np.float32


# ---- 1. symbols, declarations, ABI -------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    import yolo_fastestv2_amd as yfv2
    from yolo_fastestv2_amd import _lib
    assert os.path.exists(yfv2.LIB_PATH), "libyfv2.so not built"
    L = _lib.lib()
    assert L.yfv2_abi_version() == _lib.ABI_VERSION == 7                      # additive: the ABI number stays
    header = open(os.path.join(REPO, "include", "yfv2.h")).read()
    for name, frame in (("yfv2_train_batch_frames_u8", _lib.Frame), ("yfv2_train_batch_frames_yuv", _lib.FrameYuv)):
        assert hasattr(L, name), name
        res, args = _lib._PROTOTYPES[name]
        assert res is C.c_int and args == [C.c_void_p, C.POINTER(frame), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        m = re.search(r"YFV2_API int %s\s*\(([^;]*)\);" % name, header)
        assert m, "%s is not declared in include/yfv2.h" % name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert len(params) == 7 and params[3] == "const float* alpha" and params[4] == "const float* beta" and params[5] == "float* dst", params
    assert "#define YFV2_ABI_VERSION 7" in header or re.search(r"YFV2_ABI_VERSION\s*=?\s*7", header)
    # the public frame structs did not change
    assert C.sizeof(_lib.Frame) == 24 and C.sizeof(_lib.FrameYuv) == 64
    # a null handle is refused without touching a device
    assert L.yfv2_train_batch_frames_u8(None, None, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.yfv2_train_batch_frames_yuv(None, None, 1, None, None, None, None) == _lib.ERR_ARG
    for name in ("TrainBatcher", "collate_targets", "draw_contrast_brightness", "read_label_file", "datasets"):
        assert hasattr(yfv2, name), name
    assert hasattr(yfv2.Engine, "train_batch_frames") and hasattr(yfv2.Engine, "train_batch_frames_yuv")


# ---- 2. the table --------------------------------------------------------------------------------------------------------------
def test_identity_is_byte_over_255():
    t = tm.table(1, 0)
    assert t.dtype == np.float32
    for a in range(256):
        assert t[a] == F32(a) / F32(255), a
    assert np.array_equal(t, (torch.arange(256, dtype=torch.uint8).float() / 255.0).numpy())     # train.py:101
    assert np.array_equal(tm.quantised(1, 0), np.arange(256))


def test_rounding_in_the_model():
    # (1, 0.5): every byte lands on a tie, a + 0.5 -> the even neighbour
    q = tm.quantised(1, 0.5)
    for a in range(256):
        assert q[a] == (a if a % 2 == 0 else min(a + 1, 255)), a
    assert q[255] == 255                                               # 255.5 is clamped to 255 before the rounding
    # (0.5, 0): every odd byte is a tie, a / 2 -> the even neighbour
    q = tm.quantised(0.5, 0)
    for a in range(256):
        want = a // 2 if a % 2 == 0 else (a // 2 if (a // 2) % 2 == 0 else a // 2 + 1)
        assert q[a] == want, a
    assert [int(v) for v in q[:8]] == [0, 0, 1, 2, 2, 2, 3, 4]
    # the ends of the reference's range
    q = tm.quantised(1.75, 1.75)
    assert q.max() == 255 and int((q == 255).sum()) > 100 and q[0] == 2           # rint(1.75) = 2; saturates from a = 145 on
    assert q[144] == 254 and q[145] == 255                                         # 144 * 1.75 + 1.75 = 253.75, 145: 255.5 -> clamp
    q = tm.quantised(0.25, 0.25)
    assert q.max() == 64 and q[0] == 0 and q[255] == 64                            # 63.75 + 0.25 = 64: no saturation anywhere
    # two roundings, not one: a * alpha rounds to fp32 before beta is added
    a, al, be = 3, F32(1.3), F32(-7.25)
    two = F32(F32(F32(a) * al) + be)
    assert tm.table(al, be)[a] == F32(np.rint(min(max(two, F32(0)), F32(255)))) / F32(255)
    # a huge finite alpha clamps (a * alpha overflows to +inf for a >= 2; 0 * alpha stays 0), a huge negative one clamps to 0
    big = np.finfo(np.float32).max
    q = tm.quantised(big, 0)
    assert q[0] == 0 and (q[1:] == 255).all()
    assert (tm.quantised(-big, 0) == 0).all()
    assert (tm.quantised(big, -big)[2:] == 255).all() and np.isfinite(tm.table(big, -big)).all()
    assert np.isfinite(tm.table(-big, big)).all()


def test_train_batch_ref_layout():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)
    out = tm.train_batch_ref(x)
    assert out.shape == (2, 3, 4, 6) and out.dtype == np.float32
    assert np.array_equal(out, (torch.from_numpy(x).permute(0, 3, 1, 2).float() / 255.0).numpy())
    out = tm.train_batch_ref(x, [1.3, 0.5], [-7.25, 3.0])
    for b, (al, be) in enumerate(((1.3, -7.25), (0.5, 3.0))):
        for c in range(3):
            assert np.array_equal(out[b, c], tm.table(al, be)[x[b, :, :, c]])


# ---- 3. the LDS function and the width limits ----------------------------------------------------------------------------------
def test_lds_bytes_and_width_limits():
    from yolo_fastestv2_amd import datasets as ds, yuv
    full = ds.LDS_FULL
    for W in (32, 64, 96, 352, 640):
        m = ds.max_frame_width(W)
        assert m == rm.max_width(rm.TRAIN, rm.BGR, W) and ds.train_batch_lds_bytes(m, W) == rm.lds_bytes(rm.TRAIN, rm.BGR, m, W)
        assert ds.train_batch_lds_bytes(m, W) <= full
        assert m < (full - 3 * W) // 6 - 2                              # below resize_frames' limit: what this takes, that takes
        assert ds.train_batch_lds_bytes(m + 6, W) > full                # and no more than a slot's rounding below the true maximum
        my = ds.max_frame_width(W, True)
        assert my == rm.max_width(rm.TRAIN, rm.YUV8, W) and ds.train_batch_lds_bytes(my, W, True) == rm.lds_bytes(rm.TRAIN, rm.YUV8, my, W)
        assert ds.train_batch_lds_bytes(my, W, True) <= full < ds.train_batch_lds_bytes(my + 1, W, True)
        assert my <= yuv.max_width(W)
    assert ds.max_frame_width(352) == 26426 and ds.train_batch_lds_bytes(26426, 352) == full
    assert ds.max_frame_width(352, True) == 39641
    # the 16-byte slots hold what the staging writes, for every width and misalignment (the resize's own slots are the 4-byte form)
    for w in range(1, 200):
        for mis in range(4):
            assert ((mis + 3 * w + 3) >> 2) * 4 <= rm.slot(3 * w, 16)
            assert ((mis + w + 3) >> 2) * 4 <= rm.slot(w, 16)
            for px in (0, 1):
                cw = ((w - 1 + px) >> 1) + 1
                half = rm.slot((w >> 1) + 1, 16)
                assert ((mis + cw + 3) >> 2) * 4 <= half and ((mis + 2 * cw + 3) >> 2) * 4 <= 2 * half


# ---- 4. the host half of utils/datasets.py -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_draws_are_the_references(seed):
    from yolo_fastestv2_amd import datasets as ds
    random.seed(seed)
    want = []
    for _ in range(5):                                   # datasets.py:11-12, per image: alpha, then beta
        alpha = random.uniform(0.25, 1.75)
        beta = random.uniform(0.25, 1.75)
        want.append((alpha, beta))
    random.seed(seed)
    got = [ds.draw_contrast_brightness() for _ in range(5)]
    assert got == want
    r = random.Random(seed)
    assert [ds.draw_contrast_brightness(r) for _ in range(5)] == want      # random.seed(s) and Random(s) are one stream
    assert all(0.25 <= v <= 1.75 for p in got for v in p)


def _collate_labels_restated(labels):
    """collate_fn's label half (datasets.py:70-75), on copies"""
    label = [torch.from_numpy(np.array(l, dtype=np.float32).reshape(-1, 6).copy()) for l in labels]
    for i, l in enumerate(label):
        if l.shape[0] > 0:
            l[:, 0] = i
    return torch.cat(label, 0)


def test_collate_targets():
    from yolo_fastestv2_amd import datasets as ds
    rng = np.random.default_rng(7)
    a = rng.random((3, 6)).astype(np.float32)
    c = rng.random((2, 6)).astype(np.float32)
    empty = np.zeros((0, 6), np.float32)
    before = a.copy()
    for labels in ([a, empty, c], [empty, empty], [a], [empty, c, empty, a]):
        got = ds.collate_targets(labels)
        want = _collate_labels_restated(labels)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and got.shape[1] == 6
        assert torch.equal(got, want)
    assert np.array_equal(a, before), "collate_targets wrote the caller's array"
    got = ds.collate_targets([a, empty, c])
    assert got[:, 0].tolist() == [0, 0, 0, 2, 2]
    assert torch.equal(ds.collate_targets([torch.from_numpy(a), torch.from_numpy(c)]), _collate_labels_restated([a, c]))
    assert torch.equal(ds.collate_targets([a.astype(np.float64)]), _collate_labels_restated([a]))


def test_read_label_file(tmp_path):
    from yolo_fastestv2_amd import datasets as ds
    p = tmp_path / "img0.txt"
    p.write_text("3 0.5 0.25 0.125 0.0625\n17 0.1 0.2 0.3 0.4\n")
    got = ds.read_label_file(str(p))
    assert got.dtype == np.float32 and got.shape == (2, 6)
    assert np.array_equal(got, np.array([[0, 3, 0.5, 0.25, 0.125, 0.0625], [0, 17, 0.1, 0.2, 0.3, 0.4]], dtype=np.float32))
    e = tmp_path / "empty.txt"
    e.write_text("")
    got = ds.read_label_file(str(e))
    assert got.dtype == np.float32 and got.shape == (0, 6)
    t = ds.collate_targets([ds.read_label_file(str(e)), ds.read_label_file(str(p))])
    assert t[:, 0].tolist() == [1, 1] and t[:, 1].tolist() == [3, 17]
    with pytest.raises(OSError):
        ds.read_label_file(str(tmp_path / "missing.txt"))


def test_batcher_refuses_mixed_kinds_without_a_device():
    from yolo_fastestv2_amd import datasets as ds

    class NoEngine:
        device = torch.device("cpu")

    b = ds.TrainBatcher(NoEngine(), imgaug=True, rng=random.Random(3))
    with pytest.raises(ValueError):
        b([torch.zeros((2, 2, 3), dtype=torch.uint8), object()], [np.zeros((0, 6), np.float32)] * 2)
    with pytest.raises(ValueError):
        b([], [])
    with pytest.raises(ValueError):
        b([torch.zeros((2, 2, 3), dtype=torch.uint8)], [])
