"""GPU tests of the training-batch front door: Engine.train_batch_frames / train_batch_frames_yuv and datasets.TrainBatcher
(include/yfv2.h yfv2_train_batch_frames_u8 / _yuv).  Run with ``-m gpu`` on an MI355X.

One claim, everywhere: the fp32 (B, 3, H, W) batch is bit-identical to the EXISTING entry point's resized uint8 batch
(Engine.resize_frames / resize_frames_yuv, on the device) put through the numpy statement of tests/train_batch_model.py.  Every
comparison is exact; the expected value never comes from the code under test.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import train_batch_model as tm
import yuv_model as ym

pytestmark = pytest.mark.gpu

PAIRS = [(1, 0), (1, 0.5), (0.5, 0), (0.25, 0.25), (1.75, 1.75), (1.3, -7.25)]
NETS = [(32, 32), (64, 96), (352, 352)]          # (height, width); 64 x 96: an H / W swap in the plane indexing shows
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert os.path.exists(yolo_fastestv2_amd.LIB_PATH), "libyfv2.so not built"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _same(got, want, what):
    g = got.cpu().numpy() if torch.is_tensor(got) else got
    assert g.dtype == np.float32 and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d words differ, first at %s: %r vs %r" % (what, len(bad), g.size, bad[0].tolist(), g[tuple(bad[0])], want[tuple(bad[0])])


def _float_div(resized_u8):
    """``.permute(0, 3, 1, 2).float() / 255`` (train.py:101) of a resized uint8 batch, evaluated on the HOST: torch's CPU division is
    the IEEE-correct quotient the rule names.  On the device torch divides by a Python scalar by multiplying with fl32(1 / 255),
    which is one ulp off the quotient for 126 of the 256 bytes (3, 6, 7, 12, ...) - that product is not what the rule states."""
    return resized_u8.cpu().permute(0, 3, 1, 2).float() / 255


def _frames(dev, H, W, seed):
    """1 x 1, 2 x 3, 33 x 17 (h x w), the network's own size (an exact copy), 5 rows of 1921 pixels, and a crop view with
    row_pitch > 3 w at an odd byte address -> (frames, what they are)"""
    rng = np.random.default_rng(seed)
    shapes = [(1, 1), (2, 3), (33, 17), (H, W), (5, 1921)]
    frames = [torch.from_numpy(rng.integers(0, 256, s + (3,), dtype=np.uint8)).to(dev) for s in shapes]
    parent = torch.from_numpy(rng.integers(0, 256, (40, 51, 3), dtype=np.uint8)).to(dev)
    crop = parent[3:34, 8:31]                       # 31 x 23, pitch 153 > 69, first byte 3 * 153 + 24 = 483 past the (aligned) base
    assert crop.stride(0) == 153 > 3 * crop.shape[1] and crop.data_ptr() % 2 == 1
    frames.append(crop)
    return frames, ["%dx%d" % s for s in shapes] + ["crop 31x23"]


# ---- 1. all 256 table entries of every pair, ties included ---------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", PAIRS)
def test_every_byte_in_every_channel(yfv2, dev, alpha, beta):
    eng = yfv2.Engine(dev, 32, 32, max_batch=1, plan={})
    k = np.arange(1024, dtype=np.int64).reshape(32, 32)
    host = np.stack([(k + 85 * c) % 256 for c in range(3)], axis=-1).astype(np.uint8)
    assert all(len(np.unique(host[..., c])) == 256 for c in range(3))
    frame = torch.from_numpy(host).to(dev)
    resized = eng.resize_frames([frame])
    assert torch.equal(resized[0], frame), "a frame of the network's size is an exact copy"
    got = eng.train_batch_frames([frame], [alpha], [beta])
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 32, 32) and got.is_contiguous()
    want = tm.train_batch_ref(resized.cpu().numpy(), [alpha], [beta])
    _same(got, want, "pair (%g, %g)" % (alpha, beta))
    t = tm.table(alpha, beta)
    for c in range(3):                              # every entry of the table, per channel, straight from the statement
        assert np.array_equal(got[0, c].cpu().numpy(), t[host[..., c]])


# ---- 2. None is the identity ---------------------------------------------------------------------------------------------------
def test_none_is_one_zero_is_permute_float_div(yfv2, dev):
    eng = yfv2.Engine(dev, 64, 96, max_batch=8, plan={})
    frames, _ = _frames(dev, 64, 96, 21)
    B = len(frames)
    resized = eng.resize_frames(frames)
    a = eng.train_batch_frames(frames)
    b = eng.train_batch_frames(frames, [1.0] * B, [0.0] * B)
    assert torch.equal(a, b)
    assert torch.equal(a.cpu(), _float_div(resized))                           # train.py:101 on the transposed batch
    _same(a, tm.train_batch_ref(resized.cpu().numpy()), "identity")


# ---- 3. a pair per frame, every network size, B = 1, 3 and beyond max_batch -------------------------------------------------------
@pytest.mark.parametrize("H,W", NETS)
def test_pair_per_frame_equals_the_single_frame_call(yfv2, dev, H, W):
    frames, names = _frames(dev, H, W, 31 + H)
    B = len(frames)
    alpha = [PAIRS[(k + 1) % len(PAIRS)][0] for k in range(B)]
    beta = [PAIRS[(k + 1) % len(PAIRS)][1] for k in range(B)]
    eng = yfv2.Engine(dev, H, W, max_batch=1, plan={})
    ptrs = [f.data_ptr() for f in frames]
    got = eng.train_batch_frames(frames, alpha, beta)                          # B = 6 on a handle made for 1: max_batch grows
    assert eng.max_batch >= B and tuple(got.shape) == (B, 3, H, W)
    assert [f.data_ptr() for f in frames] == ptrs, "a frame was copied"
    resized = eng.resize_frames(frames).cpu().numpy()
    want = tm.train_batch_ref(resized, alpha, beta)
    for b in range(B):
        _same(got[b], want[b], "%d x %d, frame %d (%s), pair (%g, %g)" % (H, W, b, names[b], alpha[b], beta[b]))
        alone = eng.train_batch_frames([frames[b]], [alpha[b]], [beta[b]])    # B = 1
        assert torch.equal(alone[0], got[b]), (b, names[b])
    three = eng.train_batch_frames(frames[1:4], alpha[1:4], beta[1:4])         # B = 3
    assert torch.equal(three, got[1:4])
    k = names.index("%dx%d" % (H, W))                                          # the exact copy: the table of the frame's own bytes
    assert np.array_equal(got[k].cpu().numpy(), tm.table(alpha[k], beta[k])[frames[k].cpu().numpy()].transpose(2, 0, 1))


# ---- 4. decoder-format frames ----------------------------------------------------------------------------------------------------
def test_yuv_frames_odd_origin_odd_size(yfv2, dev):
    rng = np.random.default_rng(41)
    eng = yfv2.Engine(dev, 64, 96, max_batch=1, plan={})
    frames = []
    for fmt, name, colour in ((ym.NV12, "nv12", ym.BT709_LIMITED), (ym.I420, "i420", ym.BT601_FULL), (ym.NV12, "nv12", ym.BT601_LIMITED)):
        planes = ym.random_planes(rng, 58, 75, fmt)
        t = tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in planes)
        frames.append(yfv2.YuvFrame(t, name, colour, x0=3, y0=5, width=41, height=37))       # odd origin, odd size
    frames.append(yfv2.YuvFrame(frames[0].planes, "nv12", ym.BT709_FULL, x0=0, y0=0, width=1, height=1))
    B = len(frames)
    alpha, beta = [1.3, 0.5, 1.0, 1.75], [-7.25, 0.0, 0.5, 1.75]
    got = eng.train_batch_frames_yuv(frames, alpha, beta)
    resized = eng.resize_frames_yuv(frames)
    assert tuple(got.shape) == (B, 3, 64, 96)
    _same(got, tm.train_batch_ref(resized.cpu().numpy(), alpha, beta), "yuv")
    ident = eng.train_batch_frames_yuv(frames)
    assert torch.equal(ident.cpu(), _float_div(resized))
    # ... and through the B, G, R door: the model's conversion of the same rectangle, same pair
    bgr = [torch.from_numpy(ym.yuv_to_bgr([p.cpu().numpy() for p in f.planes], f.format, f.colour, f.x0, f.y0, f.width, f.height)).to(dev) for f in frames]
    assert torch.equal(got, eng.train_batch_frames(bgr, alpha, beta))


# ---- 5. out= -----------------------------------------------------------------------------------------------------------------------
def test_out_is_reused_and_its_tail_left_alone(yfv2, dev):
    eng = yfv2.Engine(dev, 32, 32, max_batch=4, plan={})
    frames, _ = _frames(dev, 32, 32, 51)
    out = torch.full((4, 3, 32, 32), SENTINEL, dtype=torch.float32, device=dev)
    first = eng.train_batch_frames(frames[:4], [1.3] * 4, [-7.25] * 4, out=out)
    assert first is out and not bool((out == SENTINEL).any())
    want4 = tm.train_batch_ref(eng.resize_frames(frames[:4]).cpu().numpy(), [1.3] * 4, [-7.25] * 4)
    _same(out, want4, "out, four frames")
    head = out[:2]
    assert eng.train_batch_frames(frames[4:6], [0.5, 1.0], [0.0, 0.5], out=head) is head      # fewer frames into the same memory
    want2 = tm.train_batch_ref(eng.resize_frames(frames[4:6]).cpu().numpy(), [0.5, 1.0], [0.0, 0.5])
    _same(out[:2], want2, "out, two frames")
    _same(out[2:], want4[2:], "the tail of out")
    with pytest.raises(ValueError):
        eng.train_batch_frames(frames[:2], out=out)                  # a wrong shape is refused, not sliced
    with pytest.raises(ValueError):
        eng.train_batch_frames(frames[:2], out=torch.empty((2, 3, 32, 32), dtype=torch.float16, device=dev))


# ---- 6. errors raise before anything is enqueued ---------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(yfv2, dev):
    from yolo_fastestv2_amd import _lib, datasets as ds
    eng = yfv2.Engine(dev, 32, 32, max_batch=2, plan={})
    frames, _ = _frames(dev, 32, 32, 61)
    limit = ds.max_frame_width(32)
    assert limit == (160 * 1024 - 1024 - 12 * 32) // 6 - 6 == 27066
    rng = np.random.default_rng(62)
    widest = torch.from_numpy(rng.integers(0, 256, (2, limit, 3), dtype=np.uint8)).to(dev)
    wider = torch.zeros((1, limit + 1, 3), dtype=torch.uint8, device=dev)
    out = torch.full((2, 3, 32, 32), SENTINEL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    for alpha, beta, words in (([1.0, nan], [0.0, 0.0], ["frame 1", "finite"]), ([1.0, 1.0], [inf, 0.0], ["frame 0", "finite"]),
                               ([-inf, 1.0], [0.0, 0.0], ["frame 0", "finite"])):
        with pytest.raises(_lib.Yfv2Error) as e:
            eng.train_batch_frames(frames[:2], alpha, beta, out=out)
        assert e.value.code == _lib.ERR_ARG and all(w in str(e.value) for w in words) and "yfv2_train_batch_frames_u8" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        eng.train_batch_frames(frames[:2], [1.0, 1.0], None, out=out)          # the Python layer refuses a lone alpha itself
    with pytest.raises(ValueError):
        eng.train_batch_frames(frames[:2], [1.0], [0.0], out=out)              # ... and a pair list of the wrong length
    with pytest.raises(_lib.Yfv2Error) as e:
        eng.train_batch_frames([frames[0], wider], out=out)
    assert e.value.code == _lib.ERR_ARG and "frame 1" in str(e.value) and "wider than %d" % limit in str(e.value), str(e.value)
    # the raw call: one of alpha / beta missing, a misaligned dst, NULL dst, B above max_batch, and the YUV door's own name
    L, h = _lib.lib(), eng._h
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    arr, keep = eng._frame_table(frames[:2])
    two = (C.c_float * 2)(1.0, 1.0)
    d0 = out.data_ptr()
    assert d0 % 16 == 0
    for a, b, dptr, B, code, words in ((two, None, d0, 2, _lib.ERR_ARG, ["both"]), (None, two, d0, 2, _lib.ERR_ARG, ["both"]),
                                       (None, None, d0 + 4, 2, _lib.ERR_ARG, ["16-byte aligned"]), (None, None, d0 + 8, 2, _lib.ERR_ARG, ["16-byte aligned"]),
                                       (None, None, None, 2, _lib.ERR_ARG, ["null pointer"]), (None, None, d0, 0, _lib.ERR_ARG, ["B < 1"]),
                                       (None, None, d0, 3, _lib.ERR_BATCH, ["max_batch=2"])):
        rc = L.yfv2_train_batch_frames_u8(h, arr, B, a, b, C.c_void_p(dptr) if dptr else None, st)
        msg = _lib.last_error(h)
        assert rc == code and all(w in msg for w in words) and "yfv2_train_batch_frames_u8" in msg, (words, rc, msg)
    assert L.yfv2_train_batch_frames_u8(h, None, 1, None, None, C.c_void_p(d0), st) == _lib.ERR_ARG
    yarr = (_lib.FrameYuv * 1)()
    assert L.yfv2_train_batch_frames_yuv(h, yarr, 1, None, None, C.c_void_p(d0), st) == _lib.ERR_ARG
    assert "yfv2_train_batch_frames_yuv" in _lib.last_error(h) and "frame 0" in _lib.last_error(h)
    ylimit = ds.max_frame_width(32, True)
    wide_y = yfv2.YuvFrame((torch.zeros((1, ylimit + 1), dtype=torch.uint8, device=dev), torch.zeros((1, ylimit + 2), dtype=torch.uint8, device=dev)), "nv12")
    with pytest.raises(_lib.Yfv2Error) as e:
        eng.train_batch_frames_yuv([wide_y], out=out[:1])
    assert e.value.code == _lib.ERR_ARG and "wider than %d" % ylimit in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a failed call wrote its output"
    # the handle is intact, and the widest frame it admits goes through
    got = eng.train_batch_frames([widest, frames[2]], [1.3, 1.0], [-7.25, 0.5], out=out)
    _same(got, tm.train_batch_ref(eng.resize_frames([widest, frames[2]]).cpu().numpy(), [1.3, 1.0], [-7.25, 0.5]), "widest frame")


# ---- 7. the batcher, and one training forward on its batch ------------------------------------------------------------------------------
def test_batcher_feeds_the_training_forward(yfv2, dev, coco_weights, images_u8):
    from yolo_fastestv2_amd import datasets as ds
    hwc = [np.ascontiguousarray(images_u8[k].transpose(1, 2, 0)) for k in range(2)]
    frames = [torch.from_numpy(hwc[0]).to(dev), torch.from_numpy(np.ascontiguousarray(np.repeat(hwc[1], 2, axis=1)[:300])).to(dev)]    # 352 x 352, 300 x 704
    labels = [np.array([[0, 3, 0.5, 0.5, 0.2, 0.3]], np.float32), np.zeros((0, 6), np.float32)]
    eng = yfv2.Engine(dev, 352, 352, max_batch=2, plan={})
    batcher = ds.TrainBatcher(eng, imgaug=True, rng=random.Random(7))
    imgs, targets = batcher(frames, labels)
    r = random.Random(7)
    drawn = [ds.draw_contrast_brightness(r) for _ in range(2)]
    alpha, beta = [p[0] for p in drawn], [p[1] for p in drawn]
    assert batcher.last_alpha == alpha and batcher.last_beta == beta
    assert torch.equal(imgs, eng.train_batch_frames(frames, alpha, beta))
    resized = eng.resize_frames(frames)
    want = tm.train_batch_ref(resized.cpu().numpy(), alpha, beta)
    _same(imgs, want, "batcher")
    assert targets.device == imgs.device and targets.dtype == torch.float32 and torch.equal(targets.cpu(), ds.collate_targets(labels))
    # the validation loader's form: no draws, the identity
    state = r.getstate()
    plain = ds.TrainBatcher(eng, imgaug=False, rng=r)(frames, labels)[0]
    assert r.getstate() == state and torch.equal(plain.cpu(), _float_div(resized))
    # one train-mode forward on the batch, against the same forward on the tensor torch builds from the statement's bytes
    model = yfv2.Detector(80, 3, True).to(dev)
    model.load_state_dict(coco_weights)
    model.train()
    built = torch.from_numpy(want).to(dev)                      # = (table applied on the host).permute.float()/255, bit for bit
    assert torch.equal(built, imgs)
    a = [p.detach().clone() for p in model(imgs)]
    teng = model.engine_for(imgs, sync=False)
    b = [p.detach().clone() for p in teng.train_forward(built)]
    assert len(a) == 6 and all(torch.isfinite(p).all() for p in a)
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)
