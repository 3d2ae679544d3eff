"""The handle's growable device blocks (csrc/yfv2_ctx.h DeviceBlock): loss, AP, k-means and tile workspaces, the two first-use buffers.

One engine at 352x352 with max_batch 4 serves every case, in file order.  Each case makes a small call, a call large enough to
force the block to grow (free + allocate behind a device wait), and the small call again; every result must equal, bit for bit,
the same call on a fresh engine whose block was sized by that call alone.  What a fresh engine returns is pinned to the reference
or its numpy model by test_loss.py, test_gpu_ap*.py, test_gpu_anchors.py, test_gpu_tiles.py and test_gpu_frames.py; this file adds
that a block's history changes no bit.  The last case destroys the engine that has grown everything.
"""
import os

import numpy as np
import pytest
import torch

from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu

MAX_DET = 300


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert os.path.exists(yolo_fastestv2_amd.LIB_PATH), "libyfv2.so not built"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fresh(yfv2, dev, cfg, coco_weights):
    """a new engine of the shared configuration (weights only where the call runs the network)"""
    def make(weights=False):
        eng = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=4, plan={})
        if weights:
            eng.load_state_dict(coco_weights)
        return eng
    return make


@pytest.fixture(scope="module")
def engine(fresh):
    eng = fresh(weights=True)
    eng.first_generation = eng._generation
    return eng


def bits(t):
    a = np.atleast_1d(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def same(got, want, what):
    """nested tuples / lists / dicts of tensors, arrays and numbers, bit for bit"""
    if isinstance(want, dict):
        assert set(got) == set(want), what
        for k in want:
            same(got[k], want[k], "%s[%s]" % (what, k))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, "%s[%d]" % (what, i))
    elif want is None:
        assert got is None, what
    else:
        assert np.array_equal(bits(got), bits(want)), "%s differs" % what


def grow_and_return(engine, fresh, small, large, what, weights=False):
    """small, large, small on the shared engine against each call alone on an engine of its own"""
    want_small, want_large = small(fresh(weights)), large(fresh(weights))
    same(small(engine), want_small, what + ": small call")
    same(large(engine), want_large, what + ": large call (the block grows)")
    same(small(engine), want_small, what + ": small call in the grown block")
    assert engine._generation == engine.first_generation, "the shared engine was re-created"


def test_loss_workspace(engine, fresh, dev):
    rng = np.random.default_rng(11)
    preds = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev) for s in engine.logit_shapes(2)]

    def labels(T):
        """[image, class, cx, cy, w, h], normalised.  The reg / cls gradients of matches that share a cell meet in float atomics, whose
        order is not fixed: random labels differ in the last bit from run to run on one engine (measured: up to ten words of 2^-31 at
        T = 64, on the parent commit as well).  So that "the same bits" is defined, no two matches here share a cell: per image 23
        boxes of 14 x 20 pixels (within a factor 2 of the first stride-16 anchor only) on a lattice 3.5 cells apart on the 22 x 22
        map, and 9 of 130 x 100 pixels (the first stride-32 anchor only) 3.5 cells apart on the 11 x 11 map; a match and its two
        neighbour cells stay more than a cell away from the next label's."""
        r = np.random.default_rng(100 + T)
        rows = []
        for k in range(T):
            j = k // 2
            if j < 23:
                rows.append([k % 2, r.integers(0, 80), (2.3 + 3.5 * (j % 6)) / 22.0, (2.7 + 3.5 * (j // 6)) / 22.0, 14 / 352.0, 20 / 352.0])
            else:
                rows.append([k % 2, r.integers(0, 80), (1.3 + 3.5 * ((j - 23) % 3)) / 11.0, (1.7 + 3.5 * ((j - 23) // 3)) / 11.0, 130 / 352.0, 100 / 352.0])
        return np.asarray(rows, np.float32)

    def call(T):
        return lambda eng: eng.loss(preds, torch.from_numpy(labels(T)), want_grad=True)
    grow_and_return(engine, fresh, call(1), call(64), "loss with gradients, B = 2, T = 1 / 64")


def _ap_inputs(dev, N, T, seed):
    r = np.random.default_rng(seed)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    mask = r.integers(0, 8, N)
    conf = np.round(r.uniform(0.01, 1.0, N), 2)     # two decimals: plenty of equal confidences
    return to(mask, torch.int32), to(conf, torch.float32), to(r.integers(0, 20, N), torch.float32), to(r.integers(0, 20, T), torch.float32)


def test_ap_workspace(engine, fresh, dev):
    def call(N, T):
        mask, conf, cls, labels = _ap_inputs(dev, N, T, N)
        return lambda eng: (eng.ap_per_class(mask & 1, conf, cls, labels), eng.ap_per_class_multi(mask, conf, cls, labels, 3))
    grow_and_return(engine, fresh, call(10, 5), call(5000, 700), "AP and AP-multi (K = 3), N = 10 / 5000, T = 5 / 700")


def test_kmeans_workspace(engine, fresh, dev):
    def call(N, k):
        r = np.random.default_rng(N)
        wh = torch.from_numpy(r.uniform(4.0, 300.0, (N, 2))).to(dev)
        c0 = wh[torch.from_numpy(r.choice(N, k, replace=False)).to(dev)].clone()

        def run(eng):
            cent, assign, avg, info = eng.anchor_kmeans(wh, c0, want_assign=False)   # the assignments live in the workspace
            return cent, assign, avg, info
        return run
    grow_and_return(engine, fresh, call(100, 3), call(5000, 6), "k-means without assignments, N = 100 / 5000 (k = 6)")


def test_tile_workspace(engine, fresh, dev):
    def call(T, F):
        r = np.random.default_rng(10 * T + F)
        td = np.zeros((T, MAX_DET, 6), np.float32)
        tc = r.integers(1, 40, T).astype(np.int32)
        for k in range(T):
            xy = r.uniform(0, 250, (tc[k], 2))
            td[k, :tc[k], 0:2] = xy
            td[k, :tc[k], 2:4] = xy + r.uniform(10, 100, (tc[k], 2))
            td[k, :tc[k], 4] = np.sort(r.uniform(0.3, 1.0, tc[k]))[::-1]      # NMS output: descending confidence
            td[k, :tc[k], 5] = r.integers(0, 3, tc[k])
        tiles = [(k * F // T, 100 * (k % 2), 50 * (k % 3), 352, 352) for k in range(T)]     # frame non-decreasing, overlapping tiles
        tdd, tcd = torch.from_numpy(td).to(dev), torch.from_numpy(tc).to(dev)

        def run(eng):
            out = eng.new_tiled_buffers(F)
            for t, fill in zip(out, (-12345.0, -7, -9)):
                t.fill_(fill)
            return eng.merge_tiles(tdd, tcd, tiles, F, 0.4, out=out)
        return run
    grow_and_return(engine, fresh, call(2, 1), call(6, 3), "merge_tiles, T = 2 / 6, F = 1 / 3")


def test_first_use_buffers(engine, fresh, dev, images_u8):
    """detect_frames allocates the resized batch, detect_tiled its per-tile results (and grows the tile workspace to max_batch tiles):
    detect_frames, detect_tiled of two 500x700 frames, detect_frames again - the third result is the first, and each is a fresh engine's"""
    pic = lambda k, h, w: torch.from_numpy(oracle.resize_linear_u8(np.ascontiguousarray(images_u8[k].transpose(1, 2, 0)), w, h)).to(dev)   # reference picture k at h x w
    small_frames = [pic(0, 300, 420), pic(1, 352, 352)]
    big_frames = [pic(2, 500, 700), pic(3, 500, 700)]
    tiles = [(f, x0, 0, 400, 500) for f in range(2) for x0 in (0, 300)]      # four tiles: max_batch, the engine is not re-created

    def frames(eng):
        d, i, c = eng.detect_frames(small_frames, 0.3, 0.4)
        n = c.cpu().numpy()
        return [d[b, :n[b]] for b in range(2)], [i[b, :n[b]] for b in range(2)], c

    def tiled(eng):
        out = eng.new_tiled_buffers(2)
        for t, fill in zip(out, (-12345.0, -7, -9)):
            t.fill_(fill)
        return eng.detect_tiled(big_frames, tiles=tiles, conf_thres=0.3, iou_thres=0.4, out=out)
    grow_and_return(engine, fresh, frames, tiled, "detect_frames / detect_tiled / detect_frames", weights=True)
    assert int(frames(engine)[2].sum()) > 0, "the frames must produce detections for the comparison to mean anything"


def test_destroying_the_engine_that_grew_every_block(engine, dev):
    """the blocks release themselves in the handle's destructor, on its device: destroy returns, and the device still works"""
    assert engine._generation == engine.first_generation
    torch.cuda.synchronize(dev)
    engine.close()
    assert engine._h is None
    torch.cuda.synchronize(dev)
    assert float(torch.ones(8, device=dev).sum()) == 8.0
