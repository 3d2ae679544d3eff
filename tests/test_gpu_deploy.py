"""GPU tests of the ncnn sample's deployment path (include/yfv2.h yfv2_export_maps, yfv2_deploy_post,
yfv2_detect_deploy_frames_u8).  Run with ``-m gpu`` on an MI355X.

The claims: export_maps writes the layout of Detector(export_onnx=True) with obj / class channels that are the bits of
Engine.decode's columns; deploy_post returns, bit for bit, what the reference's compiled sample returned on the cases of
golden_deploy.npz and what tests/deploy_model.py (the numpy statement of the rule, itself checked against those goldens on the
host) returns on fresh maps - batches, per-image scales, ties, the 4096-row limit, truncation at max_out and dropped rows
included; detect_deploy_frames equals its four steps called one after the other; the C++ class returns the same boxes.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import deploy_model as dm
from conftest import GOLDEN
from test_gpu_parity import DECODE_ULP, _ulp_distance

pytestmark = pytest.mark.gpu

COCO_ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]


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
def golden_deploy():
    return dict(np.load(os.path.join(GOLDEN, "golden_deploy.npz"), allow_pickle=False))


_ENGINES = {}


def _engine(yfv2, dev, h, w, classes, anchors=COCO_ANCHORS, max_batch=1):
    """one weightless engine per configuration (export_maps / deploy_post need no weights)"""
    key = (h, w, classes, tuple(float(a) for a in anchors))
    if key not in _ENGINES:
        _ENGINES[key] = yfv2.Engine(dev, h, w, classes, 3, anchors=[float(a) for a in anchors], max_batch=max_batch, plan={})
    return _ENGINES[key]


def _random_maps(rng, B, h, w, classes, obj_lo=0.0, spread=1.0):
    maps = []
    for d in (16, 32):
        fh, fw = h // d, w // d
        reg = (0.5 + spread * (rng.random((B, fh, fw, 12)) - 0.5)).astype(np.float32)
        obj = (obj_lo + (1 - obj_lo) * rng.random((B, fh, fw, 3))).astype(np.float32)
        e = np.exp(3 * rng.standard_normal((B, fh, fw, classes))).astype(np.float32)
        maps.append(np.concatenate([reg, obj, (e / e.sum(-1, keepdims=True)).astype(np.float32)], -1))
    return maps


def _post(eng, dev, maps, thresh, nms, scale=None, max_out=None):
    """deploy_post on host maps into sentinel-filled buffers -> host (boxes, count, dropped)"""
    B = maps[0].shape[0]
    out = eng.new_deploy_buffers(B, max_out)
    out[0].fill_(-77)
    out[1].fill_(-9)
    sc = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale, np.float32)).to(dev)
    boxes, cnt = eng.deploy_post(torch.from_numpy(maps[0]).to(dev), torch.from_numpy(maps[1]).to(dev), float(thresh), float(nms), scale=sc,
                                 max_out=max_out, out=out)
    dropped = eng.deploy_dropped()
    return boxes.cpu().numpy(), cnt.cpu().numpy(), dropped


def _assert_same(got, want, what):
    gb, gc, gd = got
    wb, wc, wd = want
    assert np.array_equal(gc, wc), "%s: counts %s vs %s" % (what, gc.tolist(), wc.tolist())
    bad = np.argwhere(gb != wb)
    assert bad.size == 0, "%s: %d words differ, first at %s: %d vs %d" % (what, len(bad), bad[0].tolist(), gb[tuple(bad[0])], wb[tuple(bad[0])])
    assert gd == wd, "%s: dropped %d vs %d" % (what, gd, wd)


# ---- 1. export maps ----------------------------------------------------------------------------------------------------
# 32x32 at 1 and 5 classes, 64x96 at 80, 352x352 at batch 2 (several workgroups per scale, a partial last one); classes 1, 3, 4
# and 95 give 16, 18, 19 and 110 floats per pixel: every remainder of the 16-byte store width; 255 classes: the wide softmax form
@pytest.mark.parametrize("h,w,classes,B", [(32, 32, 1, 2), (32, 32, 5, 2), (64, 96, 80, 3), (352, 352, 80, 2), (32, 32, 3, 1), (32, 32, 4, 3),
                                           (96, 64, 95, 2), (64, 64, 255, 1)])
def test_export_maps_layout_and_bits(yfv2, dev, h, w, classes, B):
    eng = _engine(yfv2, dev, h, w, classes)
    g = torch.Generator().manual_seed(h * 1000 + w + classes)
    preds = [(3 * torch.randn(s, generator=g)).to(dev) for s in eng.logit_shapes(B)]
    m0, m1 = eng.export_maps(preds)
    dec = eng.decode(preds).cpu().numpy()
    C5 = 15 + classes
    assert tuple(m0.shape) == (B, h // 16, w // 16, C5) and tuple(m1.shape) == (B, h // 32, w // 32, C5)    # detector.py:43-44
    assert m0.is_contiguous() and m1.is_contiguous()
    row0 = 0
    for s, m in enumerate((m0.cpu().numpy(), m1.cpu().numpy())):
        fh, fw = m.shape[1], m.shape[2]
        d = dec[:, row0:row0 + 3 * fh * fw].reshape(B, fh, fw, 3, 5 + classes)             # rows (y, x, a)
        row0 += 3 * fh * fw
        assert np.array_equal(m[..., 12:15].view(np.uint32), d[..., 4].view(np.uint32)), "scale %d: obj bits differ from decode" % s
        for a in range(3):
            assert np.array_equal(m[..., 15:].view(np.uint32), d[..., a, 5:].view(np.uint32)), "scale %d: class bits differ from decode" % s
        ref = torch.sigmoid(preds[3 * s].cpu()).permute(0, 2, 3, 1).numpy()
        worst = int(_ulp_distance(m[..., :12], ref).max())
        print("export_maps %dx%d c%d scale %d: reg within %d ulp of torch.sigmoid" % (h, w, classes, s, worst))
        assert worst <= DECODE_ULP["obj"], worst
    # the torch glue of Detector.forward(export_onnx=True) gives the same layout (values to rounding)
    r2, o2, c2 = preds[:3]
    glue = torch.cat((r2.sigmoid(), o2.sigmoid(), torch.softmax(c2, 1)), 1).permute(0, 2, 3, 1)
    assert float((glue - m0).abs().max()) < 1e-5


def test_export_maps_into_an_unaligned_buffer(yfv2, dev):
    """the maps may start at any dword: the span of every workgroup finds its own 16-byte boundary; nothing outside is written"""
    eng = _engine(yfv2, dev, 64, 96, 80)
    B = 2
    g = torch.Generator().manual_seed(5)
    preds = [(3 * torch.randn(s, generator=g)).to(dev) for s in eng.logit_shapes(B)]
    want = [m.cpu() for m in eng.export_maps(preds)]
    for off in (1, 2, 3):
        bufs = [torch.full((int(np.prod(s)) + 8,), -5.0, device=dev) for s in eng.map_shapes(B)]
        outs = [b[off:off + int(np.prod(s))].view(s) for b, s in zip(bufs, eng.map_shapes(B))]
        eng.export_maps(preds, out=outs)
        for b, o, wnt, s in zip(bufs, outs, want, eng.map_shapes(B)):
            assert torch.equal(o.cpu(), wnt)
            guard = torch.cat((b[:off], b[off + int(np.prod(s)):])).cpu()
            assert (guard == -5.0).all()


# ---- 2. deploy_post ----------------------------------------------------------------------------------------------------
def _case(z, c):
    in_h, in_w, classes = (int(v) for v in z[c + "_hw"])
    thresh, nms, sw, sh = (np.float32(v) for v in z[c + "_par"])
    return in_h, in_w, classes, z[c + "_anchors"], thresh, nms, sw, sh


def test_deploy_post_equals_the_compiled_sample(yfv2, dev, golden_deploy):
    z = golden_deploy
    for c in (str(c) for c in z["cases"]):
        in_h, in_w, classes, anchors, thresh, nms, sw, sh = _case(z, c)
        eng = _engine(yfv2, dev, in_h, in_w, classes, anchors)
        maps = [np.ascontiguousarray(z[c + "_map0"][None]), np.ascontiguousarray(z[c + "_map1"][None])]
        boxes, cnt, dropped = _post(eng, dev, maps, thresh, nms, scale=np.float32([[sw, sh]]))
        want = z[c + "_rec"]
        assert int(cnt[0]) == len(want) and dropped == 0, (c, int(cnt[0]), len(want), dropped)
        assert np.array_equal(boxes[0, :len(want)], want), "%s: record %s differs" % (c, np.argwhere(boxes[0, :len(want)] != want)[:1].tolist())
        assert (boxes[0, len(want):] == 0).all(), c


@pytest.mark.parametrize("B", [1, 3, 17])
def test_deploy_post_equals_the_model_on_fresh_maps(yfv2, dev, golden_deploy, B):
    """every golden case's configuration, fresh seeded maps, per-image scales"""
    z = golden_deploy
    for k, c in enumerate(str(c) for c in z["cases"]):
        in_h, in_w, classes, anchors, thresh, nms, _, _ = _case(z, c)
        if in_h == 352:
            thresh = np.float32(0.2)        # (random maps have ~1800 candidates at 0.01; the model's Python walk is the cost)
        eng = _engine(yfv2, dev, in_h, in_w, classes, anchors)
        rng = np.random.default_rng(1000 * B + k)
        maps = _random_maps(rng, B, in_h, in_w, classes, obj_lo=0.3 if "dense" in c else 0.0, spread=0.3 if "dense" in c else 1.0)
        scale = (0.5 + 2 * rng.random((B, 2))).astype(np.float32)
        got = _post(eng, dev, maps, thresh, nms, scale=scale)
        want = dm.deploy_batch(maps[0], maps[1], anchors, in_h, thresh, nms, scale=scale)
        assert want[1].sum() > 0, c
        _assert_same(got, want, "%s B=%d" % (c, B))


def test_deploy_post_all_rows_pass_at_the_row_limit_and_truncation(yfv2, dev):
    """512x512: 3840 rows, thresh 0 - every row is a candidate; then max_out < count keeps the first max_out and the full count"""
    eng = _engine(yfv2, dev, 512, 512, 2)
    assert eng.rows == 3840
    rng = np.random.default_rng(21)
    maps = _random_maps(rng, 2, 512, 512, 2, obj_lo=0.3, spread=0.3)
    want = dm.deploy_batch(maps[0], maps[1], COCO_ANCHORS, 512, 0.0, 0.25)
    got = _post(eng, dev, maps, 0.0, 0.25)
    _assert_same(got, want, "3840 candidates")
    # nothing suppressed (nms 2): all 3840 survive, in score order
    want_all = dm.deploy_batch(maps[0][:1], maps[1][:1], COCO_ANCHORS, 512, 0.0, 2.0)
    assert int(want_all[1][0]) == 3840
    _assert_same(_post(eng, dev, [maps[0][:1], maps[1][:1]], 0.0, 2.0), want_all, "3840 survivors")
    n = int(want[1].min())
    assert n > 40
    for max_out in (1, 40):
        got = _post(eng, dev, maps, 0.0, 0.25, max_out=max_out)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0][:, :max_out])
    # fewer survivors than max_out: the tail is zeroed, not left as it was
    few = dm.deploy_batch(maps[0], maps[1], COCO_ANCHORS, 512, 0.93, 0.25)
    got = _post(eng, dev, maps, 0.93, 0.25, max_out=256)
    assert 0 < int(few[1].max()) < 256 and np.array_equal(got[1], few[1]) and np.array_equal(got[0], few[0][:, :256])


def test_deploy_post_drops_and_counts_rows_without_a_representable_box(yfv2, dev):
    """a NaN / infinite reg value in the INPUT map (data): the sample's (int) is undefined there; the row is dropped and counted"""
    eng = _engine(yfv2, dev, 64, 96, 5)
    rng = np.random.default_rng(8)
    maps = _random_maps(rng, 3, 64, 96, 5, obj_lo=0.5)
    maps[0][0, 1, 2, 0] = np.nan          # anchor 0 of a cell: x centre
    maps[0][1, 3, 5, 6] = np.inf          # anchor 1: width
    maps[1][2, 0, 1, 11] = -np.inf        # anchor 2, scale 1: height
    maps[0][2, 0, 0, 2] = 3e5             # finite, but (2 v)^2 * anchor * scale leaves int32
    scale = np.float32([[1, 1], [1.5, 0.75], [2000, 1]])
    want = dm.deploy_batch(maps[0], maps[1], COCO_ANCHORS, 64, 0.05, 0.25, scale=scale)
    assert want[2] == 4
    got = _post(eng, dev, maps, 0.05, 0.25, scale=scale)
    _assert_same(got, want, "dropped rows")
    # the word is per call: a clean call reads 0 again
    clean = _random_maps(rng, 3, 64, 96, 5)
    assert _post(eng, dev, clean, 0.05, 0.25)[2] == 0


def test_deploy_post_ranks_equal_scores_by_candidate_order(yfv2, dev):
    """cells copied within and across the two scales and across anchors: many equal scores, same class, overlapping boxes"""
    eng = _engine(yfv2, dev, 128, 128, 2)
    rng = np.random.default_rng(4)
    maps = _random_maps(rng, 2, 128, 128, 2, obj_lo=0.3, spread=0.2)
    for m in maps:
        m[:, :, 1::2] = m[:, :, 0::2]                    # every second column repeats its neighbour
        m[..., 13] = m[..., 12]                          # anchor 1's objectness = anchor 0's
    maps[1][:, :, :, 12:] = maps[0][:, ::2, ::2, 12:]    # the coarse map repeats scores of the fine one
    for nms in (0.25, 2.0):
        want = dm.deploy_batch(maps[0], maps[1], COCO_ANCHORS, 128, 0.0, nms)
        score = want[0][0, :want[1][0], 5].view(np.float32)
        assert (np.diff(score) == 0).sum() > 10           # the survivors themselves contain ties
        _assert_same(_post(eng, dev, maps, 0.0, nms), want, "ties nms=%g" % nms)


def test_deploy_argument_checks(yfv2, dev):
    from yolo_fastestv2_amd import _lib as m
    eng = _engine(yfv2, dev, 64, 96, 5)
    L = m.lib()
    maps = [torch.zeros(s, device=dev) for s in eng.map_shapes(1)]
    boxes, cnt = eng.new_deploy_buffers(1)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda thresh, max_out, B=1, b=boxes: L.yfv2_deploy_post(eng._h, p(maps[0]), p(maps[1]), B, None, thresh, 0.25, p(b) if b is not None else None,
                                                                   p(cnt), max_out, None)
    assert call(-0.1, 1) == m.ERR_ARG and "thresh" in m.last_error(eng._h)
    assert call(float("nan"), 1) == m.ERR_ARG
    assert call(0.3, 0) == m.ERR_ARG and call(0.3, eng.rows + 1) == m.ERR_ARG
    assert call(0.3, 1, b=None) == m.ERR_ARG
    assert call(0.3, 1, B=0) == m.ERR_BATCH and call(0.3, 1, B=eng.max_batch + 1) == m.ERR_BATCH
    assert L.yfv2_export_maps(eng._h, None, 1, p(maps[0]), p(maps[1]), None) == m.ERR_ARG
    assert L.yfv2_detect_deploy_frames_u8(eng._h, None, 1, 0.3, 0.25, p(boxes), p(cnt), 1, None) == m.ERR_STATE      # no weights
    assert call(0.3, eng.rows) == m.OK
    torch.cuda.synchronize(dev)
    with pytest.raises(ValueError):
        eng.deploy_post(maps[0], maps[1], max_out=0)


# ---- 3. detect_deploy_frames --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coco_engine(yfv2, dev, cfg, coco_weights):
    eng = yfv2.Engine(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=4, plan={})
    eng.load_state_dict(coco_weights)
    return eng


def _frames(images_u8, dev):
    from oracle import yfv2_oracle as oracle
    out = []
    for k, (h, w) in enumerate([(480, 640), (352, 352), (353, 517), (720, 1280)]):
        hwc = np.ascontiguousarray(images_u8[k % len(images_u8)].transpose(1, 2, 0))
        out.append(torch.from_numpy(oracle.resize_linear_u8(hwc, w, h)).to(dev))
    return out


@pytest.mark.parametrize("thresh,nms", [(0.3, 0.25), (0.01, 0.25)])
def test_detect_deploy_frames_is_its_four_steps(yfv2, dev, coco_engine, images_u8, thresh, nms):
    eng = coco_engine
    frames = _frames(images_u8, dev)
    out = eng.new_deploy_buffers(len(frames))
    out[0].fill_(-77)
    boxes, cnt = eng.detect_deploy_frames(frames, thresh, nms, out=out)
    got = (boxes.cpu().numpy(), cnt.cpu().numpy())
    assert eng.deploy_dropped() == 0 and not eng.nonfinite()
    m0, m1 = eng.export_maps(eng.forward(eng.resize_frames(frames)))
    scale = torch.tensor([[np.float32(f.shape[1]) / np.float32(eng.width), np.float32(f.shape[0]) / np.float32(eng.height)] for f in frames],
                         dtype=torch.float32, device=dev)
    b2, c2 = eng.deploy_post(m0, m1, thresh, nms, scale=scale)
    assert np.array_equal(got[1], c2.cpu().numpy()) and int(got[1].min()) > 0
    assert np.array_equal(got[0], b2.cpu().numpy())
    # ... and the numpy model agrees on those maps
    want = dm.deploy_batch(m0.cpu().numpy(), m1.cpu().numpy(), eng.anchors, eng.height, thresh, nms, scale=scale.cpu().numpy())
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    # the Python entry point returns the same records as tuples
    lists = yfv2.ncnn_sample.detection(eng, frames, thresh, nms)
    for b, lst in enumerate(lists):
        assert len(lst) == int(got[1][b])
        for k, t in enumerate(lst):
            assert t[:5] == tuple(int(v) for v in got[0][b, k, :5]) and np.float32(t[5]).view(np.int32) == got[0][b, k, 5]


def test_pipeline_submit_deploy_frames(yfv2, dev, cfg, coco_weights, coco_engine, images_u8):
    frames = _frames(images_u8, dev)[:2]
    pipe = yfv2.DetectPipeline(dev, cfg["height"], cfg["width"], cfg["classes"], cfg["anchor_num"], anchors=cfg["anchors"], max_batch=2, depth=2, plan={})
    pipe.load_state_dict(coco_weights)
    torch.cuda.synchronize(dev)
    t = pipe.submit_deploy_frames(frames, 0.3, 0.25, max_out=50)
    boxes, cnt = pipe.result(t, host=True)
    wb, wc = coco_engine.detect_deploy_frames(frames, 0.3, 0.25, max_out=50)
    assert torch.equal(boxes.cpu(), wb.cpu()) and torch.equal(cnt.cpu(), wc.cpu())


# ---- 4. the C++ class -----------------------------------------------------------------------------------------------------
def test_cpp_detection_ncnn_matches_python(yfv2, dev, cfg, coco_weights, coco_engine, images_u8, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "yfv2_deploy_test")
    if not os.path.exists(exe):      # normally prebuilt by __graft_entry__.build() and shipped with the tree
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(exe), "tests/cpp/yfv2_deploy_test missing: run __graft_entry__.build()"
    wpath = str(tmp_path / "coco.yfv2w")
    assert yfv2.export_weights(coco_weights, wpath) > 0
    frame = _frames(images_u8, dev)[0]
    ipath = str(tmp_path / "frame.raw")
    frame.cpu().numpy().tofile(ipath)
    anchors = ",".join(repr(float(a)) for a in cfg["anchors"])
    r = subprocess.run([exe, wpath, anchors, ipath, str(frame.shape[1]), str(frame.shape[0]), "0.3", "0.25"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = [[int(v) for v in ln.split()] for ln in r.stdout.strip().splitlines() if ln.strip()]
    want = yfv2.ncnn_sample.detection(coco_engine, [frame], 0.3, 0.25)[0]
    assert len(want) > 0 and len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g[:5]) == w[:5] and np.uint32(g[5]) == np.float32(w[5]).view(np.uint32)
