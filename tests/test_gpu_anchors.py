"""GPU tests of anchor k-means: Engine.anchor_kmeans / yolo_fastestv2_amd.genanchors (include/yfv2.h yfv2_anchor_kmeans,
csrc/yfv2_anchors.hip).  Run with ``-m gpu`` on an MI355X.

The claims: on every golden case the device assigns EVERY point as the reference's own genanchors.py does (the goldens' gap
condition leaves no exemption), takes the same number of passes, and its centroids and average IoU are within 1e-12 relative
of the reference's and BIT-IDENTICAL to the numpy model of the kernels' summation order (tests/anchors_model.py); a repeated
call and another iteration group size change no bit; empty clusters, bad input, max_iter and bad arguments are reported as
include/yfv2.h says.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import anchors_model as am

pytestmark = pytest.mark.gpu


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
def engine(yfv2, dev):
    return yfv2.Engine(dev, 64, 64, classes=2, plan={})   # any configuration will do; no weights, no anchors


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(am.GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def cases(golden):
    """case index -> (X, initial centroids, golden, model result), each computed once and left unchanged"""
    cache = {}

    def get(i, with_model=True):
        if i not in cache:
            X, C0, g = am.load_case(golden, i)
            cache[i] = [X, C0, g, None]
        if with_model and cache[i][3] is None:
            cache[i][3] = am.kmeans(cache[i][0], cache[i][1])
        return cache[i]
    return get


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def run(engine, dev, X, C0, **kw):
    cent, assign, avg, info = engine.anchor_kmeans(torch.from_numpy(X).to(dev), torch.from_numpy(np.ascontiguousarray(C0)).to(dev), **kw)
    return cent.cpu().numpy(), None if assign is None else assign.cpu().numpy(), float(avg.cpu()), info


@pytest.mark.parametrize("i", range(len(am.CASES)))
def test_every_golden_case_matches_the_reference_and_the_model_bit_for_bit(engine, dev, cases, i):
    X, C0, g, m = cases(i)
    cent, assign, avg, info = run(engine, dev, X, C0)
    assert info == {"iterations": int(g["iterations"]), "converged": 1, "empty_cluster": -1, "bad_input": 0}
    differing = int((assign != g["assign"].astype(np.int32)).sum())
    print("case %s: %d passes, %d of %d assignments differ from the reference, centroid error %.3g relative, avg IoU error %.3g relative"
          % (am.CASES[i], info["iterations"], differing, len(X), np.max(np.abs(cent - g["centroids"]) / np.abs(g["centroids"])),
             abs(avg - float(g["avg_iou"])) / float(g["avg_iou"])))
    assert differing == 0
    assert np.all(np.abs(cent - g["centroids"]) <= 1e-12 * np.abs(g["centroids"]))
    assert abs(avg - float(g["avg_iou"])) <= 1e-12 * float(g["avg_iou"])
    assert np.array_equal(bits(cent), bits(m["centroids"]))
    assert bits(avg) == bits(m["avg_iou"])
    assert m["iterations"] == info["iterations"] and np.array_equal(m["assign"], assign)


def test_repeated_calls_and_other_group_sizes_change_no_bit(engine, dev, cases):
    X, C0, g, _ = cases(4, with_model=False)
    first = run(engine, dev, X, C0)
    try:
        for group in (8, 1, 3, 64):
            engine.debug_kmeans_group(group)
            cent, assign, avg, info = run(engine, dev, X, C0)
            assert info == first[3] and info["iterations"] == int(g["iterations"])
            assert np.array_equal(bits(cent), bits(first[0])) and np.array_equal(assign, first[1]) and bits(avg) == bits(first[2])
    finally:
        engine.debug_kmeans_group(8)


def test_the_input_tensors_are_left_alone_and_assignments_are_optional(engine, dev, cases):
    X, C0, g, m = cases(2)
    x_t, c_t = torch.from_numpy(X).to(dev), torch.from_numpy(C0.copy()).to(dev)
    cent, assign, avg, info = engine.anchor_kmeans(x_t, c_t, want_assign=False)   # assign = NULL at the C ABI
    assert assign is None and info["converged"] == 1 and info["iterations"] == int(g["iterations"])
    assert np.array_equal(c_t.cpu().numpy(), C0) and np.array_equal(x_t.cpu().numpy(), X)
    assert np.array_equal(bits(cent.cpu().numpy()), bits(m["centroids"])) and bits(float(avg.cpu())) == bits(m["avg_iou"])


def test_wh_at_an_address_that_is_8_but_not_16_byte_aligned(engine, dev, cases):
    X, C0, g, m = cases(7)
    buf = torch.zeros(2 * len(X) + 1, dtype=torch.float64, device=dev)
    view = buf[1:].view(-1, 2)
    view.copy_(torch.from_numpy(X))
    assert view.data_ptr() % 16 == 8
    cent, assign, avg, info = engine.anchor_kmeans(view, torch.from_numpy(C0.copy()).to(dev))
    assert info["converged"] == 1 and np.array_equal(bits(cent.cpu().numpy()), bits(m["centroids"]))
    assert np.array_equal(assign.cpu().numpy(), m["assign"])


def test_two_identical_initial_centroids_report_the_empty_cluster(yfv2, engine, dev, cases, tmp_path):
    X, C0, _, _ = cases(1, with_model=False)
    C0 = C0.copy()
    C0[1] = C0[0]
    cent, assign, avg, info = run(engine, dev, X, C0)
    assert info["empty_cluster"] == 1 and info["converged"] == 0 and info["bad_input"] == 0 and info["iterations"] == 1
    assert np.isfinite(cent).all() and np.array_equal(cent, C0)   # the last completed update: none
    assert not (assign == 1).any() and np.isfinite(avg)
    before = C0.copy()
    with pytest.raises(ValueError, match="cluster 1"):
        yfv2.genanchors.kmeans(X, C0, 0.005, str(tmp_path / "anchors6.txt"), 352, 352, device=dev)
    assert np.array_equal(C0, before) and not (tmp_path / "anchors6.txt").exists()


@pytest.mark.parametrize("value", [0.0, -0.25, float("nan"), float("inf")])
@pytest.mark.parametrize("where", [(0, 0), (1029, 1)])
def test_a_width_or_height_that_is_not_a_positive_finite_number_is_bad_input(yfv2, engine, dev, cases, tmp_path, value, where):
    X, C0, _, _ = cases(3, with_model=False)
    X = X.copy()
    X[where] = value
    cent, assign, avg, info = run(engine, dev, X, C0)
    assert info["bad_input"] == 1 and info["converged"] == 0 and info["iterations"] == 1 and info["empty_cluster"] == -1
    assert np.array_equal(cent, C0)
    assert assign.min() >= 0 and assign.max() < len(C0)
    with pytest.raises(ValueError, match="finite number > 0"):
        yfv2.genanchors.kmeans(X, C0.copy(), 0.005, str(tmp_path / "a.txt"), 352, 352, device=dev)


def test_max_iter_stops_the_loop_with_the_centroids_of_the_completed_updates(yfv2, engine, dev, cases, tmp_path):
    X, C0, g, _ = cases(3, with_model=False)
    m = am.kmeans(X, C0, max_iter=2)
    assert len(m["updates"]) == 1
    cent, assign, avg, info = run(engine, dev, X, C0, max_iter=2)
    assert info == {"iterations": 2, "converged": 0, "empty_cluster": -1, "bad_input": 0}
    assert np.array_equal(bits(cent), bits(m["updates"][0]))          # the model's centroids after one update
    assert np.array_equal(assign, m["assign"]) and bits(avg) == bits(m["avg_iou"])   # ... and what pass 2 made of them
    one = run(engine, dev, X, C0, max_iter=1)
    assert one[3]["iterations"] == 1 and one[3]["converged"] == 0 and np.array_equal(one[0], C0)
    with pytest.raises(RuntimeError, match="max_iter = 2"):
        yfv2.genanchors.kmeans(X, C0.copy(), 0.005, str(tmp_path / "a.txt"), 352, 352, device=dev, max_iter=2)
    # exactly as many passes as the loop needs: converged
    exact = run(engine, dev, X, C0, max_iter=int(g["iterations"]))
    assert exact[3]["converged"] == 1 and exact[3]["iterations"] == int(g["iterations"])


def test_argument_errors_are_reported_before_anything_is_enqueued(yfv2, engine, dev, cases):
    from yolo_fastestv2_amd import _lib
    L = _lib.lib()
    X, C0, _, _ = cases(0, with_model=False)
    x_t = torch.from_numpy(X).to(dev)
    pad = torch.full((2 * 3 + 1,), -7.0, dtype=torch.float64, device=dev)
    c_t = pad[:6].view(3, 2)
    assign = torch.full((7,), -7, dtype=torch.int32, device=dev)
    avg = torch.full((), -7.0, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    info = _lib.KmeansInfo()
    info.struct_size = C.sizeof(_lib.KmeansInfo)
    info.iterations = -7
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(wh=P(x_t), N=7, cent=P(c_t), k=3, max_iter=10, asg=P(assign), av=P(avg), inf=C.byref(info)):
        return L.yfv2_anchor_kmeans(engine._h, wh, N, cent, k, max_iter, asg, av, inf, stream)

    bad = [dict(wh=None), dict(cent=None), dict(av=None), dict(inf=None), dict(N=0), dict(N=-5), dict(k=0), dict(k=33), dict(max_iter=0),
           dict(wh=C.c_void_p(x_t.data_ptr() + 4)), dict(cent=C.c_void_p(c_t.data_ptr() + 4))]
    for kw in bad:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert "yfv2_anchor_kmeans" in _lib.last_error(engine._h), kw
    assert L.yfv2_anchor_kmeans(None, P(x_t), 7, P(c_t), 3, 10, None, P(avg), C.byref(info), stream) == _lib.ERR_ARG
    assert L.yfv2_debug_kmeans_group(engine._h, 0) == _lib.ERR_ARG and L.yfv2_debug_kmeans_group(engine._h, 65) == _lib.ERR_ARG
    torch.cuda.synchronize(dev)
    assert (pad.cpu() == -7.0).all() and (assign.cpu() == -7).all() and float(avg.cpu()) == -7.0 and info.iterations == -7
    # the same buffers with good arguments: the call works (k = 32 and k = 1 are the limits)
    c_t.copy_(torch.from_numpy(C0))
    assert call() == _lib.OK and info.converged == 1 and info.iterations == 3
    assert float(pad[6].cpu()) == -7.0
    wide = am.make_x(11, 4099)
    m = am.kmeans(wide, wide[:32], max_iter=3)
    cent, asg, av, inf32 = run(engine, dev, wide, wide[:32], max_iter=3)
    assert inf32["iterations"] == m["iterations"] and np.array_equal(asg, m["assign"]) and np.array_equal(bits(cent), bits(m["centroids"]))
    assert bits(av) == bits(m["avg_iou"]) and asg.max() == 31


def test_a_shorter_info_struct_gets_the_fields_it_has(engine, dev, cases):
    from yolo_fastestv2_amd import _lib
    X, C0, g, _ = cases(0, with_model=False)
    x_t, c_t = torch.from_numpy(X).to(dev), torch.from_numpy(C0.copy()).to(dev)
    avg = torch.zeros((), dtype=torch.float64, device=dev)
    info = _lib.KmeansInfo()
    info.struct_size, info.empty_cluster, info.bad_input = 12, 77, 77    # a caller whose header ends after `converged`
    rc = _lib.lib().yfv2_anchor_kmeans(engine._h, C.c_void_p(x_t.data_ptr()), 7, C.c_void_p(c_t.data_ptr()), 3, 100, None, C.c_void_p(avg.data_ptr()),
                                       C.byref(info), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == _lib.OK and (info.struct_size, info.iterations, info.converged) == (12, int(g["iterations"]), 1)
    assert (info.empty_cluster, info.bad_input) == (77, 77)


def test_main_end_to_end_writes_the_reference_file_and_its_anchors_decode(yfv2, dev, golden, cases, tmp_path):
    X, C0, g, _ = cases(1, with_model=False)
    traintxt = am.write_label_tree(str(tmp_path / "data"), X)
    random.seed(int(g["seed"]))
    out = tmp_path / "out"
    results = yfv2.genanchors.main(["genanchors", "--traintxt", traintxt, "--output_dir", str(out), "--num_clusters", "6"])
    assert (out / "anchors6.txt").read_bytes() == g["file"].tobytes()
    (k, centroids, avg_iou, iterations), = results
    assert k == 6 and iterations == int(g["iterations"])
    anchors = yfv2.genanchors.anchors_for_cfg(centroids, 352, 352)
    eng = yfv2.Engine(dev, 352, 352, classes=3, plan={})
    eng.set_anchors(anchors)
    preds = [torch.randn(s, device=dev, generator=torch.Generator(dev).manual_seed(1)) for s in eng.logit_shapes(1)]
    boxes = eng.decode(preds).cpu()
    assert tuple(boxes.shape) == (1, eng.rows, 8) and torch.isfinite(boxes).all()
