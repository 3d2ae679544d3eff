"""Anchor k-means without a GPU: the host half of yolo_fastestv2_amd.genanchors against the reference's goldens
(tests/golden/golden_anchors.npz, made by make_golden_anchors.py from the reference's own genanchors.py), and the numpy model
of the kernels' summation order (tests/anchors_model.py) against the same goldens.  The model is what
tests/test_gpu_anchors.py compares the device with bit for bit."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import anchors_model as am
from yolo_fastestv2_amd import _lib, genanchors


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(am.GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def model_runs(golden):
    """the model's result for every case, computed once"""
    runs = []
    for i in range(len(am.CASES)):
        X, C0, g = am.load_case(golden, i)
        runs.append((g, am.kmeans(X, C0)))
    return runs


def test_golden_holds_the_cases_and_their_gap_condition(golden):
    assert [tuple(int(v) for v in row) for row in golden["cases"]] == am.CASES
    for i, (N, k, seed) in enumerate(am.CASES):
        assert k == 1 or float(golden["c%d_min_gap" % i]) >= 1e-9   # no assignment can hinge on the summation order


@pytest.mark.parametrize("i", range(len(am.CASES)))
def test_write_anchors_to_file_reproduces_the_reference_file(golden, tmp_path, i):
    X, _, g = am.load_case(golden, i)
    path = tmp_path / "anchors.txt"
    genanchors.write_anchors_to_file(g["centroids"], X, str(path), int(golden["width"]), int(golden["height"]), avg_iou=float(g["avg_iou"]))
    assert path.read_bytes() == g["file"].tobytes()


def test_write_anchors_to_file_without_a_kmeans_result_recomputes_the_average(golden, tmp_path):
    X, _, g = am.load_case(golden, 1)
    path = tmp_path / "anchors.txt"
    genanchors.write_anchors_to_file(g["centroids"], X, str(path), int(golden["width"]), int(golden["height"]))
    assert path.read_bytes() == g["file"].tobytes()


def test_read_label_dims_walks_jpg_and_png_entries(tmp_path):
    X = am.make_x(2, 255)
    traintxt = am.write_label_tree(str(tmp_path / "data"), X)
    got = genanchors.read_label_dims(traintxt)
    assert got.dtype == np.float64 and got.shape == (255, 2)
    assert np.array_equal(got, X)


def test_anchors_for_cfg_is_sorted_by_width_and_rounded_like_the_file(golden):
    _, _, g = am.load_case(golden, 1)
    flat = genanchors.anchors_for_cfg(g["centroids"], 352, 352)
    assert len(flat) == 12 and all(isinstance(v, float) for v in flat)
    assert flat[0::2] == sorted(flat[0::2])
    first_line = g["file"].tobytes().decode().split("\n")[0]
    assert flat == [float(v) for v in first_line.replace(" ", "").split(",")]
    # a different width / height scales each column on its own
    wide = genanchors.anchors_for_cfg(np.array([[0.5, 0.25], [0.125, 0.75]]), 320, 480)
    assert wide == [40.0, 360.0, 160.0, 120.0]


def test_main_draws_the_initial_centroids_as_the_reference_does(golden, tmp_path, monkeypatch):
    X, C0, g = am.load_case(golden, 1)
    traintxt = am.write_label_tree(str(tmp_path / "data"), X)
    seen = {}

    def fake_kmeans(dims, centroids, eps, anchor_file, width, height, **kw):
        seen.update(dims=dims.copy(), centroids=centroids.copy(), anchor_file=anchor_file, size=(width, height))
        return centroids, np.zeros(len(dims), np.int32), 0.5, 1

    monkeypatch.setattr(genanchors, "kmeans", fake_kmeans)
    random.seed(int(g["seed"]))
    genanchors.main(["genanchors", "--traintxt", traintxt, "--output_dir", str(tmp_path / "out"), "--num_clusters", "6"])
    assert np.array_equal(seen["dims"], X)
    assert np.array_equal(seen["centroids"], X[[int(v) for v in g["init_idx"]]])
    assert seen["anchor_file"] == os.path.join(str(tmp_path / "out"), "anchors6.txt") and seen["size"] == (352, 352)


def test_main_warns_when_the_cluster_count_is_not_the_models(tmp_path, monkeypatch):
    traintxt = am.write_label_tree(str(tmp_path / "data"), am.make_x(1, 7))
    monkeypatch.setattr(genanchors, "kmeans", lambda dims, c, *a, **kw: (c, None, 0.5, 1))
    with pytest.warns(UserWarning, match="6 anchor pairs"):
        genanchors.main(["genanchors", "--traintxt", traintxt, "--output_dir", str(tmp_path / "out"), "--num_clusters", "3"])


def test_tree_sum_is_the_documented_tree():
    rng = np.random.RandomState(0)
    v = rng.rand(1000)
    padded = np.concatenate([v, np.zeros(24)]).reshape(4, 256)
    lane = ((padded[0] + padded[1]) + padded[2]) + padded[3]
    waves = []
    for w in range(4):
        a = list(lane[64 * w:64 * w + 64])
        for half in (32, 16, 8, 4, 2, 1):
            a = [a[l] + a[l + half] for l in range(half)]
        waves.append(a[0])
    assert am.tree_sum(v) == ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert abs(am.tree_sum(v) - np.sum(v)) < 1e-12 * np.sum(v)


def test_model_similarity_is_the_references_four_cases():
    # one box per case and the boundary where two cases meet (the first test that holds decides)
    X = np.array([[0.2, 0.3]])
    for c, expect in (((0.4, 0.5), 0.2 * 0.3 / (0.4 * 0.5)), ((0.4, 0.1), 0.2 * 0.1 / (0.2 * 0.3 + (0.4 - 0.2) * 0.1)),
                      ((0.1, 0.5), 0.1 * 0.3 / (0.2 * 0.3 + 0.1 * (0.5 - 0.3))), ((0.1, 0.1), (0.1 * 0.1) / (0.2 * 0.3)),
                      ((0.2, 0.3), 0.2 * 0.3 / (0.2 * 0.3))):
        assert am.similarity(X, np.array([c]))[0, 0] == expect


@pytest.mark.parametrize("i", range(len(am.CASES)))
def test_model_of_the_kernels_matches_the_reference(model_runs, i):
    g, m = model_runs[i]
    assert m["converged"] == 1 and m["empty_cluster"] == -1
    assert m["iterations"] == int(g["iterations"])
    assert np.array_equal(m["assign"], g["assign"].astype(np.int64))   # every point: the gap condition leaves no exemption
    assert np.all(np.abs(m["centroids"] - g["centroids"]) <= 1e-12 * np.abs(g["centroids"]))
    assert abs(m["avg_iou"] - float(g["avg_iou"])) <= 1e-12 * float(g["avg_iou"])


def test_model_stops_at_max_iter_without_moving_the_centroids_again(golden):
    X, C0, _ = am.load_case(golden, 3)
    two = am.kmeans(X, C0, max_iter=2)
    full = am.kmeans(X, C0, max_iter=3)
    assert two["converged"] == 0 and two["iterations"] == 2 and len(two["updates"]) == 1
    assert np.array_equal(two["centroids"], full["updates"][0])


def test_model_reports_the_first_empty_cluster(golden):
    X, C0, _ = am.load_case(golden, 1)
    C0[1] = C0[0]
    m = am.kmeans(X, C0)
    assert m["empty_cluster"] == 1 and m["converged"] == 0 and np.array_equal(m["centroids"], C0)


def test_kmeans_info_struct_is_five_int32_with_its_size_first():
    assert C.sizeof(_lib.KmeansInfo) == 20
    assert [f[0] for f in _lib.KmeansInfo._fields_] == ["struct_size", "iterations", "converged", "empty_cluster", "bad_input"]
    assert _lib.KmeansInfo.struct_size.offset == 0
    header = open(os.path.join(os.path.dirname(am.__file__), "..", "include", "yfv2.h")).read()
    body = header.split("typedef struct yfv2_kmeans_info {")[1].split("} yfv2_kmeans_info;")[0]
    assert body.count("int32_t ") == 5
