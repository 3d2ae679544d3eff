"""The loss-case table of tests/loss_cases.py on the CPU: golden_loss_shapes.npz holds what the REFERENCE's compute_loss and
autograd produced at every case (tests/golden/make_golden.py loss_shapes).  Here: (a) the oracle - what the GPU test compares
the kernels with - reproduces it exactly, with its width / height parameters at work; (b) the table exercises what it claims
to (every anchor, every offset candidate, a crowded cell); (c) every reference figure is finite; (d) an H / W mix-up would show."""
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
from conftest import GOLDEN

# cases with labels that may still leave a scale without a match (nb == 0): case index -> scales (0: stride 16, 1: stride 32).
# None today: the seeds of the T = 1 and T = 3 cases were chosen so that their labels match on both scales.
NO_MATCH_ALLOWED = {}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_loss_shapes.npz")))


@pytest.fixture(scope="module")
def inputs():
    return [LC.case_inputs(c) for c in LC.CASES]


@pytest.fixture(scope="module")
def census(inputs):
    return [LC.match_census(c, t[valid]) for c, (_, t, valid) in zip(LC.CASES, inputs)]


def test_table_covers_what_the_issue_lists():
    cs = LC.CASES
    assert {(c.H, c.W) for c in cs} >= {(32, 32), (32, 64), (64, 32), (64, 96), (352, 32), (288, 384), (640, 384)}
    assert {c.classes for c in cs} >= {1, 2, 3, 80, 255}
    assert {c.B for c in cs} >= {1, 2, 3, 5, 9}
    assert all(c.B == 4 for c in cs if (c.H, c.W) == (640, 384))
    assert {c.T for c in cs} >= {0, 1, 3} and any(c.T and 15 * c.T % 128 for c in cs)
    assert cs[LC.CROWDED][2:5] == (200, 32, 64)
    assert {c.flavour for c in cs} == {"plain", "saturated", "bad_rows"}
    assert sum(c.seed == LC.EDGE_SEED for c in cs) == 1 and len({c.seed for c in cs}) == len(cs)
    a, b = (cs[i] for i in LC.REUSE)
    assert (a.H, a.W, a.classes) == (b.H, b.W, b.classes) and a.B == 5 and b.B == 2 and b.T < a.T
    assert (cs[LC.DROPIN].H, cs[LC.DROPIN].W) == (288, 384)


def test_oracle_reproduces_the_reference_golden_at_every_shape(golden, inputs):
    assert [tuple(r) for r in golden["cases"]] == [tuple(c[:6]) for c in LC.CASES]
    assert list(golden["flavours"]) == [c.flavour for c in LC.CASES]
    for ci, (c, (preds, t, valid)) in enumerate(zip(LC.CASES, inputs)):
        assert np.array_equal(t, golden["targets%d" % ci]), ci
        losses, grads = LC.oracle_loss(c, preds, t[valid])
        assert np.array_equal(losses.astype(np.float32), golden["loss%d" % ci]), (ci, losses, golden["loss%d" % ci])
        for k, (g, r) in enumerate(zip(grads, LC.golden_grads(golden, ci, preds))):
            assert np.array_equal(g, r), (ci, k)


def test_labels_reach_every_anchor_candidate_and_a_crowded_cell(inputs, census):
    anchors = np.zeros(6, np.int64)
    cands = np.zeros((2, 5), np.int64)
    for ci, (c, cen) in enumerate(zip(LC.CASES, census)):
        for li, (d, (h, w)) in enumerate(zip(cen, LC.map_shapes(c))):
            assert sum(d["candidates"]) == d["nb"] == sum(d["anchors"]), (ci, li, d)      # the counting restatement agrees with build_target
            if c.T and li not in NO_MATCH_ALLOWED.get(ci, ()):
                assert d["nb"] >= 1, "case %d (%s): no match on scale %d" % (ci, LC.case_id(c), li)
            anchors[3 * li:3 * li + 3] += d["anchors"]
            if h * w > 1:
                cands[li] += d["candidates"]
            else:
                assert d["candidates"][1:] == [0, 0, 0, 0], (ci, li, d)                  # a 1x1 map has no neighbour
    assert (anchors > 0).all(), anchors
    assert (cands > 0).all(), cands
    assert max(d["crowd"] for d in census[LC.CROWDED]) >= 20, census[LC.CROWDED]
    # the edge case does carry centres on and past both edges
    t = inputs[[c.seed for c in LC.CASES].index(LC.EDGE_SEED)][1]
    assert (t[:, 2] == 1.0).any() and (t[:, 3] == 1.0).any() and (t[:, 2] > 1.0).any() and (t[:, 3] > 1.0).any()


def test_bad_rows_are_out_of_range_and_would_match_otherwise(inputs):
    for c, (_, t, valid) in zip(LC.CASES, inputs):
        if c.flavour != "bad_rows":
            assert valid.all() and len(t) == c.T
            continue
        bad = t[~valid]
        assert len(bad) == 4 and valid.sum() == c.T
        assert sorted(bad[:2, 0]) == [-1, c.B] and sorted(bad[2:, 1]) == [-1, c.classes]
        ok = t[valid]
        assert ((ok[:, 0] >= 0) & (ok[:, 0] < c.B) & (ok[:, 1] >= 0) & (ok[:, 1] < c.classes)).all()
        # each bad row, given a valid image and class, adds matches: skipping it is not a no-op
        base = sum(d["nb"] for d in LC.match_census(c, ok))
        for r in bad:
            fixed = r.copy()
            fixed[0], fixed[1] = 0, 0
            assert sum(d["nb"] for d in LC.match_census(c, np.vstack((ok, fixed[None])))) > base


def test_reference_figures_are_finite_in_every_flavour(golden):
    for ci, c in enumerate(LC.CASES):
        assert np.isfinite(golden["loss%d" % ci]).all(), ci
        for k in range(6):
            key = "grad%d_%d" % (ci, k)
            assert np.isfinite(golden[key] if k % 3 == 1 else golden[key + "_val"]).all(), (ci, k)
        if c.classes == 1:
            assert golden["loss%d" % ci][2] == 0 and not len(golden["grad%d_2_idx" % ci]) and not len(golden["grad%d_5_idx" % ci])


def test_saturated_cases_carry_the_stated_magnitudes(inputs):
    for c, (preds, _, _) in zip(LC.CASES, inputs):
        for k, p in enumerate(preds):
            top = float(np.abs(p).max())
            if c.flavour == "saturated":
                mag = LC.REG_SATURATION if k % 3 == 0 else LC.OBJ_CLS_SATURATION
                assert top == mag and 0.1 < float((np.abs(p) == mag).mean()) < 0.3, (c, k, top)
            else:
                assert top < LC.REG_SATURATION


def test_swapping_label_axes_moves_the_loss_on_non_square_inputs(golden, inputs):
    seen = 0
    for ci, (c, (preds, t, valid)) in enumerate(zip(LC.CASES, inputs)):
        if c.H == c.W or not c.T:
            continue
        seen += 1
        ref = float(golden["loss%d" % ci][3])
        with torch.no_grad():
            swapped = float(LC.oracle.compute_loss([torch.from_numpy(p) for p in preds], torch.from_numpy(LC.swapped_axes(t[valid])),
                                                   LC.anchors_for(c.H, c.W), c.classes, 3, c.W, c.H)[3])
        assert abs(swapped - ref) > 1e-3 * abs(ref), (ci, LC.case_id(c), ref, swapped)
    assert seen >= 8
