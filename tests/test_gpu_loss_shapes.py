"""yfv2_loss (the four launches of yfv2_loss.hip) at the shapes of tests/loss_cases.py: non-square, 1-wide / 1-high, 1x1 and
larger-than-22x22 maps, 1 .. 255 classes, batches 1 .. 9, 0 .. 200 labels, saturated logits, rows outside the precondition.

The yardstick is the fp32 oracle (= the reference's compute_loss and autograd bit for bit at every case: golden_loss_shapes.npz,
checked on the CPU by tests/test_loss_shapes_host.py), with tests/test_loss.py's rules: losses within 1e-5 * max(1, |ref|),
each gradient map within 1e-5 * max(largest |ref gradient| of the map, 1e-3).  Per case the float64 oracle is run as well and
two figures are recorded (record_parity; committed as profiles/loss_shapes_parity.json): e_ref, the fp32 oracle against
float64, and e_dev, the device against float64, both as fractions of the map's largest gradient."""
import functools
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_loss_shapes.npz")))


@functools.lru_cache(maxsize=None)
def _case(ci):
    """inputs and references of one case, computed once and never written to: (preds, targets with any bad rows, fp32
    reference losses, fp32 reference gradients, float64 gradients)"""
    c = LC.CASES[ci]
    preds, t, valid = LC.case_inputs(c)
    z = _golden()
    assert np.array_equal(t, z["targets%d" % ci])
    _, g64 = LC.oracle_loss(c, preds, t[valid], torch.float64)
    return preds, t, z["loss%d" % ci], LC.golden_grads(z, ci, preds), g64


def _engine(c, max_batch=None):
    import yolo_fastestv2_amd as yfv2
    return yfv2.Engine(torch.device("cuda:0"), c.H, c.W, c.classes, 3, anchors=LC.anchors_for(c.H, c.W), max_batch=max_batch or c.B)


def _run(eng, preds, t, want_grad=True):
    dp = [torch.from_numpy(p).to(eng.device) for p in preds]
    losses, grads = eng.loss(dp, torch.from_numpy(t), want_grad=want_grad)
    return losses.cpu().numpy(), None if grads is None else [g.cpu().numpy() for g in grads]


def _fractions(got, exact):
    """per map: max |got - exact| as a fraction of the map's largest exact gradient (floored at 1e-3, as the rule's scale is)"""
    return [float(np.abs(g.astype(np.float64) - e).max() / max(float(np.abs(e).max()), 1e-3)) for g, e in zip(got, exact)]


def _hold(losses, grads, ref_losses, ref_grads, what):
    print("%s: losses %s reference %s" % (what, losses, ref_losses))
    errs = [float(np.abs(g - r).max()) for g, r in zip(grads, ref_grads)]
    print("%s: gradient max abs err per map %s, largest reference gradient per map %s" % (what, errs, [float(np.abs(r).max()) for r in ref_grads]))
    assert np.isfinite(losses).all() and all(np.isfinite(g).all() for g in grads), what
    assert np.abs(losses - ref_losses).max() <= 1e-5 * max(1.0, float(np.abs(ref_losses).max())), (what, losses, ref_losses)
    for k, (err, r) in enumerate(zip(errs, ref_grads)):
        assert err <= 1e-5 * max(float(np.abs(r).max()), 1e-3), "%s map %d: max abs err %g (largest gradient %g)" % (what, k, err, np.abs(r).max())


@pytest.mark.parametrize("ci", range(len(LC.CASES)), ids=[LC.case_id(c) for c in LC.CASES])
def test_hip_loss_and_gradients_at_other_shapes(ci, record_parity):
    c = LC.CASES[ci]
    preds, t, ref_losses, ref_grads, g64 = _case(ci)
    eng = _engine(c)
    losses, grads = _run(eng, preds, t)                  # a bad_rows case: ALL rows go in; the references saw the valid ones
    e_ref, e_dev = _fractions(ref_grads, g64), _fractions(grads, g64)
    record_parity("loss_shapes/" + LC.case_id(c), e_ref=max(e_ref), e_dev=max(e_dev), e_ref_maps=e_ref, e_dev_maps=e_dev,
                  loss_rel_err=float(np.abs(losses - ref_losses).max() / max(1.0, float(np.abs(ref_losses).max()))))
    print("e_ref %s\ne_dev %s" % (e_ref, e_dev))
    _hold(losses, grads, ref_losses, ref_grads, LC.case_id(c))
    if c.classes == 1:
        assert losses[2] == 0.0 and not grads[2].any() and not grads[5].any()
    if c.T == 0:
        assert losses[0] == 0.0 and losses[2] == 0.0 and not any(grads[k].any() for k in (0, 2, 3, 5))
    # forward only: the same four values, no gradients
    l2, g2 = _run(eng, preds, t, want_grad=False)
    assert g2 is None and np.array_equal(l2, losses), (l2, losses)
    # the same call again: gradients are overwritten, not accumulated (atomic sums may differ by their rounding only)
    l3, g3 = _run(eng, preds, t)
    _hold(l3, g3, losses, grads, LC.case_id(c) + " second call against the first")
    _hold(l3, g3, ref_losses, ref_grads, LC.case_id(c) + " second call")


def test_one_handle_serves_a_smaller_batch_after_a_larger_one():
    """the objectness target bytes and the match counters live in a workspace whose layout moves with B: B = 5, then B = 2 with
    fewer labels on the same handle must give what a fresh handle gives"""
    big, small = (LC.CASES[i] for i in LC.REUSE)
    eng = _engine(big)
    preds, t, ref_losses, ref_grads, _ = _case(LC.REUSE[0])
    _hold(*_run(eng, preds, t), ref_losses, ref_grads, "B = 5 on the shared handle")
    preds, t, ref_losses, ref_grads, _ = _case(LC.REUSE[1])
    used = _run(eng, preds, t)
    fresh = _run(_engine(small), preds, t)
    _hold(*used, *fresh, "B = 2 on the used handle against a fresh handle")
    _hold(*used, ref_losses, ref_grads, "B = 2 on the used handle")
    l2, g2 = _run(eng, preds, t, want_grad=False)
    assert g2 is None and np.array_equal(l2, used[0])


def test_compute_loss_drop_in_on_raw_tensors_at_288x384():
    """utils/loss.py's entry point on tensors that carry no _yfv2_engine (not a Detector's output): the engine comes from
    cfg's width / height; a scaled total scales the gradients"""
    import yolo_fastestv2_amd as yfv2
    c = LC.CASES[LC.DROPIN]
    assert (c.H, c.W) == (288, 384)
    preds, t, ref_losses, ref_grads, _ = _case(LC.DROPIN)
    dev = torch.device("cuda:0")
    dp = [torch.from_numpy(p).to(dev).requires_grad_() for p in preds]
    assert not hasattr(dp[0], "_yfv2_engine")
    cfg = {"anchor_num": 3, "classes": c.classes, "width": c.W, "height": c.H, "anchors": LC.anchors_for(c.H, c.W)}
    out = yfv2.compute_loss(dp, torch.from_numpy(t).to(dev), cfg, dev)
    assert isinstance(out, tuple) and len(out) == 4
    for v in out:
        assert tuple(v.shape) == (1,) and v.device.type == "cuda" and v.dtype == torch.float32
    got = np.asarray([float(v.detach()) for v in out], np.float32)
    assert np.abs(got - ref_losses).max() <= 1e-5 * max(1.0, float(np.abs(ref_losses).max())), (got, ref_losses)
    (out[3] * 2.0).backward()
    for k, (p, r) in enumerate(zip(dp, ref_grads)):
        err = float(np.abs(p.grad.cpu().numpy() - 2.0 * r).max())
        assert err <= 2.0 * 1e-5 * max(float(np.abs(r).max()), 1e-3), "map %d: max abs err %g of twice the gradient (largest %g)" % (k, err, np.abs(r).max())
