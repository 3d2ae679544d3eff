"""Every training kernel of yfv2_train.hip one layer deep on the device, at the shapes of tests/train_cases.py: Detector in train()
mode, compute_loss and backward run on the MI355X; the arenas are read back (Engine.debug_train_tensor) into a run record, and
tests/train_layers.py evaluates every op in float64 from the device's OWN operands and compares with the device's result of that
op.  Every ratio error / bound must be <= 1, with the bound's k read from the kernel (train_layers.K - no allowance for ATen's
arithmetic here) and p.grad, what the caller sees, as the parameter gradients.  The ratios per kernel kind and case are recorded
(record_parity; committed as the "gpu" key of profiles/train_layers_parity.json).

Two sequence tests, device against device, run one module across input sizes and across batch sizes (the `_train_bound` re-keying,
Train::record at a smaller batch on a kept handle) and compare .grad after each step with a fresh module's at the same weights."""
import numpy as np
import pytest
import torch

import loss_cases as LC
import train_cases as TC
import train_layers as TL

pytestmark = pytest.mark.gpu

RUN = [i for i, c in enumerate(TC.CASES) if not c.raises]
IDS = [TC.case_id(TC.CASES[i]) for i in RUN]


def _cfg(c):
    return {"anchor_num": 3, "classes": c.classes, "width": c.W, "height": c.H, "anchors": TC.anchors_for(c.H, c.W)}


def _model(c, w, dev):
    import yolo_fastestv2_amd as yfv2
    model = yfv2.Detector(c.classes, 3, True).to(dev)
    model.load_state_dict({k: v.clone() for k, v in w.items()})
    model.train()
    return model


def _iteration(model, c, x, t, dev):
    """forward, loss, backward on the device -> (logits, their gradients, losses)"""
    import yolo_fastestv2_amd as yfv2
    preds = model(torch.from_numpy(x).to(dev))
    for p in preds:
        p.retain_grad()
    losses = yfv2.compute_loss(preds, torch.from_numpy(t).to(dev), _cfg(c), dev)
    losses[3].backward()
    return preds, [p.grad if p.grad is not None else torch.zeros_like(p) for p in preds], losses


@pytest.mark.parametrize("ci", RUN, ids=IDS)
def test_every_training_kernel_one_layer_deep(ci, record_parity):
    c = TC.CASES[ci]
    dev = torch.device("cuda:0")
    w, x, t = TC.case_inputs(c)
    model = _model(c, w, dev)
    run_before = {k: v.clone() for k, v in w.items() if k.endswith(("running_mean", "running_var"))}
    preds, dlogits, losses = _iteration(model, c, x, t, dev)
    eng = preds[0]._yfv2_engine
    rec = TL.device_record(model, eng, torch.from_numpy(x), preds, dlogits, run_before, c.H, c.W, c.classes)
    rep = TL.check(rec, c.H, c.W, c.classes)
    print(rep.as_json())
    record_parity("train_layers/gpu/" + TC.case_id(c), **{k: round(v, 4) for k, v in rep.ratios().items()})
    # the loss against the float64 evaluation of the same expressions on the device's own logits (tests/test_loss.py's rule)
    got = np.asarray([float(v.detach()) for v in losses], np.float64)
    ref, _ = LC.oracle_loss(c, [p.detach().cpu().numpy() for p in preds], t, torch.float64)
    print("losses", got, "float64 on the device's logits", ref)
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max())), (got, ref)
    assert len(rep.worst) >= 26, sorted(rep.worst)
    bad = {k: v for k, v in rep.worst.items() if not v[0] <= 1.0}
    assert not bad, bad


def _close(model, fresh, scale=1.0, what=""):
    """test_train_gpu.py's gradient-accumulation rule: rtol 1e-5, atol 1e-7 of the tensor's largest gradient"""
    ref = dict(fresh.named_parameters())
    for k, p in model.named_parameters():
        g = scale * ref[k].grad
        assert p.grad is not None and torch.isfinite(p.grad).all(), (what, k)
        assert torch.allclose(p.grad, g, rtol=1e-5, atol=1e-7 * float(g.abs().max() + 1e-12)), (what, k, float((p.grad - g).abs().max()), float(g.abs().max()))


def _sequence(steps):
    """steps: (H, W, B) per step.  One module and one optimizer walk them; after each backward .grad must be what a fresh module
    computes at the same weights and input, a second backward without zero_grad() must double it, and zero_grad() must start over"""
    import yolo_fastestv2_amd as yfv2
    dev = torch.device("cuda:0")
    inputs = [TC.sequence_inputs(H, W, B, i) for i, (H, W, B) in enumerate(steps)]     # one label per image: see train_cases.py
    w0 = TC.case_inputs(inputs[0][0])[0]
    model = _model(inputs[0][0], w0, dev)
    opt = yfv2.SGD(params=model.parameters(), lr=TC.LR, momentum=0.949, weight_decay=0.0005)
    engines = set()
    for i, (c, x, t) in enumerate(inputs):
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        fresh = _model(c, state, dev)
        _iteration(fresh, c, x, t, dev)
        opt.zero_grad()
        preds, _, losses = _iteration(model, c, x, t, dev)
        engines.add(id(preds[0]._yfv2_engine))
        assert tuple(preds[0].shape) == (c.B, 12, c.H // 16, c.W // 16) and bool(torch.isfinite(losses[3]))
        _close(model, fresh, 1.0, "step %d %s" % (i, TC.case_id(c)))
        _iteration(model, c, x, t, dev)                          # no zero_grad(): the gradients of the same weights add up
        _close(model, fresh, 2.0, "step %d %s accumulated" % (i, TC.case_id(c)))
        opt.zero_grad()
        _iteration(model, c, x, t, dev)
        _close(model, fresh, 1.0, "step %d %s after zero_grad" % (i, TC.case_id(c)))
        before = model.output_reg_layers.weight.detach().clone()
        opt.step()
        assert not torch.equal(before, model.output_reg_layers.weight.detach())
    return engines


def test_one_module_and_optimizer_across_input_sizes():
    engines = _sequence(TC.SEQUENCE_SIZES)
    assert len(engines) == 2                                     # one engine per input size, the first one used again by the third step


def test_one_module_across_batch_sizes():
    """Batches 3, 1, 3 at 64 x 96 on one module.

    With five labels in the one image of the batch-1 step this test failed in one of two runs, at 1.00 of the rule: .grad of
    backbone.first_conv.1.bias off by 4.7e-4 on an entry of 38.8 (largest 813.3) after two backward passes.  The cause was the loss,
    not the training kernels: yfv2_loss returned other last bits in the logit gradients in 2 of 40 iterations of that step (float
    atomicAdd over the labels that share a cell), and all 225 parameter gradients followed it exactly, 38 to 2; at batch 3, and with
    the loss repeating, every gradient repeats bit for bit, on a used handle as on a fresh one.  The steps now carry one label per
    image (train_cases.sequence_inputs); the rule is unchanged."""
    engines = _sequence([(64, 96, B) for B in TC.SEQUENCE_BATCHES])
    assert len(engines) == 1


def test_one_value_per_channel_is_refused_before_any_launch():
    """nn.BatchNorm2d in train mode raises ValueError on one value per channel (batch 1 at 32 x 32: the 1 x 1 map); the library
    normalised with variance 0 and returned beta.  Detector.forward raises the same error; yfv2_train_forward returns YFV2_ERR_ARG"""
    from yolo_fastestv2_amd import _lib
    (c,) = [c for c in TC.CASES if c.raises]
    dev = torch.device("cuda:0")
    w, x, t = TC.case_inputs(c)
    model = _model(c, w, dev)
    stats = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        model(torch.from_numpy(x).to(dev))
    for k, v in model.state_dict().items():
        assert torch.equal(v, stats[k]), k                        # nothing ran: no statistic moved, no counter stepped
    # the C entry point, on a handle that is bound (batch 2 runs) and then meets batch 1
    x2 = torch.from_numpy(np.concatenate((x, x))).to(dev)
    preds = model(x2)
    eng = preds[0]._yfv2_engine
    with pytest.raises(_lib.Yfv2Error) as e:
        eng.train_forward(x2[:1].contiguous())
    assert e.value.code == _lib.ERR_ARG and "more than 1 value per channel" in str(e.value) and "yfv2_train_forward" in str(e.value)
    preds = model(x2)                                            # the handle still serves the batch it can
    assert all(bool(torch.isfinite(p).all()) for p in preds)
