"""The one-layer-deep checker of tests/train_layers.py on the CPU, at every case of tests/train_cases.py.

(a) It ACCEPTS the fp32 oracle's record - ATen's arithmetic, with oneDNN on and with oneDNN off (another summation order; NNPACK is
    switched off with it: from batch 16 on it computes convolutions by Winograd / FFT transforms, which is another algorithm, with
    errors of 3e-5 where the exact result is 0, not another order of the same sums): every ratio error / bound <= 1.  The ratios are
    recorded (record_parity; committed as the "cpu" key of profiles/train_layers_parity.json).
(b) It REJECTS mutated records: each mutant below is one defect a kernel could have, applied to the record, and must push the ratio
    of the kind it aims at from <= 1 to > 1.
(c) The case table reaches every launch path it claims to (train_cases.coverage).
(d) The oracle, with its width / height parameters at work, still reproduces what the reference's own modules produced at every case
    (golden_train_shapes.npz, make_golden.py train_shapes), and refuses the one-value-per-channel case with the reference's message."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_cases as TC
import train_layers as TL
from conftest import GOLDEN
from oracle import yfv2_oracle as oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden  # noqa: E402  (TRAIN_KEEP, TRAIN_BN, train_shapes_keep)

RUN = [i for i, c in enumerate(TC.CASES) if not c.raises]
IDS = [TC.case_id(TC.CASES[i]) for i in RUN]


@functools.lru_cache(maxsize=None)
def _step(ci, onednn):
    """the fp32 oracle's training step of case ci with its run record: computed once per backend, never written to"""
    c = TC.CASES[ci]
    w, x, t = TC.case_inputs(c)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # as make_golden.py train_shapes ran it: the summation order of ATen's reductions follows the thread count
    try:
        with torch.backends.mkldnn.flags(enabled=onednn), torch.backends.nnpack.flags(enabled=onednn):
            return oracle.train_step(w, torch.from_numpy(x), torch.from_numpy(t), TC.anchors_for(c.H, c.W), c.classes, TC.LR, width=c.W, height=c.H, trace=True)
    finally:
        torch.set_num_threads(threads)


def _record(ci, onednn=True):
    return _step(ci, onednn)["record"]


@pytest.mark.parametrize("onednn", (True, False), ids=("onednn", "plain"))
@pytest.mark.parametrize("ci", RUN, ids=IDS)
def test_checker_accepts_the_fp32_oracle(ci, onednn, record_parity):
    c = TC.CASES[ci]
    rec = _record(ci, onednn)
    assert sorted(k[2:] for k in rec if k.startswith("y:")) == sorted(TL.conv_names()) and len(TL.conv_names()) == 73
    assert sorted(k[2:] for k in rec if k.startswith("v:")) == sorted(TL.named_tensors())
    rep = TL.check(rec, c.H, c.W, c.classes, aten=True)
    record_parity("train_layers/cpu/%s/%s" % (TC.case_id(c), "onednn" if onednn else "plain"), **{k: round(v, 4) for k, v in rep.ratios().items()})
    print(rep.as_json())
    assert set(rep.worst) >= {"stem_fwd", "dw_fwd", "pw_fwd", "head_fwd", "bn_mean", "bn_invstd", "bn_apply", "bn_running_mean", "bn_running_var", "maxpool_fwd",
                              "copy", "bn_bwd_dy", "bn_dgamma", "bn_dbeta", "stem_wgrad", "dw_wgrad", "pw_wgrad", "head_wgrad", "head_bias_grad", "dgrad:maxpool",
                              "dgrad:dw", "dgrad:pw", "dgrad:dw+pw", "dgrad:pass+pw", "dgrad:dw+pw+upcat", "dgrad:pw+upcat"}, sorted(rep.worst)
    bad = {k: v for k, v in rep.worst.items() if not v[0] <= 1.0}
    assert not bad, bad


# ---- mutants: (record, case) -> (mutated record, the ops / tensors to check, the kind whose ratio must rise above 1)
def _copy(rec):
    out = dict(rec)
    for k in ("pgrad", "run_after"):
        out[k] = dict(rec[k])
    return out


def _op(c, name):
    return next(o for o in TL.topology(c.H, c.W, c.classes) if o.name == name and o.kind in ("conv", "head"))


def mutant_weight_gradient_drops_a_pixel(rec, c):
    name = "fpn.cls_head_3.block.3"
    op, out = _op(c, name), _copy(rec)
    x, dy = TL._view(rec, op.src), rec["dy:" + name].double().clone()
    b, co, ci, yy, xx = np.unravel_index(int((dy[:, :, None].abs() * x[:, None].abs()).argmax()), (dy.shape[0], dy.shape[1], x.shape[1], dy.shape[2], dy.shape[3]))
    dy[b, co, yy, xx] = 0.0                                   # output channel co never sees pixel (b, yy, xx)
    out["pgrad"][name + ".weight"] = TL._conv_weight_grad(x, rec["param"][name + ".weight"].shape, dy, op).float()
    return out, {name}, "pw_wgrad"


def mutant_data_gradient_loses_its_last_column(rec, c):
    key = "z:backbone.stage2.1.branch_main.0"                 # consumed by a 3 x 3 depthwise conv on the H / 8 x W / 8 map
    out = _copy(rec)
    g = rec[TL._gkey(key)].clone()
    assert g[..., -1].abs().max() > 0
    g[..., -1] = 0.0
    out[TL._gkey(key)] = g
    return out, {key}, "dgrad:dw"


def mutant_dy_ignores_a_relu_mask_bit(rec, c):
    name = "backbone.stage3.1.branch_main.0"
    op, out = _op(c, name), _copy(rec)
    y, z, dz = (rec[p + name].double() for p in ("y:", "z:", "dz:"))
    blocked = (z <= 0) * dz.abs()
    assert blocked.max() > 0
    z = z.clone()
    z.view(-1)[int(blocked.argmax())] = 1.0                   # this element's gradient passes although its ReLU output was 0
    dy = TL.bn_backward64(y, z, dz, rec["mean:" + name].double(), rec["invstd:" + name].double(), rec["param"][op.bn + ".weight"].double(), True)[0]
    out["dy:" + name] = dy.float()
    return out, {name}, "bn_bwd_dy"


def mutant_running_variance_moved_with_the_biased_variance(rec, c):
    name = "fpn.reg_head_3.block.3"
    op, out = _op(c, name), _copy(rec)
    y = rec["y:" + name].double()
    var = y.var((0, 2, 3), unbiased=False)
    out["run_after"][op.bn + ".running_var"] = (0.9 * rec["run_before"][op.bn + ".running_var"].double() + 0.1 * var).float()
    return out, {name}, "bn_running_var"


def mutant_head_weight_gradient_from_one_scale(rec, c):
    name, out = "output_reg_layers", _copy(rec)
    op = next(o for o in TL.topology(c.H, c.W, c.classes) if o.kind == "head" and o.name == name and o.slot == 0)
    out["pgrad"][name + ".weight"] = TL._conv_weight_grad(TL._view(rec, op.src), rec["param"][name + ".weight"].shape, rec["dlogits"][0].double(), op).float()
    return out, {name}, "head_wgrad"


def mutant_maxpool_gradient_goes_to_the_last_maximum(rec, c):
    out = _copy(rec)
    z, gout = rec["z:backbone.first_conv.0"], rec["g:backbone.maxpool"]
    B, C, H, W = z.shape
    cols = F.unfold(F.pad(z, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(B, C, 9, -1)
    hit = cols == cols.max(2, keepdim=True)[0]
    tied = (hit.sum(2) > 1) * gout.reshape(B, C, -1).abs()    # windows whose maximum occurs twice (a run of ReLU zeros), by the size of their gradient
    assert tied.max() > 0, "no max-pool window with a tied maximum and a gradient"
    b, ch, l = np.unravel_index(int(tied.argmax()), tuple(tied.shape))
    taps = torch.nonzero(hit[b, ch, :, l]).flatten()
    oy, ox = divmod(int(l), W // 2)
    pos = lambda k: (2 * oy - 1 + int(k) // 3, 2 * ox - 1 + int(k) % 3)  # noqa: E731
    g = rec["dz:backbone.first_conv.0"].clone()
    v = gout.reshape(B, C, -1)[b, ch, l]
    g[(b, ch) + pos(taps[0])] -= v
    g[(b, ch) + pos(taps[-1])] += v
    out["dz:backbone.first_conv.0"] = g
    return out, {"z:backbone.first_conv.0"}, "dgrad:maxpool"


MUTANTS = (mutant_weight_gradient_drops_a_pixel, mutant_data_gradient_loses_its_last_column, mutant_dy_ignores_a_relu_mask_bit,
           mutant_running_variance_moved_with_the_biased_variance, mutant_head_weight_gradient_from_one_scale, mutant_maxpool_gradient_goes_to_the_last_maximum)


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m.__name__[7:] for m in MUTANTS])
@pytest.mark.parametrize("ci", RUN, ids=IDS)
def test_checker_rejects_a_mutated_record(ci, mutant):
    c = TC.CASES[ci]
    rec = _record(ci)
    bad, only, kind = mutant(rec, c)
    before = TL.check(rec, c.H, c.W, c.classes, only=only, aten=True).ratios()
    after = TL.check(bad, c.H, c.W, c.classes, only=only, aten=True).ratios()
    print(kind, before[kind], "->", after[kind])
    assert before[kind] <= 1.0 < after[kind], (kind, before[kind], after[kind])
    # ... and under the device's own table (no ATen allowance), which is what the GPU test applies
    assert TL.check(bad, c.H, c.W, c.classes, only=only).ratios()[kind] > 1.0


def test_the_table_reaches_every_path_it_names():
    cov = TC.coverage()
    missing = [k for k in TC.REQUIRED if not cov.get(k)]
    assert not missing, missing
    ids = {TC.case_id(c): c for c in TC.CASES}
    assert cov["pw_wgrad_upw2_ragged_wave"] == ["64x64_b87_c2"] and cov["stem_wgrad_ragged_third_chunk"] == ["160x128_b2_c80"]
    assert "128x128_b1_c80" in cov["reduce_segments_2"] and "160x128_b2_c80" in cov["reduce_segment_crosses_image"]
    assert {(c.H, c.W, c.B, c.classes) for c in TC.CASES} == {(32, 32, 2, 3), (32, 64, 5, 255), (96, 32, 4, 1), (64, 96, 3, 20), (128, 128, 1, 80),
                                                            (160, 128, 2, 80), (64, 64, 87, 2), (32, 32, 1, 3)}
    assert [c.raises for c in TC.CASES] == [False] * 7 + [True] and len(ids) == len(TC.CASES)
    # the formulas against the figures the table's comments give
    assert TC.reduce_segments(1 * 64 * 64, 24) == 2 and TC.reduce_segments(2 * 80 * 64, 24) == 5
    assert TC.wgrad_chunks(2, 80 * 64) == 3 and TC.pw_wgrad_launch(16, 87, 288, 72) == (64, 1, 87, 2, 12)
    assert TC.pw_gemm_grid(2, 5, 255) == (4, 1, 4) and TC.pw_gemm_grid(64, 2, 24)[0] == 2
    fpn = next(o for o in TL.topology(64, 64, 2) if o.name == "fpn.conv1x1_2.0")
    assert (fpn.cin, fpn.cout, fpn.oh * fpn.ow) == (288, 72, 16)


def test_sequence_steps_carry_one_label_per_image_that_matches_on_both_scales():
    """the sequence tests of the GPU file compare two runs: no cell may sum DIFFERENT labels (yfv2_loss's atomic order), see train_cases.py"""
    for steps in (TC.SEQUENCE_SIZES, [(64, 96, B) for B in TC.SEQUENCE_BATCHES]):
        for i, (H, W, B) in enumerate(steps):
            c, x, t = TC.sequence_inputs(H, W, B, i)
            assert x.shape == (B, 3, H, W) and list(t[:, 0]) == list(range(B))
            tg = oracle.build_target([(H // 16, W // 16), (H // 32, W // 32)], t, TC.anchors_for(H, W), 3, W, H)
            assert all(len(g[0]) > 0 for g in tg), (H, W, B, [len(g[0]) for g in tg])
    assert any(B == 1 for B in TC.SEQUENCE_BATCHES) and len({s[:2] for s in TC.SEQUENCE_SIZES}) == 2


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_train_shapes.npz")))


def test_golden_lists_the_table(golden):
    assert [tuple(r) for r in golden["cases"]] == [tuple(c[:6]) for c in TC.CASES]
    assert list(golden["raises"]) == [c.raises for c in TC.CASES] and float(golden["lr"]) == TC.LR
    assert tuple(golden["subsample"]) == make_golden.TRAIN_SHAPES_SUBSAMPLE
    assert os.path.getsize(os.path.join(GOLDEN, "golden_train_shapes.npz")) < 512 * 1024


@pytest.mark.parametrize("ci", RUN, ids=IDS)
def test_oracle_reproduces_the_reference_golden_at_every_shape(ci, golden):
    """make_train_golden's rules: losses to 1e-6, gradients to 1e-5 of the tensor's largest entry, updated values to 1e-6"""
    g, mine = golden, _step(ci, True)
    assert np.array_equal(TC.case_inputs(TC.CASES[ci])[2], g["targets%d" % ci])
    for a, b in zip(g["loss%d" % ci], mine["losses"]):
        assert abs(float(a) - b) <= 1e-6 * max(1.0, abs(float(a))), (float(a), b)
    names = [str(n) for n in g["names"]]
    assert names == sorted(mine["grads"]) and len(names) == 225
    for k, gn, gm in zip(names, g["gnorm%d" % ci], g["gmax%d" % ci]):
        t = mine["grads"][k]
        assert abs(float(t.double().norm()) - gn) <= 1e-5 * max(gn, 1e-9), (k, float(t.double().norm()), gn)
        assert abs(float(t.abs().max()) - gm) <= 1e-5 * max(gm, 1e-9), (k, float(t.abs().max()), gm)
    for k in make_golden.TRAIN_KEEP:
        ref = g["grad%d:%s" % (ci, k)]
        sc = float(g["gmax%d" % ci][names.index(k)])
        assert np.abs(make_golden.train_shapes_keep(mine["grads"][k].numpy()) - ref).max() <= 1e-5 * max(sc, 1e-6), k
        ref = g["after%d:%s" % (ci, k)]
        assert np.abs(make_golden.train_shapes_keep(mine["new_w"][k].numpy()) - ref).max() <= 1e-6 * max(1.0, float(np.abs(ref).max())), k
    for bn in make_golden.TRAIN_BN:
        for sfx in (".running_mean", ".running_var"):
            ref = g["after%d:%s" % (ci, bn + sfx)]
            assert np.abs(mine["new_w"][bn + sfx].numpy() - ref).max() <= 1e-6 * max(1.0, float(np.abs(ref).max())), bn + sfx


def test_one_value_per_channel_raises_as_the_reference_does(golden):
    (ci,) = [i for i, c in enumerate(TC.CASES) if c.raises]
    c = TC.CASES[ci]
    assert c.B * (c.H // 32) * (c.W // 32) == 1
    msg = str(golden["error%d" % ci])
    assert msg.startswith("Expected more than 1 value per channel when training")
    w, x, t = TC.case_inputs(c)
    with pytest.raises(ValueError) as e:
        oracle.train_step(w, torch.from_numpy(x), torch.from_numpy(t), TC.anchors_for(c.H, c.W), c.classes, TC.LR, width=c.W, height=c.H)
    assert str(e.value) == msg


def test_debug_train_tensor_is_declared_where_the_wrapper_expects_it():
    import ctypes as C
    import re

    from yolo_fastestv2_amd import _lib
    res, args = _lib._PROTOTYPES["yfv2_debug_train_tensor"]
    assert res == C.c_int64 and args == [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64]
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "yfv2.h")).read()
    assert re.search(r"YFV2_API int64_t yfv2_debug_train_tensor\(yfv2_handle h, const char\* name, int32_t which, float\* host_dst, int64_t capacity\);", header)
    assert _lib.lib().yfv2_debug_train_tensor(None, b"x", 0, None, 0) == -1          # no handle: refused, nothing dereferenced
