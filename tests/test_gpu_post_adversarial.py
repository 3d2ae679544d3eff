"""Crafted inputs through every post-processing launch (tests/adversarial_post.py).

(a) yfv2_nms (nms_kernel<0>, two and four sort keys per thread) on crafted decoded rows, bit-exact against the reference's own
    non_max_suppression (golden_post_adversarial.npz) at conf 0.3 / 0.01 / 0.0 / -1.0, iou 0.4 / 0.5 / 0.0 / -0.1 / 1.0, with
    and without a class filter, 80 and 255 classes.
(b) crafted logits through the three forms yfv2_detect and its callers use: Engine.post on the default plan (the fused decode
    + NMS launch where classes <= 96 and rows <= 2048), Engine.post on the two-launch plan (decode_kernel<true> + nms_kernel<1>),
    and decode + nms (decode_kernel<false> + nms_kernel<0>): rows, indices and counts bit-identical.
(c) the same logits against the oracle: the three-call NMS equals oracle.non_max_suppression on the device's own decoded
    tensor, bit for bit, and that tensor is within DECODE_ULP of oracle.decode on the finite cases.
Bit-exact comparisons take any NaN as equal to any NaN (payload and sign are specified by neither side)."""
import os

import numpy as np
import pytest
import torch

import adversarial_post as A
from conftest import GOLDEN
from oracle import yfv2_oracle as oracle
from test_gpu_parity import DECODE_ULP, _ulp_distance

pytestmark = pytest.mark.gpu

SIZE_OF_ROWS = {1815: 352, 3840: 512}
# (b) / (c): every class count at 352 x 352, every size at 80 classes, and a few crossings (97 / 255 classes and 512 x 512: two
# launches on either plan)
LOGIT_CONFIGS = ([(nc, (352, 352)) for nc in (1, 2, 3, 4, 5, 80, 93, 96, 97, 255)] +
                 [(80, hw) for hw in ((320, 320), (32, 32), (64, 96), (352, 32), (288, 384), (512, 512))] +
                 [(3, (32, 32)), (96, (288, 384)), (97, (64, 96)), (255, (512, 512))])
POST_THRES = ((0.3, 0.4), (0.0, 0.5), (-1.0, 0.45))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_post_adversarial.npz")))


def _engine(dev, h, w, nc, B, plan=None):
    import yolo_fastestv2_amd as yfv2
    return yfv2.Engine(dev, h, w, nc, 3, anchors=A.ANCHORS, max_batch=B, plan=plan if plan is not None else {})


def _host(dets, idx, cnt):
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    d, i = dets.cpu().numpy(), idx.cpu().numpy()
    return [d[b, :c[b]] for b in range(len(c))], [i[b, :c[b]] for b in range(len(c))]


@pytest.mark.parametrize("c", range(len(A.DECODED_CONFIGS)), ids=["%d-rows-%d-classes" % rc for rc in A.DECODED_CONFIGS])
def test_nms_on_crafted_rows_vs_reference_golden(dev, golden, c):
    rows, nc = A.DECODED_CONFIGS[c]
    dec = A.decoded_batch(rows, nc)
    assert np.array_equal(A.probe(dec), golden["probe%d" % c])
    s = SIZE_OF_ROWS[rows]
    eng = _engine(dev, s, s, nc, dec.shape[0])
    assert eng.rows == rows
    d_dec = torch.from_numpy(dec).to(dev)
    bad = []
    for a, ct in enumerate(A.CONF_THRES):
        for i, it in enumerate(A.IOU_THRES):
            for f, cl in enumerate(A.CLASS_FILTER):
                got_rows, got_idx = _host(*eng.nms(d_dec, ct, it, classes=cl))
                for b in range(dec.shape[0]):
                    g_rows, g_idx = A.golden_result(golden, c, a, i, f, b)
                    if not (A.same_bits(got_rows[b], g_rows) and np.array_equal(got_idx[b], g_idx)):
                        bad.append((A.DECODED_CASES[b][0], ct, it, cl, len(got_idx[b]), len(g_idx)))
    assert not bad, bad[:10]


def _logits(nc, h, w):
    per_case = [A.logit_batch(case, nc, h, w) for case in A.LOGIT_CASES]
    return [np.concatenate([p[k] for p in per_case]) for k in range(6)], len(per_case[0][0])


@pytest.mark.parametrize("nc,hw", LOGIT_CONFIGS, ids=["%d-classes-%dx%d" % (nc, hw[0], hw[1]) for nc, hw in LOGIT_CONFIGS])
def test_crafted_logits_three_forms_and_oracle(dev, nc, hw):
    h, w = hw
    host, per = _logits(nc, h, w)
    B = host[0].shape[0]
    fused = _engine(dev, h, w, nc, B)
    two = _engine(dev, h, w, nc, B, plan={"post_two_launches": 1})
    preds = [torch.from_numpy(p).to(dev) for p in host]
    dec_dev = fused.decode(preds)
    dec = dec_dev.cpu().numpy()
    bad = []
    for ct, it in POST_THRES:
        r1, i1 = _host(*fused.post(preds, ct, it))
        r2, i2 = _host(*two.post(preds, ct, it))
        r3, i3 = _host(*fused.nms(dec_dev, ct, it))
        with np.errstate(invalid="ignore"):
            o_rows, o_idx = oracle.non_max_suppression(dec, ct, it)
        for b in range(B):
            case = A.LOGIT_CASES[b // per]
            for name, r, i in (("fused post", r1, i1), ("two-launch post", r2, i2), ("oracle on the device's decode", o_rows, o_idx)):
                if not (A.same_bits(r[b], r3[b]) and np.array_equal(i[b], i3[b])):
                    bad.append((name, case, b, ct, it, len(i[b]), len(i3[b])))
    assert not bad, bad[:10]

    # decode against the oracle on the finite cases: DECODE_ULP as test_gpu_parity.test_decode_from_golden_logits applies it
    finite = np.asarray([A.LOGIT_CASES[b // per] != A.NONFINITE_CASE for b in range(B)])
    ref = oracle.decode([torch.from_numpy(p[finite]) for p in host], A.ANCHORS, h)
    got = dec[finite]
    d = _ulp_distance(got, ref)
    n0 = 3 * (h // 16) * (w // 16)
    stride = np.where(np.arange(ref.shape[1]) < n0, 16.0, 32.0)[None, :, None]
    err = np.abs(got[..., :2].astype(np.float64) - ref[..., :2]) - 1.5 * np.spacing(np.abs(ref[..., :2]).astype(np.float32))
    centre = float((np.maximum(err, 0.0) / (2.0 ** -24 * 2.0 * stride)).max())
    tiny = np.abs(ref[..., 4:]) < 1e-30          # a denormal's last place says nothing: compared absolutely
    assert np.abs(got[..., 4:][tiny].astype(np.float64) - ref[..., 4:][tiny]).max(initial=0.0) <= 1e-35
    dd = d[..., 4:]
    worst = {"centre_in_sigmoid_ulp": centre, "size": int(d[..., 2:4].max()), "obj": int(dd[..., 0][~tiny[..., 0]].max(initial=0)),
             "cls": int(dd[..., 1:][~tiny[..., 1:]].max(initial=0))}
    assert all(worst[k] <= v for k, v in DECODE_ULP.items()), worst
