#!/usr/bin/env python3
"""One case of tests/plan_cases.py on the device, run in its OWN interpreter by tests/test_gpu_plans.py (these kernels have never
run at these shapes outside the default plan: a fault in here must end this child and not the GPU test run).  A progress marker
after every stage, one JSON line of figures at the end, then PLAN CASE OK.  usage: plan_shapes.py CASE_INDEX

forward cases: the handle runs the launch sequence the host dry run names for the case; fp32 and uint8 entries within the
               noise floor of the oracle (tests/noise_floor.py); range guard quiet; detect == nms(decode(forward)) bit for bit at
               conf 0.3 and 0.01; NMS of the device's decoded tensor == the oracle's bit for bit; decode within class_counts.py's
               bounds; every image keeps a detection at 0.01; towers_unpaired: logits bit-equal to the default plan's
batch cases:   B images in one call == the same handle on three chunks of B / 3, bit for bit (logits and detections); images 0 and
               B - 1 within the noise floor
post cases:    detect on the post_two_launches handle == detect on a default-plan handle bit for bit, on the case's images and
               on a synthetic logit set in which every row is a candidate (Engine.post, the launches detect runs)"""
import faulthandler
import json
import os
import sys

faulthandler.enable()
TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import noise_floor  # noqa: E402
import plan_cases  # noqa: E402
import yolo_fastestv2_amd as yfv2  # noqa: E402
from oracle import yfv2_oracle as oracle  # noqa: E402

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]
THRESHOLDS = ((0.3, 0.4), (0.01, 0.4))
FRONT_FUSED = "stem + backbone.stage2.0 in one launch"


def mark(msg):
    print("[plan_shapes] " + msg, flush=True)


def engine(dev, c, plan, weights):
    eng = yfv2.Engine(dev, c.H, c.W, c.classes, 3, anchors=ANCHORS, max_batch=c.B, plan=plan)
    eng.load_state_dict(weights)
    return eng


def check_launch_sequence(eng, c, plan):
    """the handle's launches are the ones the dry run named for this case; returns their number"""
    want = list(plan_cases.launch_sequence(plan, c.classes, c.H, c.W))
    got = [plan_cases.strip_geometry(s["name"]) for s in eng.stages()]
    if len(want) == len(got) + 1:     # include/yfv2.h yfv2_debug_plan_image: the view keeps the fused front's two images as two steps
        assert got[0].startswith(FRONT_FUSED), got[0]
        assert got[1:] == want[2:], "launches differ from the dry run's:\n%s\n%s" % (got, want)
    else:
        assert not got[0].startswith(FRONT_FUSED), got[0]
        assert got == want, "launches differ from the dry run's:\n%s\n%s" % (got, want)
    return len(got)


def host_dets(dets, idx, cnt):
    torch.cuda.synchronize()
    n = cnt.cpu().numpy()
    d, i = dets.cpu().numpy(), idx.cpu().numpy()
    return [d[b, :n[b]].copy() for b in range(len(n))], [i[b, :n[b]].astype(np.int64) for b in range(len(n))]


def assert_same_dets(a, b, what):
    assert len(a[0]) == len(b[0]), what
    for k, (ra, rb, ia, ib) in enumerate(zip(a[0], b[0], a[1], b[1])):
        assert ra.shape == rb.shape, "%s: image %d keeps %d against %d" % (what, k, ra.shape[0], rb.shape[0])
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), "%s: rows differ, image %d" % (what, k)
        assert np.array_equal(ia, ib), "%s: indices differ, image %d" % (what, k)


def floor_figures(st):
    return {k: [float("%.4g" % v) for v in vals] for k, vals in st.items()}      # device max, device rms, reference max, reference rms


def uint8_images(c):
    g = torch.Generator().manual_seed(c.image_seed * 7 + 1)
    x8 = torch.randint(0, 256, (c.B, c.H, c.W, 3), generator=g, dtype=torch.uint8)
    x8[0, : c.H // 2] = 255                      # saturated / black halves: the largest accumulators, exact zeros
    x8[c.B - 1, :, : c.W // 2] = 0
    return x8


def refs_of(w, x):
    return [t.numpy() for t in oracle.forward64(w, x)], [t.numpy() for t in oracle.forward(w, x)]


def run_forward(c, dev, w, x, fig):
    mark("oracle forward")
    refs = refs_of(w, x)
    x8 = uint8_images(c)
    xf8 = x8.permute(0, 3, 1, 2).float() / 255.0      # the fp32 tensor the reference would see (float() / 255 in fp32)
    refs8 = refs_of(w, xf8)
    mark("engine")
    eng = engine(dev, c, c.plan, w)
    fig["launches"] = check_launch_sequence(eng, c, c.plan)
    mark("launch sequence ok")
    xd = x.to(dev)
    got = [t.clone() for t in eng.forward(xd)]
    torch.cuda.synchronize()
    mark("forward done")
    fig["fp32"] = floor_figures(noise_floor.assert_logits_within_noise_floor(got, w, x, plan_cases.case_id(c), refs=refs))
    mark("logits ok")
    got8 = [t.clone() for t in eng.forward(x8.to(dev))]
    torch.cuda.synchronize()
    mark("uint8 forward done")
    fig["uint8"] = floor_figures(noise_floor.assert_logits_within_noise_floor(got8, w, xf8, plan_cases.case_id(c) + " uint8", refs=refs8))
    assert not eng.nonfinite(), "the range guard tripped"
    mark("uint8 logits ok")
    if c.plan == plan_cases.UNPAIRED:
        base = engine(dev, c, {}, w)
        assert [s["name"] for s in base.stages()] != [s["name"] for s in eng.stages()]
        for k, a, b in zip(noise_floor.LOGIT_KEYS, got, base.forward(xd)):
            assert torch.equal(a, b), "%s differs from the default plan's" % k
        mark("bit-equal to the default plan")
    dec_d = eng.decode(got)
    dec = dec_d.cpu()
    rows_n = 3 * ((c.H // 16) * (c.W // 16) + (c.H // 32) * (c.W // 32))
    assert tuple(dec.shape) == (c.B, rows_n, 5 + c.classes)
    o_dec = oracle.decode([t.cpu() for t in got], ANCHORS, c.H)
    d = np.abs(dec.numpy().astype(np.float64) - o_dec.astype(np.float64))
    assert (d[..., :4] <= 1e-4 * np.maximum(1.0, np.abs(o_dec[..., :4]))).all(), "decoded boxes: worst %g" % d[..., :4].max()
    assert d[..., 4:].max() <= 1e-5, "decoded scores: worst %g" % d[..., 4:].max()
    mark("decode ok")
    fig["kept"] = {}
    for conf, iou in THRESHOLDS:
        fused = host_dets(*eng.detect(xd, conf, iou))
        three = host_dets(*eng.nms(eng.decode(eng.forward(xd)), conf, iou))
        assert_same_dets(fused, three, "detect against nms(decode(forward)) at conf %g" % conf)
        rows, idx = yfv2.nms_with_indices(dec, conf, iou)
        o_rows, o_idx = oracle.non_max_suppression(dec.numpy(), conf, iou)
        assert_same_dets(([r.numpy() for r in rows], [np.asarray(i, np.int64) for i in idx]), (o_rows, o_idx), "NMS against the oracle at conf %g" % conf)
        assert_same_dets(three, (o_rows, o_idx), "the handle's own NMS against the oracle at conf %g" % conf)
        fig["kept"]["%g" % conf] = [int(r.shape[0]) for r in o_rows]
        mark("post ok at conf %g: kept %s" % (conf, fig["kept"]["%g" % conf]))
    assert min(fig["kept"]["0.01"]) >= 1, "an image keeps no detection at conf 0.01: the post checks are vacuous"
    assert not eng.nonfinite()


def run_batch(c, dev, w, x, fig):
    ends = x[[0, c.B - 1]]
    mark("oracle forward")
    refs = refs_of(w, ends)
    mark("engine")
    eng = engine(dev, c, c.plan, w)
    fig["launches"] = check_launch_sequence(eng, c, c.plan)
    xd = x.to(dev)
    whole = [t.clone() for t in eng.forward(xd)]
    whole_det = {conf: host_dets(*eng.detect(xd, conf, iou)) for conf, iou in THRESHOLDS}
    torch.cuda.synchronize()
    mark("batch of %d done" % c.B)
    n = c.B // 3
    for k in range(3):
        part = eng.forward(xd[k * n:(k + 1) * n])
        for key, a, b in zip(noise_floor.LOGIT_KEYS, whole, part):
            assert torch.equal(a[k * n:(k + 1) * n], b), "%s: images %d..%d differ between the batch of %d and a chunk of %d" % (key, k * n, (k + 1) * n - 1, c.B, n)
        for conf, iou in THRESHOLDS:
            got = host_dets(*eng.detect(xd[k * n:(k + 1) * n], conf, iou))
            assert_same_dets((whole_det[conf][0][k * n:(k + 1) * n], whole_det[conf][1][k * n:(k + 1) * n]), got, "chunk %d at conf %g" % (k, conf))
    mark("chunks ok")
    fig["kept"] = {"%g" % conf: [int(sum(r.shape[0] for r in whole_det[conf][0]))] for conf, _ in THRESHOLDS}
    assert min(r.shape[0] for r in whole_det[0.01][0]) >= 1, "an image keeps no detection at conf 0.01"
    fig["fp32"] = floor_figures(noise_floor.assert_logits_within_noise_floor([t[[0, c.B - 1]] for t in whole], w, ends, plan_cases.case_id(c), refs=refs))
    assert not eng.nonfinite(), "the range guard tripped"
    mark("logits ok")


def all_candidate_logits(c, dev):
    """two images of logits in which EVERY row passes conf 0.3, as class_counts.py builds its stress rows: objectness in (0.32, 1), one
    hot class per row with a softmax share of about 0.98, boxes several cells wide (every box overlaps its neighbours), exact score
    ties on every seventh cell of image 1"""
    g = torch.Generator().manual_seed(11)
    out = []
    for s in (16, 32):
        h, w = c.H // s, c.W // s
        reg = torch.randn(2, 12, h, w, generator=g)
        reg[:, 2::4] = -1.0 + 3.0 * torch.rand(2, 3, h, w, generator=g)
        reg[:, 3::4] = -1.0 + 3.0 * torch.rand(2, 3, h, w, generator=g)
        p = 0.32 + 0.68 * torch.rand(2, 3, h, w, generator=g)
        p.clamp_(max=0.9999)
        obj = torch.log(p / (1.0 - p))
        obj[1].view(-1)[::7] = float(np.log(3.0))            # sigmoid = 0.75
        cls = 0.01 * torch.rand(2, c.classes, h, w, generator=g)
        hot = torch.randint(0, c.classes, (2, 1, h, w), generator=g)
        few = torch.rand(2, 1, h, w, generator=g) < 0.75         # three cells of four share four classes: the greedy walk suppresses
        hot = torch.where(few, hot % min(c.classes, 4), hot)
        cls.scatter_(1, hot, float(np.log(max(c.classes - 1, 1))) + 4.0 + 0.5 * torch.rand(2, 1, h, w, generator=g))
        out += [reg, obj, cls]
    return [t.contiguous().to(dev) for t in out]


def run_post(c, dev, w, x, fig):
    mark("engines")
    two = engine(dev, c, c.plan, w)
    one = engine(dev, c, {}, w)
    fig["launches"] = check_launch_sequence(two, c, c.plan)
    xd = x.to(dev)
    fig["kept"] = {}
    for conf, iou in THRESHOLDS:
        a, b = host_dets(*two.detect(xd, conf, iou)), host_dets(*one.detect(xd, conf, iou))
        assert_same_dets(a, b, "two-launch detect against the fused launch at conf %g" % conf)
        fig["kept"]["%g" % conf] = [int(r.shape[0]) for r in a[0]]
    assert min(fig["kept"]["0.01"]) >= 1, "an image keeps no detection at conf 0.01"
    mark("images ok: kept %s" % fig["kept"])
    syn = all_candidate_logits(c, dev)
    dec = one.decode(syn).cpu().numpy()
    cand = (dec[..., 4:5] * dec[..., 5:]).max(-1) > np.float32(0.3)
    assert cand.all(), "%d of %d synthetic rows are no candidates" % (int((~cand).sum()), cand.size)
    fig["kept_synthetic"] = {}
    for conf, iou in THRESHOLDS:
        a, b = host_dets(*two.post(syn, conf, iou)), host_dets(*one.post(syn, conf, iou))
        assert_same_dets(a, b, "all rows candidates: two-launch post against the fused launch at conf %g" % conf)
        assert_same_dets(a, oracle.non_max_suppression(dec, conf, iou), "all rows candidates: post against the oracle at conf %g" % conf)
        fig["kept_synthetic"]["%g" % conf] = [int(r.shape[0]) for r in a[0]]
        assert min(fig["kept_synthetic"]["%g" % conf]) >= 1
    mark("all-candidates post ok: %d candidates -> %s" % (dec.shape[1], fig["kept_synthetic"]))
    assert not two.nonfinite() and not one.nonfinite()


def main():
    index = int(sys.argv[1])
    c = plan_cases.CASES[index]
    dev = torch.device("cuda:0")
    mark("case %d %s" % (index, plan_cases.case_id(c)))
    w = yfv2.random_state_dict(c.weight_seed, classes=c.classes)
    x = torch.rand(c.B, 3, c.H, c.W, generator=torch.Generator().manual_seed(c.image_seed))
    fig = {"case": plan_cases.case_id(c)}
    {"forward": run_forward, "batch": run_batch, "post": run_post}[c.kind](c, dev, w, x, fig)
    print("FIGURES " + json.dumps(fig, sort_keys=True), flush=True)
    print("PLAN CASE OK %s" % plan_cases.case_id(c), flush=True)


if __name__ == "__main__":
    main()
