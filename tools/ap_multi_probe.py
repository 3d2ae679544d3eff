#!/usr/bin/env python3
"""Average precision at K = 10 IoU thresholds in one device pass (Engine.batch_statistics_multi + Engine.ap_per_class_multi) against
ten rounds of the single-threshold entry points (Engine.batch_statistics + Engine.ap_per_class) in the same process.

Workload: tools/ap_probe.py's - --rows (default 1 500 000: 5 000 images x 300 detections) over 80 classes, 36 000 targets, once with
uniform classes and once with 30 % of the rows in one class.
  matching   the 5 000 images in batches of --batch (default 100), 300 seeded detections each, about 7 targets per image (jittered
             copies of detections); one launch per batch (multi) against ten (single), enqueue only, one wait at the end
  ap         one ap_per_class_multi call against ten ap_per_class calls on the ten bit planes (each waits for its stream); the
             mask's bit k is set with a density that falls with k, as a rising threshold gives
Per case: median wall clock in ms of --repeats after --warmup rounds for each of the four, `multi_ms` / `single_x10_ms` = matching +
ap, and `ratio` = single_x10_ms / multi_ms.  The results of the two paths are compared bit for bit before anything is timed.
Prints one JSON line.   usage: python tools/ap_multi_probe.py [--rows 1500000] [--repeats 5] [--warmup 2] > profiles/ap_multi_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K = 10
CASES = ("uniform", "skew")


def ap_workload(n, case, seed):
    rng = np.random.default_rng(seed)
    conf = rng.random(n).astype(np.float32)
    cls = rng.integers(0, 80, n).astype(np.float32)
    if case == "skew":
        cls[rng.random(n) < 0.3] = 0.0
    mask = np.zeros(n, np.uint32)
    for k in range(K):
        mask |= (rng.random(n) < 0.4 * (1 - k / (K + 1.0))).astype(np.uint32) << np.uint32(k)
    labels = rng.integers(0, 80, 36000).astype(np.float32)
    return mask.view(np.int32), conf, cls, labels


def match_workload(images, batch, seed, dev):
    import torch
    g = torch.Generator().manual_seed(seed)
    out = []
    for lo in range(0, images, batch):
        b = min(batch, images - lo)
        xy = torch.randint(0, 300, (b, 300, 2), generator=g).float()
        wh = torch.randint(10, 90, (b, 300, 2), generator=g).float()
        conf = torch.rand((b, 300, 1), generator=g).sort(1, descending=True).values
        lab = torch.randint(0, 80, (b, 300, 1), generator=g).float()
        dets = torch.cat([xy, xy + wh, conf, lab], 2)
        src = dets[:, :7]
        box = src[..., :4] + torch.randint(-8, 9, (b, 7, 4), generator=g).float()
        img = torch.arange(b).float()[:, None, None].expand(b, 7, 1)
        targets = torch.cat([img, src[..., 5:6], box], 2).reshape(-1, 6)
        out.append((dets.contiguous().to(dev), torch.full((b,), 300, dtype=torch.int32).to(dev), targets.contiguous().to(dev)))
    return out


def median_ms(fn, warmup, repeats):
    import torch
    times = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1500000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    import yolo_fastestv2_amd as yfv2
    dev = torch.device("cuda:0")
    eng = yfv2.Engine(dev, 64, 64, 2, 3, plan={})
    thr = np.linspace(0.5, 0.95, K).astype(np.float32)
    res = {"tool": "ap_multi_probe", "rows": args.rows, "K": K, "classes": 80, "targets": 36000, "batch": args.batch,
           "repeats": args.repeats, "warmup": args.warmup}

    batches = match_workload(args.rows // 300, args.batch, args.seed, dev)
    for dets, cnt, tg in batches[:2]:     # the two paths agree before they are timed
        m = eng.batch_statistics_multi(dets, cnt, tg, thr)
        for k in range(K):
            assert torch.equal((m >> k) & 1, eng.batch_statistics(dets, cnt, tg, float(thr[k]))), "matching: bit %d differs" % k
    match_multi = median_ms(lambda: [eng.batch_statistics_multi(d, c, t, thr, sync=False) for d, c, t in batches], args.warmup, args.repeats)
    match_single = median_ms(lambda: [eng.batch_statistics(d, c, t, float(x), sync=False) for d, c, t in batches for x in thr], args.warmup, args.repeats)
    assert eng.stats_overflowed() == 0
    res["matching"] = {"launches_multi": len(batches), "launches_single": K * len(batches), "multi_ms": match_multi, "single_x10_ms": match_single,
                       "ratio": round(match_single / match_multi, 2)}

    for case in CASES:
        mask, conf, cls, labels = ap_workload(args.rows, case, args.seed)
        dv = [torch.from_numpy(a).to(dev) for a in (mask, conf, cls, labels)]
        planes = [((dv[0] >> k) & 1).contiguous() for k in range(K)]
        outs = eng.ap_per_class_multi(*dv, K)
        for k in range(K):
            one = eng.ap_per_class(planes[k], *dv[1:])
            assert all(np.array_equal(outs[k][key].view(np.uint64), one[key].view(np.uint64)) for key in ("p", "r", "ap")) and outs[k]["means"] == one["means"], \
                "ap: record %d differs" % k
        ap_multi = median_ms(lambda: eng.ap_per_class_multi(*dv, K), args.warmup, args.repeats)
        ap_single = median_ms(lambda: [eng.ap_per_class(p, *dv[1:]) for p in planes], args.warmup, args.repeats)
        multi, single = match_multi + ap_multi, match_single + ap_single
        res[case] = {"largest_class_rows": int(outs[0]["n_pred"].max()), "mean_ap_per_threshold": [o["means"][2] for o in outs],
                     "ap_multi_ms": ap_multi, "ap_single_x10_ms": ap_single, "ap_ratio": round(ap_single / ap_multi, 2),
                     "multi_ms": round(multi, 3), "single_x10_ms": round(single, 3), "ratio": round(single / multi, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
