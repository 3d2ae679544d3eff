#!/usr/bin/env python3
"""Second-stage crops (Engine.crop_detections, include/yfv2.h yfv2_crop_detections_u8) against the composition it replaces.

Workload: four frames generated on the device (nothing is read from disk) - 1920x1080, 1280x720, 854x480 and 352x352 - with 300
detection rows each: seeded boxes of 2 % to 40 % of the frame's sides, some crossing an edge, conf-descending, classes 0..79.
Crops of --out x --out pixels (default 128), pad 0.1.  After a warm-up, in ONE process:
  crop_detections  the one call: frame table, two plan launches, the resize launch over the capacity; device events over --iters
  composition      what a caller does without it: dets and count to the host (which waits for the device), the rule in Python
                   (tests/crops_model.py), torch views of the frames, a second engine's resize_frames on the views; wall-clock
                   over --host-iters, since the host step needs the results anyway.  composition_host_ms is the copy and the
                   Python rule alone, composition_resize_ms the second engine's call alone (device events).
The two results are compared byte for byte.  Prints one JSON line and writes it to --json (default profiles/crops_probe.json).
usage: python tools/crops_probe.py [--out 128] [--iters 50] [--host-iters 3] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import yolo_fastestv2_amd as yfv2  # noqa: E402

SIZES = ((1080, 1920), (720, 1280), (480, 854), (352, 352))
R = 300


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rows(rng, h, w):
    cx, cy = rng.uniform(0, w, R), rng.uniform(0, h, R)
    bw, bh = rng.uniform(0.02, 0.4, R) * w, rng.uniform(0.02, 0.4, R) * h
    conf = np.sort(rng.uniform(0.3, 1.0, R))[::-1]
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2, conf, rng.integers(0, 80, R).astype(np.float64)], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=int, default=128)
    ap.add_argument("--pad", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=os.path.join(REPO, "profiles", "crops_probe.json"))
    args = ap.parse_args()

    import crops_model
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    frames = [torch.randint(0, 256, (h, w, 3), generator=gen, device=dev, dtype=torch.uint8) for h, w in SIZES]
    rng = np.random.default_rng(args.seed)
    B = len(SIZES)
    dets = torch.from_numpy(np.stack([rows(rng, h, w) for h, w in SIZES])).to(dev)
    count = torch.full((B,), R, device=dev, dtype=torch.int32)
    size = (args.out, args.out)
    cap = B * R
    eng = yfv2.Engine(dev, 352, 352, max_batch=B, plan={})
    second = yfv2.Engine(dev, args.out, args.out, max_batch=cap, plan={})
    out = eng.crop_detections(frames, dets, count, size, pad=args.pad, cap=cap)
    out2 = torch.empty((cap, args.out, args.out, 3), device=dev, dtype=torch.uint8)

    def run_call():
        eng.crop_detections(frames, dets, count, size, pad=args.pad, cap=cap, out=out)

    host_ms, state = [], {}

    def run_composition():
        t0 = time.perf_counter()
        d, c = dets.cpu().numpy(), count.cpu().numpy()            # waits for the device
        p = crops_model.plan(d, c, SIZES, args.pad, args.pad)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        views = [frames[b][y0:y0 + h, x0:x0 + w] for b, (x0, y0, w, h) in zip(p["frame"].tolist(), p["rect"].tolist())]
        state["views"], state["plan"] = views, p
        return second.resize_frames(views, out=out2[:len(views)])

    for _ in range(args.warmup):
        run_call()
    ref = run_composition()
    torch.cuda.synchronize()
    p = state["plan"]
    n = len(state["views"])
    same = (int(out[3][-1]) == n and bool(torch.equal(out[0][:n], ref)) and np.array_equal(out[1][:n].cpu().numpy(), p["src"])
            and np.array_equal(out[2][:n].cpu().numpy(), p["rect"]) and np.array_equal(out[3].cpu().numpy(), p["offset"])
            and np.array_equal(out[4].cpu().numpy(), p["skipped"]))

    ms_call = timed(run_call, args.iters)
    ms_resize = timed(lambda: second.resize_frames(state["views"], out=out2[:n]), max(args.host_iters, 3))
    host_ms.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        run_composition()
        torch.cuda.synchronize()
    ms_comp = (time.perf_counter() - t0) * 1e3 / args.host_iters

    res = {"tool": "crops_probe", "frames": ["%dx%d" % (w, h) for h, w in SIZES], "rows_per_frame": R, "out": "%dx%d" % size, "pad": args.pad,
           "crops": n, "skipped": int(p["skipped"].sum()), "iters": args.iters, "host_iters": args.host_iters,
           "crop_detections_equals_composition": same,
           "crop_detections_ms": round(ms_call, 4), "crops_per_s": round(n / ms_call * 1e3, 0),
           "composition_ms": round(ms_comp, 2), "composition_host_ms": round(float(np.mean(host_ms)), 2), "composition_resize_ms": round(ms_resize, 4),
           "speedup": round(ms_comp / ms_call, 1)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
