#!/usr/bin/env python3
"""Crops as network input (Engine.crop_tensors, include/yfv2.h yfv2_crop_tensors_u8) against what it replaces.

Workload: tools/crops_probe.py's - four frames generated on the device, 1920x1080, 1280x720, 854x480 and 352x352, 300 seeded
detection rows each; crops of --out x --out pixels (default 128), pad 0.1: 1200 crops.  After a warm-up of every variant, in ONE
process, the variants run in alternation for --rounds rounds of --iters calls each (device events around each block; the median
over the rounds and the min .. max spread are reported):
  tensors_f32 / _f16            (a) crop_tensors, stretch form, ImageNet mean / std, planes R, G, B
  tensors_f32_lb / _f16_lb      ... the letterbox form of the same call
  glue_f32 / _f16               (b) what it replaces: crop_detections, then the torch glue
                                    crops.permute(0, 3, 1, 2).float().div(255).sub(mean).div(std) [.half()] - planes B, G, R, the
                                    glue's cheapest form (a channel flip would be one more pass)
  crops_u8                      (c) crop_detections alone
Every variant writes into preallocated outputs where it can (the glue's intermediates are torch's own).  The stretch tensors are
compared with the glue's result bit for bit (same plane order for the comparison).  bytes_written: what each variant's final
output is, and for the glue every pass's writes.  Prints one JSON line and writes it to --json (default
profiles/crop_tensors_probe.json).
usage: python tools/crop_tensors_probe.py [--out 128] [--iters 50] [--rounds 15] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import yolo_fastestv2_amd as yfv2  # noqa: E402

SIZES = ((1080, 1920), (720, 1280), (480, 854), (352, 352))
R = 300
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def rows(rng, h, w):
    cx, cy = rng.uniform(0, w, R), rng.uniform(0, h, R)
    bw, bh = rng.uniform(0.02, 0.4, R) * w, rng.uniform(0.02, 0.4, R) * h
    conf = np.sort(rng.uniform(0.3, 1.0, R))[::-1]
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2, conf, rng.integers(0, 80, R).astype(np.float64)], 1).astype(np.float32)


def block_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=int, default=128)
    ap.add_argument("--pad", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=os.path.join(REPO, "profiles", "crop_tensors_probe.json"))
    args = ap.parse_args()

    assert torch.cuda.is_available(), "crop_tensors_probe.py measures on the GPU: no device found"
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
    mean_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device=dev).view(1, 3, 1, 1)

    u8 = eng.crop_detections(frames, dets, count, size, pad=args.pad, cap=cap)
    outs = {(dt, lb): eng.crop_tensors(frames, dets, count, size, dtype=dt, letterbox=lb, pad=args.pad, cap=cap)
            for dt in (torch.float32, torch.float16) for lb in (False, True)}

    def tensors(dt, lb, rgb=True):
        return lambda: eng.crop_tensors(frames, dets, count, size, mean=MEAN, std=STD, rgb=rgb, letterbox=lb, fill=(114, 114, 114), dtype=dt,
                                        pad=args.pad, cap=cap, out=outs[(dt, lb)])

    def crops():
        return eng.crop_detections(frames, dets, count, size, pad=args.pad, cap=cap, out=u8)

    def glue(half):
        def run():
            t = crops()[0].permute(0, 3, 1, 2).float().div(255).sub(mean_t).div(std_t)
            return t.half() if half else t
        return run

    variants = {"tensors_f32": tensors(torch.float32, False), "glue_f32": glue(False), "crops_u8": crops,
                "tensors_f16": tensors(torch.float16, False), "glue_f16": glue(True),
                "tensors_f32_lb": tensors(torch.float32, True), "tensors_f16_lb": tensors(torch.float16, True)}
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()

    # the same values: the stretch form in the glue's plane order against the glue, bit for bit
    n = int(u8[3][-1])
    same = {}
    for half, dt in ((False, torch.float32), (True, torch.float16)):
        got = tensors(dt, False, rgb=False)()[0][:n].clone()
        ref = glue(half)()[:n]
        bits = torch.int32 if dt == torch.float32 else torch.int16
        ref = ref.contiguous()
        same["f16" if half else "f32"] = {"equal": bool(torch.equal(got.view(bits), ref.view(bits))),
                                          "differing_values": int((got.view(bits) != ref.view(bits)).sum()),
                                          "max_abs_diff": float((got.float() - ref.float()).abs().max())}
    torch.cuda.synchronize()

    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(block_ms(fn, args.iters))
    px = n * args.out * args.out * 3
    written = {"crops_u8": px, "tensors_f32": 4 * px, "tensors_f16": 2 * px, "glue_f32": px + 4 * 4 * px, "glue_f16": px + 4 * 4 * px + 2 * px}
    res = {"tool": "crop_tensors_probe", "frames": ["%dx%d" % (w, h) for h, w in SIZES], "rows_per_frame": R, "out": "%dx%d" % size, "pad": args.pad,
           "crops": n, "iters": args.iters, "rounds": args.rounds, "tensors_equal_glue_bits": same,
           "median_ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
           "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()}, "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
           "bytes_per_crop": {"u8": args.out * args.out * 3, "f32": args.out * args.out * 12, "f16": args.out * args.out * 6},
           "bytes_written": written}
    med = res["median_ms"]
    res["glue_over_tensors"] = {"f32": round(med["glue_f32"] / med["tensors_f32"], 2), "f16": round(med["glue_f16"] / med["tensors_f16"], 2)}
    res["tensors_write_GBps"] = {"f32": round(written["tensors_f32"] / med["tensors_f32"] / 1e6, 1), "f16": round(written["tensors_f16"] / med["tensors_f16"] / 1e6, 1)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
