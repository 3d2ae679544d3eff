#!/usr/bin/env python3
"""Training batches on the device (Engine.train_batch_frames / train_batch_frames_yuv, include/yfv2.h yfv2_train_batch_frames_u8 /
_yuv) against the chain they replace, on the same machine in the same process.

Workload: a seeded batch of --frames frames (default 64, the training batch of DESIGN.md 4.3) mixing 1920x1080, 1280x720, 640x480
and 352x352 in shuffled order (tools/frames_probe.py's mix), generated on the device, as packed B, G, R and as NV12 planes; one
contrast / brightness pair per frame drawn as utils/datasets.py:11-12 draws them (random.Random(seed)).
  (a) new_bgr / new_nv12      the one launch: resize + table + NCHW fp32
  (b) chain_bgr / chain_nv12  Engine.resize_frames(_yuv) -> the per-frame 256-entry uint8 table applied by torch indexing ->
                              .permute(0, 3, 1, 2).float() / 255  (train.py:101 on a device-resident uint8 batch)
  (c) the fp32 batch's bytes over (a) against the HBM roof, and the launch's algorithmic bytes (staged source rows + the batch)
Timing: device events on one stream around blocks of --iters calls, after --warmup calls of every variant; the variants alternate
inside each of --blocks rounds and the MEDIAN block is reported, with the spread.  (a) and (b) are also compared bit for bit: with
the division as the IEEE quotient (a tensor divisor; what torch computes on the host) they must be equal; as timed - `/ 255` by a
Python scalar, which torch evaluates on the device as a product with fl32(1 / 255) - the chain is one ulp off in about half the words.
Writes one JSON object to --out (default profiles/train_batch_probe.json) and prints it.
usage: python tools/train_batch_probe.py [--frames 64] [--iters 200] [--blocks 9] [--warmup 5] [--out PATH]
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import yolo_fastestv2_amd as yfv2  # noqa: E402

SIZES = [(1080, 1920), (720, 1280), (480, 640), (352, 352)]   # (h, w), as tools/frames_probe.py
HBM_PEAK = 8.0e12
H = W = 352
TRAIN_ITERATION_MS = 10.8                                      # DESIGN.md 4.3, batch 64


def make_frames(dev, n, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    order = np.random.default_rng(seed).permutation(np.arange(n) % len(SIZES))
    bgr = [torch.randint(0, 256, SIZES[k] + (3,), generator=gen, device=dev, dtype=torch.uint8) for k in order]
    nv12 = []
    for k in order:
        h, w = SIZES[k]
        y = torch.randint(0, 256, (h, w), generator=gen, device=dev, dtype=torch.uint8)
        uv = torch.randint(0, 256, (h // 2, w), generator=gen, device=dev, dtype=torch.uint8)
        nv12.append(yfv2.YuvFrame((y, uv), "nv12", "bt601"))
    return bgr, nv12


def byte_tables(alpha, beta):
    """(B, 256) uint8: contrast_and_brightness per byte, the statement of include/yfv2.h in fp32 torch ops on the host"""
    a = torch.arange(256, dtype=torch.float32)[None, :]
    t = a * torch.tensor(alpha, dtype=torch.float32)[:, None]
    t = t + torch.tensor(beta, dtype=torch.float32)[:, None]
    return torch.round(torch.clamp(t, 0.0, 255.0)).to(torch.uint8)          # torch.round: half to even


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
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_batch_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_batch_probe needs an MI355X: nothing here is measured without one")

    dev = torch.device("cuda:0")
    B = args.frames
    bgr, nv12 = make_frames(dev, B, args.seed)
    r = random.Random(args.seed)
    pairs = [yfv2.draw_contrast_brightness(r) for _ in range(B)]
    alpha, beta = [p[0] for p in pairs], [p[1] for p in pairs]
    eng = yfv2.Engine(dev, H, W, max_batch=B, plan={})
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    tables = byte_tables(alpha, beta).to(dev).reshape(-1)                    # (B * 256)
    base = (torch.arange(B, device=dev, dtype=torch.int64) * 256)[:, None, None, None]

    d255 = torch.tensor(255.0, device=dev)

    def chain(resize, frames, ieee=False):
        x = resize(frames, out=u8)
        x = tables[x.to(torch.int64) + base]                                 # the per-frame table by torch indexing
        x = x.permute(0, 3, 1, 2).float()
        # train.py:101 as written: on the device torch divides by a Python scalar by MULTIPLYING with fl32(1 / 255) - one ulp off the
        # IEEE quotient for 126 of the 256 bytes.  The rule (and torch on the host) is the quotient: a tensor divisor computes that.
        return x / d255 if ieee else x / 255

    runs = {
        "new_bgr": lambda: eng.train_batch_frames(bgr, alpha, beta, out=out),
        "new_nv12": lambda: eng.train_batch_frames_yuv(nv12, alpha, beta, out=out),
        "chain_bgr": lambda: chain(eng.resize_frames, bgr),
        "chain_nv12": lambda: chain(eng.resize_frames_yuv, nv12),
        "resize_bgr_alone": lambda: eng.resize_frames(bgr, out=u8),
        "resize_nv12_alone": lambda: eng.resize_frames_yuv(nv12, out=u8),
    }
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    same, scalar_diff = {}, {}
    for kind in ("bgr", "nv12"):
        a = runs["new_" + kind]().clone()
        frames, resize = (bgr, eng.resize_frames) if kind == "bgr" else (nv12, eng.resize_frames_yuv)
        b = chain(resize, frames, ieee=True).contiguous()
        same[kind] = bool(torch.equal(a, b))
        scalar = runs["chain_" + kind]().contiguous()
        scalar_diff[kind] = {"words_differing": int((scalar != a).sum()), "of": a.numel(), "max_abs": float((scalar - a).abs().max())}
    blocks = {k: [] for k in runs}
    for _ in range(args.blocks):
        for k, fn in runs.items():
            blocks[k].append(block_ms(fn, args.iters))

    batch_bytes = B * 3 * H * W * 4
    staged = {"bgr": sum(H * 2 * 3 * int(f.shape[1]) for f in bgr),          # two source rows per output row
              "nv12": sum(H * 3 * f.width for f in nv12)}                     # two luma rows and at least one chroma row
    res = {"tool": "train_batch_probe", "frames": B, "mix": ["%dx%d" % (w, h) for h, w in SIZES], "network": "%dx%d" % (W, H),
           "iters_per_block": args.iters, "blocks": args.blocks, "warmup": args.warmup, "timing": "device events, median block",
           "new_equals_chain_with_ieee_division": same, "chain_with_torch_device_scalar_division_vs_new": scalar_diff, "fp32_batch_bytes": batch_bytes, "fp32_bytes_per_image": batch_bytes // B,
           "uint8_bytes_per_image": H * W * 3, "hbm_peak_tbs": HBM_PEAK / 1e12, "train_iteration_ms_batch64": TRAIN_ITERATION_MS}
    for k, v in blocks.items():
        med = statistics.median(v)
        res[k + "_ms"] = round(med, 4)
        res[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        res[k + "_images_per_s"] = round(B / med * 1e3)
    for kind in ("bgr", "nv12"):
        a, b = res["new_%s_ms" % kind], res["chain_%s_ms" % kind]
        res["chain_over_new_" + kind] = round(b / a, 2)
        res["new_%s_written_tbs" % kind] = round(batch_bytes / (a * 1e-3) / 1e12, 3)
        res["new_%s_written_fraction_of_hbm_peak" % kind] = round(batch_bytes / (a * 1e-3) / HBM_PEAK, 3)
        res["new_%s_algorithmic_bytes" % kind] = staged[kind] + batch_bytes
        res["new_%s_algorithmic_fraction_of_hbm_peak" % kind] = round((staged[kind] + batch_bytes) / (a * 1e-3) / HBM_PEAK, 3)
        res["new_%s_share_of_train_iteration" % kind] = round(a * (64 / B) / TRAIN_ITERATION_MS, 4)
    text = json.dumps(res, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
