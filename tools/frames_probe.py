#!/usr/bin/env python3
"""Ragged-batch detection (Engine.detect_frames, include/yfv2.h yfv2_detect_frames_u8) against what a caller does without it.

Workload: a seeded batch of --frames frames (default 256) mixing 1920x1080, 1280x720, 640x480 and 352x352 in shuffled order,
generated on the device (nothing is read from disk), random-init weights (yfv2.random_state_dict(0)), test.py's thresholds.
After a warm-up, timed with device events over --iters iterations:
  detect_frames    Engine.detect_frames on the list: ragged resize + detect + frame-coordinate epilogue
  grouped          the workaround: one Engine.resize per frame size (torch.stack of the group first), a copy of every group
                   into one batch, Engine.detect, and the boxes scaled on the host (device -> host copy + numpy); its time is
                   wall-clock with the device synchronised per iteration, since the host step needs the results anyway
                   (grouped_device_ms: its device part alone, by events)
  pre_resized      Engine.detect on a batch that is already (B, 352, 352, 3)
Then, unless --no-trace, the same detect_frames loop in a child process under `rocprofv3 --kernel-trace --stats`: the
per-launch times of resize_frames_u8_kernel and frame_boxes_kernel, and the resize kernel's algorithmic bytes (two staged
source rows per output row + the output rows) as a fraction of the 8 TB/s HBM peak.
Prints one JSON line.   usage: python tools/frames_probe.py [--frames 256] [--iters 20] [--warmup 3]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import yolo_fastestv2_amd as yfv2  # noqa: E402

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]  # data/coco.data:17
SIZES = [(1080, 1920), (720, 1280), (480, 640), (352, 352)]   # (h, w)
HBM_PEAK = 8.0e12
H = W = 352


def make_frames(dev, n, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    order = np.random.default_rng(seed).permutation(np.arange(n) % len(SIZES))
    return [torch.randint(0, 256, SIZES[k] + (3,), generator=gen, device=dev, dtype=torch.uint8) for k in order]


def resize_bytes(frames):
    """algorithmic bytes of resize_frames_u8_kernel: per output row two staged source rows of 3w bytes, plus the row itself"""
    return sum(H * (2 * 3 * int(f.shape[1]) + 3 * W) for f in frames)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def trace_stats(args):
    """the detect_frames loop alone in a child under rocprofv3 --kernel-trace --stats -> {kernel: (calls, mean ns)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "frames", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        out, rows = {}, []
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                rows.append(row)
                out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]))
        if args.keep_stats:
            with open(args.keep_stats, "w", newline="") as f:
                w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
                w.writeheader()
                w.writerows(rows)
        return out


def find(stats, name):
    for k, v in stats.items():
        if name in k:
            return v
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--keep-stats", default=None, help="also write the rocprofv3 kernel stats CSV here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    B = args.frames
    frames = make_frames(dev, B, args.seed)
    eng = yfv2.Engine(dev, H, W, 80, 3, anchors=ANCHORS, max_batch=B, plan={})
    eng.load_state_dict(yfv2.random_state_dict(0))
    out = eng.new_det_buffers(B)
    conf, iou = 0.3, 0.4

    def run_frames():
        eng.detect_frames(frames, conf, iou, out=out, check=False)

    if args.child:                      # what rocprofv3 traces: warm-up + the timed loop of detect_frames only
        for _ in range(args.warmup):
            run_frames()
        torch.cuda.synchronize()
        timed(run_frames, args.iters)
        return

    groups = {}
    for i, f in enumerate(frames):
        groups.setdefault(tuple(f.shape[:2]), []).append(i)
    groups = [(k, torch.tensor(v, device=dev), v) for k, v in groups.items()]
    batch = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    out_g = eng.new_det_buffers(B)
    sx = np.array([f.shape[1] / W for f in frames], np.float64)
    sy = np.array([f.shape[0] / H for f in frames], np.float64)

    def run_grouped_device():
        for _, ti, li in groups:
            batch.index_copy_(0, ti, eng.resize(torch.stack([frames[i] for i in li])))
        return eng.detect(batch, conf, iou, out=out_g, check=False)

    def run_grouped():
        dets, _, cnt = run_grouped_device()
        d, c = dets.cpu().numpy(), cnt.cpu().numpy()          # waits for the device
        for b in range(B):
            r = d[b, :c[b], :4].astype(np.float64)
            r[:, 0::2] *= sx[b]
            r[:, 1::2] *= sy[b]
            d[b, :c[b], :4] = r.astype(np.float32)
        return d

    pre = eng.resize_frames(frames)

    def run_pre():
        eng.detect(pre, conf, iou, out=out, check=False)

    for _ in range(args.warmup):
        run_frames(); run_grouped(); run_pre()
    torch.cuda.synchronize()
    # the two paths agree (the grouped host scaling is the test.py formula, the device epilogue restates it)
    run_frames()
    d_g = run_grouped()
    n_det = int(out[2].sum())
    same = all(np.array_equal(out[0][b, :int(out[2][b])].cpu().numpy().view(np.uint32), d_g[b, :int(out[2][b])].view(np.uint32))
               for b in range(B))

    ms_frames = timed(run_frames, args.iters)
    ms_pre = timed(run_pre, args.iters)
    ms_grouped_dev = timed(run_grouped_device, args.iters)
    t0 = time.perf_counter()
    for _ in range(args.iters):
        run_grouped()
    ms_grouped = (time.perf_counter() - t0) * 1e3 / args.iters

    res = {"tool": "frames_probe", "frames": B, "mix": ["%dx%d" % (w, h) for h, w in SIZES], "iters": args.iters,
           "detections": n_det, "detect_frames_equals_grouped": bool(same),
           "detect_frames_ms": round(ms_frames, 4), "detect_frames_fps": round(B / ms_frames * 1e3),
           "grouped_ms": round(ms_grouped, 4), "grouped_fps": round(B / ms_grouped * 1e3),
           "grouped_device_ms": round(ms_grouped_dev, 4), "grouped_device_fps": round(B / ms_grouped_dev * 1e3),
           "pre_resized_detect_ms": round(ms_pre, 4), "pre_resized_detect_fps": round(B / ms_pre * 1e3),
           "resize_bytes": resize_bytes(frames)}
    if not args.no_trace:
        st = trace_stats(args)
        calls, ns = find(st, "resize_frames_u8_kernel")
        res["resize_frames_kernel_us"] = round(ns / 1e3, 2)
        res["resize_frames_kernel_calls"] = calls
        res["resize_frames_hbm_tbs"] = round(res["resize_bytes"] / ns * 1e-3, 3)
        res["resize_frames_hbm_fraction_of_8tbs"] = round(res["resize_bytes"] / (ns * 1e-9) / HBM_PEAK, 3)
        calls, ns = find(st, "frame_boxes_kernel")
        res["frame_boxes_kernel_us"] = round(ns / 1e3, 2)
        res["frame_boxes_kernel_calls"] = calls
    print(json.dumps(res))


if __name__ == "__main__":
    main()
