#!/usr/bin/env python3
"""Decoder-format frames (Engine.resize_frames_yuv / detect_frames_yuv, include/yfv2.h yfv2_*_yuv) against the B, G, R entry points.

Workload: frames_probe.py's - a seeded batch of --frames frames (default 256) mixing 1920x1080, 1280x720, 640x480 and 352x352 in
shuffled order - as random NV12 planes generated on the device, and the same frames converted to B, G, R by the integer rule of
include/yfv2.h (torch integer ops here: a tool's reference, not a product path).  Random-init weights, test.py's thresholds.
In ONE process, after a warm-up, --rounds rounds that alternate the two sides, each timed with device events over --iters calls:
  (a) resize_bgr        Engine.resize_frames on the converted frames       - existing code, this process's own baseline
  (b) resize_yuv        Engine.resize_frames_yuv on the NV12 planes        - the code under test; its output must equal (a)'s
  (c) detect_bgr / detect_yuv   Engine.detect_frames against Engine.detect_frames_yuv, end to end
Per side: median, min and max over the rounds (the spread the comparison has to beat).  Also the bytes each resize launch reads per
frame (the staged source rows; (b) counts a chroma row once when both blended rows share it) and writes.  Then, unless --no-trace,
the two resize loops in a child process under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
Prints one JSON line.   usage: python tools/yuv_probe.py [--frames 256] [--iters 20] [--rounds 7] [--warmup 3]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import yolo_fastestv2_amd as yfv2  # noqa: E402

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]  # data/coco.data:17
SIZES = [(1080, 1920), (720, 1280), (480, 640), (352, 352)]   # (h, w)
HBM_PEAK = 8.0e12
H = W = 352
BT601 = (16, 1220542, 1673527, -852492, -409993, 2116026)     # include/yfv2.h YFV2_BT601_LIMITED


def make_planes(dev, n, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    order = np.random.default_rng(seed).permutation(np.arange(n) % len(SIZES))
    return [(torch.randint(0, 256, SIZES[k], generator=gen, device=dev, dtype=torch.uint8),
             torch.randint(0, 256, (SIZES[k][0] // 2, SIZES[k][1]), generator=gen, device=dev, dtype=torch.uint8)) for k in order]


def to_bgr(y, uv):
    """the rule of include/yfv2.h for an even-sized NV12 frame, in torch int32"""
    off, cy, cvr, cvg, cug, cub = BT601
    h, w = y.shape
    c = uv.view(h // 2, w // 2, 2).to(torch.int32).repeat_interleave(2, 0).repeat_interleave(2, 1) - 128
    u, v = c[..., 0], c[..., 1]
    yy = (y.to(torch.int32) - off).clamp_(min=0) * cy + (1 << 19)
    return torch.stack([((yy + cub * u) >> 20), ((yy + cvg * v + cug * u) >> 20), ((yy + cvr * v) >> 20)], 2).clamp_(0, 255).to(torch.uint8)


def rows_of(h):
    """the two source rows each of the H output rows blends (yfv2_axis_coef, rows)"""
    scale = 1.0 / (H / h)
    f = ((np.arange(H, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return np.clip(s, 0, h - 1), np.clip(s + 1, 0, h - 1)


def bytes_read(shape, yuv):
    h, w = shape
    if not yuv:
        return H * 2 * 3 * w
    s0, s1 = rows_of(h)
    chroma_rows = int(np.sum(1 + ((s0 >> 1) != (s1 >> 1))))
    return H * 2 * w + chroma_rows * w


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def trace_stats(args, script=os.path.abspath(__file__)):
    """the kernels' (calls, average ns) of `script --child` (this tool's, or yuv16_probe.py's) under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "yuv", "--",
               sys.executable, script, "--child", "--frames", str(args.frames), "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        with open(files[0]) as f:
            return {row["Name"]: (int(row["Calls"]), float(row["AverageNs"])) for row in csv.DictReader(f)}


def find(stats, name):
    for k, v in stats.items():
        if name in k:
            return v
    raise KeyError(name)


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    B = args.frames
    planes = make_planes(dev, B, args.seed)
    frames_yuv = [yfv2.YuvFrame(p, "nv12", "bt601") for p in planes]
    frames_bgr = [to_bgr(*p) for p in planes]
    eng = yfv2.Engine(dev, H, W, 80, 3, anchors=ANCHORS, max_batch=B, plan={})
    eng.load_state_dict(yfv2.random_state_dict(0))
    out_a = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(out_a)
    det_a, det_b = eng.new_det_buffers(B), eng.new_det_buffers(B)
    for t in det_a + det_b:             # rows beyond count are not written: equal from the start
        t.zero_()
    conf, iou = 0.3, 0.4
    sides = {
        "resize_bgr": lambda: eng.resize_frames(frames_bgr, out=out_a),
        "resize_yuv": lambda: eng.resize_frames_yuv(frames_yuv, out=out_b),
        "detect_bgr": lambda: eng.detect_frames(frames_bgr, conf, iou, out=det_a, check=False),
        "detect_yuv": lambda: eng.detect_frames_yuv(frames_yuv, conf, iou, out=det_b, check=False),
    }
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    if args.child:                      # what rocprofv3 traces: the two resize loops
        timed(sides["resize_bgr"], args.iters)
        timed(sides["resize_yuv"], args.iters)
        return

    same_resize = bool(torch.equal(out_a, out_b))
    same_detect = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(det_a, det_b))
    ms = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():     # alternating: every round times each side once
            ms[k].append(timed(fn, args.iters))
    props = torch.cuda.get_device_properties(dev)
    read_a = sum(bytes_read(tuple(p[0].shape), False) for p in planes)
    read_b = sum(bytes_read(tuple(p[0].shape), True) for p in planes)
    res = {"tool": "yuv_probe", "frames": B, "mix": ["%dx%d" % (w, h) for h, w in SIZES], "format": "nv12", "iters": args.iters, "rounds": args.rounds,
           "box": {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "compute_units": props.multi_processor_count,
                   "torch": torch.__version__, "hip": torch.version.hip},
           "resize_yuv_equals_resize_bgr": same_resize, "detect_yuv_equals_detect_bgr": same_detect, "detections": int(det_a[2].sum()),
           "ms": {k: spread(v) for k, v in ms.items()},
           "detect_bgr_fps": round(B / statistics.median(ms["detect_bgr"]) * 1e3), "detect_yuv_fps": round(B / statistics.median(ms["detect_yuv"]) * 1e3),
           "resize_yuv_over_resize_bgr": round(statistics.median(ms["resize_yuv"]) / statistics.median(ms["resize_bgr"]), 4),
           "bytes_read_per_frame": {"resize_bgr": round(read_a / B), "resize_yuv": round(read_b / B), "ratio": round(read_b / read_a, 4)},
           "bytes_written_per_frame": 3 * H * W}
    if not args.no_trace:
        st = trace_stats(args)
        for name, rd in (("resize_frames_u8_kernel", read_a), ("resize_frames_yuv_kernel", read_b)):
            calls, ns = find(st, name)
            res[name] = {"us": round(ns / 1e3, 2), "calls": calls, "hbm_tbs": round((rd + B * 3 * H * W) / ns * 1e-3, 3),
                         "hbm_fraction_of_8tbs": round((rd + B * 3 * H * W) / (ns * 1e-9) / HBM_PEAK, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
