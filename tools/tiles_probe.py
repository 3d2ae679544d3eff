#!/usr/bin/env python3
"""Tiled detection (Engine.detect_tiled, include/yfv2.h yfv2_detect_tiled_u8) against the composition it replaces.

Workload: --frames frames (default 8) of 1920x1080 generated on the device (nothing is read from disk), tile 352, overlap 64
(28 tiles per frame), random-init weights (yfv2.random_state_dict(0)): 300 detections per tile, the merge's worst case.
After a warm-up:
  detect_tiled     Engine.detect_tiled: crops -> resize -> detect -> tile-to-frame -> merge, device events over --iters
  detect_frames    its first half alone: Engine.detect_frames on the crop views (device events)
  composition      what a caller does without the entry point: detect_frames on the crop views, a copy to the host, then the
                   numpy statement of the merge rule (tests/tiles_ref.py merge_model); wall-clock over --host-iters, since
                   the host step needs the results anyway.  composition_host_ms is the copy + numpy part alone.
The two results are compared bit for bit.  Then, unless --no-trace, the detect_tiled loop alone in a child process under
`rocprofv3 --kernel-trace --stats`: the per-launch times of tile_rank_kernel and tile_merge_kernel, and the bytes the rank
launch moves (24 B read per tile row, 32 B written per candidate) against the 8 TB/s HBM peak.
Prints one JSON line.   usage: python tools/tiles_probe.py [--frames 8] [--iters 20] [--host-iters 2] [--warmup 2]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import yolo_fastestv2_amd as yfv2  # noqa: E402
from yolo_fastestv2_amd import tiling  # noqa: E402

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]  # data/coco.data:17
HBM_PEAK = 8.0e12
H = W = 352
FH, FW = 1080, 1920


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def trace_stats(args):
    """the detect_tiled loop alone in a child under rocprofv3 --kernel-trace --stats -> {kernel: (calls, mean ns)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tiles", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--seed", str(args.seed), "--metric", args.metric, "--max-out", str(args.max_out)]
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
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--metric", default="iou")
    ap.add_argument("--max-out", type=int, default=300)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--keep-stats", default=None, help="also write the rocprofv3 kernel stats CSV here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    F = args.frames
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    frames = [torch.randint(0, 256, (FH, FW, 3), generator=gen, device=dev, dtype=torch.uint8) for _ in range(F)]
    tiles = [t for f in range(F) for t in tiling.plan_tiles(FH, FW, frame=f)]
    T = len(tiles)
    eng = yfv2.Engine(dev, H, W, 80, 3, anchors=ANCHORS, max_batch=T, plan={})
    eng.load_state_dict(yfv2.random_state_dict(0))
    conf, iou = 0.3, 0.4
    code = tiling.metric_code(args.metric)
    out = eng.new_tiled_buffers(F, args.max_out)

    def run_tiled():
        eng.detect_tiled(frames, tiles=tiles, conf_thres=conf, iou_thres=iou, metric=args.metric, max_out=args.max_out, out=out, check=False)

    if args.child:                      # what rocprofv3 traces: warm-up + the timed loop of detect_tiled only
        for _ in range(args.warmup):
            run_tiled()
        torch.cuda.synchronize()
        timed(run_tiled, args.iters)
        return

    from tiles_ref import merge_model
    crops = tiling.crop_views(frames, tiles)
    out_f = eng.new_det_buffers(T)

    def run_frames():
        return eng.detect_frames(crops, conf, iou, out=out_f, check=False)

    host_ms = []

    def run_composition():
        dets, _, cnt = run_frames()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d, c = dets.cpu().numpy(), cnt.cpu().numpy()
        res = merge_model(d, c, tiles, F, iou, code, args.max_out)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        return res, c

    for _ in range(args.warmup):
        run_tiled()
    torch.cuda.synchronize()
    (wd, ws, wc), tile_count = run_composition()
    run_tiled()
    gd, gs, gc = (t.cpu().numpy() for t in out)
    same = bool(np.array_equal(gc, wc)) and all(
        np.array_equal(gs[f, :wc[f]], ws[f, :wc[f]]) and np.array_equal(gd[f, :wc[f]].view(np.uint32), wd[f, :wc[f]].view(np.uint32)) for f in range(F))

    ms_tiled = timed(run_tiled, args.iters)
    ms_frames = timed(run_frames, args.iters)
    host_ms.clear()
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        run_composition()
    ms_comp = (time.perf_counter() - t0) * 1e3 / args.host_iters

    cand = int(tile_count.sum())
    res = {"tool": "tiles_probe", "frames": F, "frame": "%dx%d" % (FW, FH), "tile": 352, "overlap": 64, "tiles": T, "metric": args.metric,
           "max_out": args.max_out, "iters": args.iters, "host_iters": args.host_iters, "candidates": cand, "kept": int(wc.sum()),
           "detect_tiled_equals_composition": same,
           "detect_tiled_ms": round(ms_tiled, 4), "detect_tiled_frames_per_s": round(F / ms_tiled * 1e3, 1),
           "detect_frames_on_crops_ms": round(ms_frames, 4), "merge_ms_by_difference": round(ms_tiled - ms_frames, 4),
           "composition_ms": round(ms_comp, 2), "composition_host_ms": round(float(np.mean(host_ms)), 2),
           "composition_frames_per_s": round(F / ms_comp * 1e3, 2), "speedup": round(ms_comp / ms_tiled, 1),
           "rank_bytes": T * 300 * 24 + cand * 32}
    if not args.no_trace:
        st = trace_stats(args)
        calls, ns = find(st, "tile_rank_kernel")
        res["tile_rank_kernel_us"], res["tile_rank_kernel_calls"] = round(ns / 1e3, 2), calls
        res["tile_rank_hbm_fraction_of_8tbs"] = round(res["rank_bytes"] / (ns * 1e-9) / HBM_PEAK, 4)
        calls, ns = find(st, "tile_merge_kernel")
        res["tile_merge_kernel_us"], res["tile_merge_kernel_calls"] = round(ns / 1e3, 2), calls
        res["tile_merge_ns_per_candidate_per_frame"] = round(ns / (cand / F), 2)
        for name in ("resize_frames_u8_kernel", "frame_boxes_kernel", "nms_kernel"):
            try:
                calls, ns = find(st, name)
                res[name + "_us"] = round(ns / 1e3, 2)
            except KeyError:
                pass
    print(json.dumps(res))


if __name__ == "__main__":
    main()
