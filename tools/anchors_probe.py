#!/usr/bin/env python3
"""Anchor k-means (Engine.anchor_kmeans, include/yfv2.h yfv2_anchor_kmeans) on a label set of COCO's order of magnitude.

Workload: --points (default 1 000 000) seeded synthetic label sizes (tests/anchors_model.make_x), k = 6 and k = 10, initial
centroids drawn as genanchors.main draws them, the loop cut at --passes passes (a multiple of the group size of 8, so every
launch of the run does a whole pass; a run that converges earlier is reported as such).  Per k:
  call_ms            wall clock of the whole call (median of --repeats after --warmup calls), host waits included
  assign_us/final_us the two launches' own durations: mean of the dispatch timestamps of a child process under
                     `rocprofv3 --kernel-trace --stats` (unless --no-trace)
  hbm_fraction       20 B per point per pass (16 read, 4 written) / assign_us against the 8 TB/s HBM peak
  numpy_pass_ms      the vectorised numpy model of the same arithmetic (tests/anchors_model.kmeans) on this box's host
With --reference-dir DIR (a checkout of the reference; needs no GPU) it instead times ONE pass of the reference's own
interpreted distance loop (genanchors.py:79-81) on 20 011 points and EXTRAPOLATES it linearly to --points.
Prints one JSON line.   usage: python tools/anchors_probe.py [--points 1000000] [--passes 40] [--repeats 5] [--warmup 2]
"""
import argparse
import csv
import glob
import importlib.util
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import anchors_model as am  # noqa: E402

HBM_PEAK = 8.0e12
KS = (6, 10)


def workload(n, k, seed):
    X = am.make_x(seed, n)
    random.seed(seed)
    return X, X[[random.randrange(n) for _ in range(k)]].copy()


def reference_pass(args):
    np.float = float
    spec = importlib.util.spec_from_file_location("ref_genanchors", os.path.join(args.reference_dir, "genanchors.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    res = {"tool": "anchors_probe", "mode": "reference", "timed_points": 20011, "extrapolated_to_points": args.points}
    for k in KS:
        X, C = workload(20011, k, args.seed)
        t0 = time.perf_counter()
        D = np.array([1 - ref.IOU(X[i], C) for i in range(len(X))])
        dt = time.perf_counter() - t0
        assert D.shape == (20011, k)
        res["k%d" % k] = {"reference_pass_s_at_20011": round(dt, 3), "reference_pass_s_EXTRAPOLATED": round(dt * args.points / 20011, 1)}
    print(json.dumps(res))


def trace_stats(args, k):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "anchors", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(k), "--points", str(args.points), "--passes", str(args.passes),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        with open(files[0]) as f:
            return {row["Name"]: (int(row["Calls"]), float(row["AverageNs"])) for row in csv.DictReader(f)}


def find(stats, name):
    for key, v in stats.items():
        if name in key:
            return v
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--passes", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--reference-dir", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reference_dir:
        return reference_pass(args)

    import torch
    import yolo_fastestv2_amd as yfv2
    dev = torch.device("cuda:0")
    eng = yfv2.Engine(dev, 352, 352, 80, 3, plan={})
    res = {"tool": "anchors_probe", "points": args.points, "passes_cap": args.passes, "repeats": args.repeats, "warmup": args.warmup}
    for k in ([args.child] if args.child else KS):
        X, C0 = workload(args.points, k, args.seed)
        x_t, c_t = torch.from_numpy(X).to(dev), torch.from_numpy(C0).to(dev)
        times, info = [], None
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cent, assign, avg, info = eng.anchor_kmeans(x_t, c_t, max_iter=args.passes)   # waits for the stream itself
            if i >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        if args.child:
            return
        call_ms = statistics.median(times)
        t0 = time.perf_counter()
        m = am.kmeans(X, C0, max_iter=3)
        numpy_pass_ms = (time.perf_counter() - t0) * 1e3 / m["iterations"]
        r = {"iterations": info["iterations"], "converged": info["converged"], "avg_iou": float(avg.cpu()),
             "call_ms": round(call_ms, 3), "call_ms_min": round(min(times), 3), "call_ms_max": round(max(times), 3),
             "call_us_per_pass": round(call_ms * 1e3 / info["iterations"], 2), "numpy_pass_ms": round(numpy_pass_ms, 1)}
        if not args.no_trace:
            st = trace_stats(args, k)
            calls, ns = find(st, "km_assign_kernel")
            r.update(assign_us=round(ns / 1e3, 2), assign_calls=calls, assign_hbm_tbs=round(20.0 * args.points / ns * 1e-3, 3),
                     assign_hbm_fraction_of_8tbs=round(20.0 * args.points / (ns * 1e-9) / HBM_PEAK, 3))
            calls, ns = find(st, "km_final_kernel")
            r.update(final_us=round(ns / 1e3, 2), final_calls=calls)
            r["launch_us_per_pass"] = round(r["assign_us"] + r["final_us"], 2)
        res["k%d" % k] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
