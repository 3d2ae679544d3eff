#!/usr/bin/env python3
"""Average precision on the device (Engine.ap_per_class, include/yfv2.h yfv2_ap_per_class) on a validation set of COCO's size.

Workload: --rows (default 1 500 000: 5 000 images x 300 detections) seeded synthetic detections over 80 classes, 36 000 targets,
once with uniform classes ("uniform") and once with 30 % of the rows in one class ("skew": the one-workgroup-per-class walk's
worst case).  Per case:
  call_ms      wall clock of the whole call (median of --repeats after --warmup calls), the final host wait included
  host_ms      the numpy ap_per_class (yolo_fastestv2_amd.ap_per_class) on the same arrays on this box's host, one call
  kernels      per launch name: calls and mean duration (us) from the dispatch timestamps of a child process that runs the same
               loop under `rocprofv3 --kernel-trace --stats` (unless --no-trace)
  sort_pass_hbm_fraction   bytes one sort pass moves (hist: 4 B read, scatter: 8 B read + 8 B written per row) over the summed
               hist + scan + scatter durations, against the 8 TB/s HBM peak
Prints one JSON line.   usage: python tools/ap_probe.py [--rows 1500000] [--repeats 5] [--warmup 2]
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
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12
CASES = ("uniform", "skew")
KERNELS = ("ap_targets_kernel", "ap_prep_kernel", "ap_hist_kernel", "ap_scan_kernel", "ap_scatter_kernel", "ap_curve_kernel")


def workload(n, case, seed):
    rng = np.random.default_rng(seed)
    conf = rng.random(n).astype(np.float32)
    cls = rng.integers(0, 80, n).astype(np.float32)
    if case == "skew":
        cls[rng.random(n) < 0.3] = 0.0
    tp = (rng.random(n) < 0.4).astype(np.int32)
    labels = rng.integers(0, 80, 36000).astype(np.float32)
    return tp, conf, cls, labels


def trace_stats(args, case):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ap", "--",
               sys.executable, os.path.abspath(__file__), "--child", case, "--rows", str(args.rows),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        with open(files[0]) as f:
            return {row["Name"]: (int(row["Calls"]), float(row["AverageNs"])) for row in csv.DictReader(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1500000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()

    import torch
    import yolo_fastestv2_amd as yfv2
    dev = torch.device("cuda:0")
    eng = yfv2.Engine(dev, 64, 64, 2, 3, plan={})
    res = {"tool": "ap_probe", "rows": args.rows, "classes": 80, "targets": 36000, "repeats": args.repeats, "warmup": args.warmup}
    for case in ([args.child] if args.child else CASES):
        tp, conf, cls, labels = workload(args.rows, case, args.seed)
        dv = [torch.from_numpy(a).to(dev) for a in (tp, conf, cls, labels)]
        times, out = [], None
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.ap_per_class(*dv)              # waits for the stream itself
            if i >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        if args.child:
            return
        t0 = time.perf_counter()
        host = yfv2.ap_per_class(tp.astype(np.float64), conf, cls, labels.tolist())
        host_ms = (time.perf_counter() - t0) * 1e3
        r = {"largest_class_rows": int(out["n_pred"].max()), "mean_ap": out["means"][2], "host_mean_ap": float(host[2]),
             "call_ms": round(statistics.median(times), 3), "call_ms_min": round(min(times), 3), "call_ms_max": round(max(times), 3),
             "host_ms": round(host_ms, 1)}
        if not args.no_trace:
            st = trace_stats(args, case)
            ker = {}
            for name in KERNELS:
                hit = [v for k, v in st.items() if name in k]
                if hit:
                    ker[name] = {"calls": hit[0][0], "mean_us": round(hit[0][1] / 1e3, 2)}
            r["kernels"] = ker
            if all(k in ker for k in ("ap_hist_kernel", "ap_scan_kernel", "ap_scatter_kernel")):
                pass_us = ker["ap_hist_kernel"]["mean_us"] + ker["ap_scan_kernel"]["mean_us"] + ker["ap_scatter_kernel"]["mean_us"]
                r["sort_pass_us"] = round(pass_us, 2)
                r["sort_pass_hbm_fraction"] = round(20.0 * args.rows / (pass_us * 1e-6) / HBM_PEAK, 4)
                per_call = sum(v["mean_us"] * v["calls"] for v in ker.values()) / (args.warmup + args.repeats)
                r["kernels_us_per_call"] = round(per_call, 1)
        res[case] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
