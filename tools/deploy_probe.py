#!/usr/bin/env python3
"""The ncnn sample's path on the device (Engine.detect_deploy_frames, include/yfv2.h yfv2_detect_deploy_frames_u8) against the
route it replaces.

Workload: --frames frames (default 256) of 640x480 made on the device from the shipped reference images (upsampled, a little
seeded noise), COCO weights, thresholds 0.3 / 0.25.  After a warm-up:
  detect_deploy    Engine.detect_deploy_frames: resize -> forward -> export maps -> the sample's post-process, device events
                   over --iters
  old route        what a caller had before: resize_frames + forward, the torch export glue of Detector.forward(export_onnx=True)
                   (six ops, a cat and a permute), a copy of the two maps to the host, then the numpy statement of the sample's
                   post-process (tests/deploy_model.py); wall-clock over --host-iters, since the host step needs the maps anyway.
                   old_route_device_ms is its device part alone (events), old_route_host_ms the copy + numpy part.
The two results are compared bit for bit (the glue's softmax is torch's, so scores may differ in the last bits: the comparison is
made on the NEW maps through the same numpy model, and the glue's maps are compared with the new ones in ulps).  Then, unless
--no-trace, the detect_deploy loop alone in a child process under `rocprofv3 --kernel-trace --stats`: the export and post launches'
own times.  Prints one JSON line (and writes it to --out).
usage: python tools/deploy_probe.py [--frames 256] [--iters 20] [--host-iters 1] [--warmup 2] [--out profiles/deploy_probe.json]
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

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]  # data/coco.data:17
H = W = 352
FH, FW = 480, 640
THRESH, NMS = 0.3, 0.25


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def trace_stats(args):
    """the detect_deploy loop alone in a child under rocprofv3 --kernel-trace --stats -> {kernel: (calls, mean ns)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "deploy", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--iters", str(args.iters),
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


def make_frames(n, dev, seed):
    imgs = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "images_u8.npz"))["images"]).to(dev)      # (6, 3, 352, 352) uint8
    up = torch.nn.functional.interpolate(imgs.float(), size=(FH, FW), mode="bilinear", align_corners=False)
    gen = torch.Generator(device=dev).manual_seed(seed)
    frames = []
    for k in range(n):
        noise = torch.randint(-3, 4, (3, FH, FW), generator=gen, device=dev)
        frames.append((up[k % len(up)] + noise).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous())
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    from oracle import yfv2_oracle as oracle
    dev = torch.device("cuda:0")
    B = args.frames
    frames = make_frames(B, dev, args.seed)
    eng = yfv2.Engine(dev, H, W, 80, 3, anchors=ANCHORS, max_batch=B, plan={})
    eng.load_state_dict(oracle.load_weights(os.path.join(REPO, "tests", "golden", "weights_coco.npz")))
    out = eng.new_deploy_buffers(B)

    def run_deploy():
        eng.detect_deploy_frames(frames, THRESH, NMS, out=out, check=False)

    if args.child:                      # what rocprofv3 traces: warm-up + the timed loop of detect_deploy only
        for _ in range(args.warmup):
            run_deploy()
        torch.cuda.synchronize()
        timed(run_deploy, args.iters)
        return

    import deploy_model as dm
    scale = np.float32([[np.float32(FW) / np.float32(W), np.float32(FH) / np.float32(H)]] * B)
    x_u8 = torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)
    logits = [torch.empty(s, device=dev, dtype=torch.float32) for s in eng.logit_shapes(B)]

    def old_device():
        r2, o2, c2, r3, o3, c3 = eng.forward(eng.resize_frames(frames, out=x_u8), out=logits)
        return (torch.cat((r2.sigmoid(), o2.sigmoid(), torch.softmax(c2, 1)), 1).permute(0, 2, 3, 1).contiguous(),
                torch.cat((r3.sigmoid(), o3.sigmoid(), torch.softmax(c3, 1)), 1).permute(0, 2, 3, 1).contiguous())

    host_ms = []

    def old_route():
        m0, m1 = old_device()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = dm.deploy_batch(m0.cpu().numpy(), m1.cpu().numpy(), ANCHORS, H, THRESH, NMS, scale=scale)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        return res

    for _ in range(args.warmup):
        run_deploy()
        old_device()
    torch.cuda.synchronize()
    run_deploy()
    gb, gc = out[0].cpu().numpy(), out[1].cpu().numpy()
    new_maps = eng.export_maps(logits)                         # (logits hold this batch: old_device ran on the same frames)
    wb, wc, _ = dm.deploy_batch(new_maps[0].cpu().numpy(), new_maps[1].cpu().numpy(), ANCHORS, H, THRESH, NMS, scale=scale)
    same = bool(np.array_equal(gc, wc) and np.array_equal(gb, wb))
    ob, oc, _ = old_route()
    glue = old_device()
    ulp = 0
    for a, b in zip(glue, new_maps):
        ai, bi = a.cpu().numpy().view(np.int32).astype(np.int64), b.cpu().numpy().view(np.int32).astype(np.int64)
        ulp = max(ulp, int(np.abs(ai - bi).max()))

    ms_deploy = timed(run_deploy, args.iters)
    ms_old_dev = timed(old_device, args.iters)
    host_ms.clear()
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        old_route()
    ms_old = (time.perf_counter() - t0) * 1e3 / args.host_iters

    res = {"tool": "deploy_probe", "frames": B, "frame": "%dx%d" % (FW, FH), "weights": "coco", "thresh": THRESH, "nms_thresh": NMS,
           "iters": args.iters, "host_iters": args.host_iters, "boxes": int(gc.sum()),
           "detect_deploy_equals_model_on_its_maps": same,
           "old_route_counts_equal": bool(np.array_equal(oc, gc)), "old_route_records_equal": bool(np.array_equal(ob, gb)),
           "torch_glue_maps_max_ulp_from_export_maps": ulp,
           "detect_deploy_ms": round(ms_deploy, 4), "detect_deploy_frames_per_s": round(B / ms_deploy * 1e3, 1),
           "old_route_ms": round(ms_old, 2), "old_route_device_ms": round(ms_old_dev, 4), "old_route_host_ms": round(float(np.mean(host_ms)), 2),
           "old_route_frames_per_s": round(B / ms_old * 1e3, 1), "speedup": round(ms_old / ms_deploy, 1)}
    if not args.no_trace:
        st = trace_stats(args)
        for name in ("export_maps_kernel", "deploy_post_kernel", "resize_frames_u8_kernel"):
            try:
                calls, ns = find(st, name)
                res[name + "_us"], res[name + "_calls"] = round(ns / 1e3, 2), calls
            except KeyError:
                pass
        if "export_maps_kernel_us" in res:      # bytes the export launch must move: every logit read once, every map float written once
            nbytes = B * 2 * 4 * 95 * (22 * 22 + 11 * 11)
            res["export_maps_bytes"] = nbytes
            res["export_maps_hbm_fraction_of_8tbs"] = round(nbytes / (res["export_maps_kernel_us"] * 1e-6) / 8.0e12, 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
