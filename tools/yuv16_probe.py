#!/usr/bin/env python3
"""10-bit decoder frames (P010 through Engine.resize_frames_yuv / detect_frames_yuv) against NV12 frames of the same
pictures - the existing 8-bit path, this process's own yardstick.

Workload: yuv_probe.py's - a seeded batch of --frames frames (default 256) mixing 1920x1080, 1280x720, 640x480 and 352x352 in
shuffled order - as random NV12 planes generated on the device, and the same pictures as P010 planes (every sample times 4, in the
high 10 bits of an int16 word).  Random-init weights, test.py's thresholds.  The P010 resize is checked once against
Engine.resize_frames of the frames converted by the 10-bit rule of include/yfv2.h (torch integer ops here: a tool's reference).
In ONE process, after a warm-up, --rounds rounds that alternate the four sides, each timed with device events over --iters calls:
  detect_p010 / detect_nv12     Engine.detect_frames_yuv end to end
  resize_p010 / resize_nv12     Engine.resize_frames_yuv, the one launch that differs
Per side: median, min and max over the rounds (the spread a comparison has to beat).  Also the bytes each resize launch reads per
frame (the staged source rows; a chroma row counts once when both blended rows share it) and writes.  Then, unless --no-trace, the
two resize loops in a child process under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
Prints one JSON line.   usage: python tools/yuv16_probe.py [--frames 256] [--iters 20] [--rounds 7] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yolo_fastestv2_amd as yfv2  # noqa: E402
from yuv_probe import ANCHORS, H, HBM_PEAK, SIZES, W, bytes_read, find, make_planes, spread, timed, trace_stats  # noqa: E402

BT601_10 = (64, 305236, 418389, -213115, -102698, 528805)     # include/yfv2.h YFV2_BT601_LIMITED, the 10-bit table


def to_p010(plane):
    """an 8-bit plane as P010 words: the 10-bit value 4 * sample in the high 10 bits (int16 holds the same bits)"""
    x = plane.to(torch.int32) << 8
    return torch.where(x >= 32768, x - 65536, x).to(torch.int16)


def to_bgr(y, uv):
    """the 10-bit rule of include/yfv2.h for an even-sized P010 frame, in torch int32"""
    off, cy, cvr, cvg, cug, cub = BT601_10
    h, w = y.shape
    val = lambda t: (t.to(torch.int32) & 0xffff) >> 6
    c = val(uv).view(h // 2, w // 2, 2).repeat_interleave(2, 0).repeat_interleave(2, 1) - 512
    u, v = c[..., 0], c[..., 1]
    yy = (val(y) - off).clamp_(min=0) * cy + (1 << 19)
    return torch.stack([((yy + cub * u) >> 20), ((yy + cvg * v + cug * u) >> 20), ((yy + cvr * v) >> 20)], 2).clamp_(0, 255).to(torch.uint8)


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
    planes16 = [tuple(to_p010(p) for p in ps) for ps in planes]
    frames_nv12 = [yfv2.YuvFrame(p, "nv12", "bt601") for p in planes]
    frames_p010 = [yfv2.YuvFrame(p, "p010", "bt601") for p in planes16]
    eng = yfv2.Engine(dev, H, W, 80, 3, anchors=ANCHORS, max_batch=B, plan={})
    eng.load_state_dict(yfv2.random_state_dict(0))
    out_8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    out_16 = torch.empty_like(out_8)
    det_8, det_16 = eng.new_det_buffers(B), eng.new_det_buffers(B)
    for t in det_8 + det_16:
        t.zero_()
    conf, iou = 0.3, 0.4
    sides = {
        "detect_p010": lambda: eng.detect_frames_yuv(frames_p010, conf, iou, out=det_16, check=False),
        "detect_nv12": lambda: eng.detect_frames_yuv(frames_nv12, conf, iou, out=det_8, check=False),
        "resize_p010": lambda: eng.resize_frames_yuv(frames_p010, out=out_16),
        "resize_nv12": lambda: eng.resize_frames_yuv(frames_nv12, out=out_8),
    }
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    if args.child:                      # what rocprofv3 traces: the two resize loops
        timed(sides["resize_nv12"], args.iters)
        timed(sides["resize_p010"], args.iters)
        return

    same = True                         # the P010 resize against the B, G, R resize of the converted frames, 32 frames at a time
    for b0 in range(0, B, 32):
        ref = eng.resize_frames([to_bgr(*p) for p in planes16[b0:b0 + 32]])
        same = same and bool(torch.equal(ref, out_16[b0:b0 + ref.shape[0]]))
    apart = int((out_16.to(torch.int16) - out_8.to(torch.int16)).abs().max())       # the two rules on one picture: about a unit
    ms = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():     # alternating: every round times each side once
            ms[k].append(timed(fn, args.iters))
    props = torch.cuda.get_device_properties(dev)
    read_8 = sum(bytes_read(tuple(p[0].shape), True) for p in planes)
    read_16 = 2 * read_8                # the same rows, two bytes a sample
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"tool": "yuv16_probe", "frames": B, "mix": ["%dx%d" % (w, h) for h, w in SIZES], "formats": ["p010", "nv12"], "iters": args.iters, "rounds": args.rounds,
           "box": {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "compute_units": props.multi_processor_count,
                   "torch": torch.__version__, "hip": torch.version.hip},
           "resize_p010_equals_resize_bgr_of_converted": same, "max_abs_p010_minus_nv12": apart,
           "detections": {"p010": int(det_16[2].sum()), "nv12": int(det_8[2].sum())},
           "ms": {k: spread(v) for k, v in ms.items()},
           "detect_p010_fps": round(B / med["detect_p010"] * 1e3), "detect_nv12_fps": round(B / med["detect_nv12"] * 1e3),
           "resize_p010_over_resize_nv12": round(med["resize_p010"] / med["resize_nv12"], 4),
           "detect_p010_over_detect_nv12": round(med["detect_p010"] / med["detect_nv12"], 4),
           "bytes_read_per_frame": {"resize_p010": round(read_16 / B), "resize_nv12": round(read_8 / B)},
           "bytes_written_per_frame": 3 * H * W}
    if not args.no_trace:
        st = trace_stats(args, os.path.abspath(__file__))
        yuv_kernels = {k: v for k, v in st.items() if "resize_frames_yuv_kernel" in k}
        for name, want16, rd in (("resize_nv12_kernel", False, read_8), ("resize_p010_kernel", True, read_16)):
            calls, ns = find({k: v for k, v in yuv_kernels.items() if ("Samples16" in k) == want16}, "resize_frames_yuv_kernel")
            res[name] = {"us": round(ns / 1e3, 2), "calls": calls, "hbm_tbs": round((rd + B * 3 * H * W) / ns * 1e-3, 3),
                         "hbm_fraction_of_8tbs": round((rd + B * 3 * H * W) / (ns * 1e-9) / HBM_PEAK, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
