#!/usr/bin/env python3
"""The 8-bit YUV samplings beyond 4:2:0 (I422, I440, I444, YUYV, UYVY, GREY through Engine.resize_frames_yuv / detect_frames_yuv;
DESIGN.md 4.24) against NV12 frames - the shipped path, this process's own yardstick - and against Engine.resize_frames on the
converted B, G, R frames.

Workload: yuv_probe.py's - a seeded batch of --frames frames (default 256) mixing 1920x1080, 1280x720, 640x480 and 352x352 in
shuffled order - as random planes of each format generated on the device.  Random-init weights, test.py's thresholds.  Each
format's resize is checked once against Engine.resize_frames of the frames converted by the rule of include/yfv2.h (torch integer
ops here: a tool's reference); the NV12 frames of the mixed batch against the all-NV12 call.
In ONE process, after a warm-up, --rounds rounds that alternate all sides, each timed with device events over --iters calls:
  resize_<fmt> / detect_<fmt>     the seven formats (nv12 is the all-4:2:0 launch, every other the general launch)
  resize_mixed / detect_mixed     one batch holding all nine 8-bit formats in turn (the general launch)
  resize_bgr                      Engine.resize_frames on the converted I444 frames
Per side: median, min and max over the rounds (the spread a comparison has to beat), and the bytes the resize launch stages per
frame.  Then, unless --no-trace, the resize loops in a child process under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
--ab OTHER.so: the one hard requirement - an all-NV12 call is the launch it was.  Alternates --sessions fresh processes of the
in-tree library and of OTHER.so (a build of the parent commit, through YFV2_LIB), each timing resize_nv12 / detect_nv12 as above, and
reports every session's median, each build's spread against itself and whether the in-tree median lies inside the other's spread.
Prints one JSON line.   usage: python tools/yuv_any_probe.py [--frames 256] [--iters 20] [--rounds 7] [--warmup 3] [--ab libyfv2_parent.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yolo_fastestv2_amd as yfv2  # noqa: E402
from yuv_probe import ANCHORS, H, SIZES, W, rows_of, spread, timed, trace_stats  # noqa: E402

BT601 = (16, 1220542, 1673527, -852492, -409993, 2116026)     # include/yfv2.h YFV2_BT601_LIMITED
FORMATS = ("nv12", "nv21", "i420", "i422", "i440", "i444", "yuyv", "uyvy", "grey")
TIMED = ("nv12", "i422", "i440", "i444", "yuyv", "uyvy", "grey")
SHIFTS = {"nv12": (1, 1), "nv21": (1, 1), "i420": (1, 1), "i422": (1, 0), "i440": (0, 1), "i444": (0, 0), "yuyv": (1, 0), "uyvy": (1, 0), "grey": (0, 0)}


def make_planes(dev, n, seed, fmt):
    """random planes of `fmt` for yuv_probe's mix and order (even sizes throughout)"""
    gen = torch.Generator(device=dev).manual_seed(seed + 1000 * FORMATS.index(fmt))
    order = np.random.default_rng(seed).permutation(np.arange(n) % len(SIZES))
    rnd = lambda r, c: torch.randint(0, 256, (r, c), generator=gen, device=dev, dtype=torch.uint8)
    sx, sy = SHIFTS[fmt]
    out = []
    for k in order:
        h, w = SIZES[k]
        if fmt == "grey":
            out.append((rnd(h, w),))
        elif fmt in ("yuyv", "uyvy"):
            out.append((rnd(h, 2 * w),))
        elif fmt in ("nv12", "nv21"):
            out.append((rnd(h, w), rnd(h >> 1, w)))
        else:
            out.append((rnd(h, w), rnd(h >> sy, w >> sx), rnd(h >> sy, w >> sx)))
    return out


def to_bgr(planes, fmt):
    """the 8-bit rule of include/yfv2.h for an even-sized frame of `fmt`, in torch int32"""
    off, cy, cvr, cvg, cug, cub = BT601
    sx, sy = SHIFTS[fmt]
    if fmt in ("yuyv", "uyvy"):
        p = planes[0].to(torch.int32)
        yo, uo = (0, 1) if fmt == "yuyv" else (1, 0)
        y, u, v = p[:, yo::2], p[:, uo::4], p[:, uo + 2::4]
    elif fmt == "grey":
        y = planes[0].to(torch.int32)
        u = v = torch.full_like(y, 128)
    elif fmt in ("nv12", "nv21"):
        y, c = planes[0].to(torch.int32), planes[1].to(torch.int32)
        u, v = (c[:, 0::2], c[:, 1::2]) if fmt == "nv12" else (c[:, 1::2], c[:, 0::2])
    else:
        y, u, v = (p.to(torch.int32) for p in planes)
    if fmt != "grey":
        if sy:
            u, v = u.repeat_interleave(2, 0), v.repeat_interleave(2, 0)
        if sx:
            u, v = u.repeat_interleave(2, 1), v.repeat_interleave(2, 1)
    u, v = u - 128, v - 128
    yy = (y - off).clamp_(min=0) * cy + (1 << 19)
    return torch.stack([((yy + cub * u) >> 20), ((yy + cvg * v + cug * u) >> 20), ((yy + cvr * v) >> 20)], 2).clamp_(0, 255).to(torch.uint8)


def bytes_staged(shape, fmt):
    """bytes the resize launch stages for one frame: per output row the two blended source rows' luma and the chroma row(s) - once
    when both blended rows share it"""
    h, w = shape
    if fmt == "bgr":
        return H * 2 * 3 * w
    sx, sy = SHIFTS[fmt]
    s0, s1 = rows_of(h)
    chroma_rows = int(np.sum(1 + ((s0 >> sy) != (s1 >> sy))))
    if fmt in ("yuyv", "uyvy"):
        return chroma_rows * 2 * w
    if fmt == "grey":
        return H * 2 * w
    return H * 2 * w + chroma_rows * 2 * (w >> sx)


def nv12_sides(eng, dev, B, seed):
    frames = [yfv2.YuvFrame(p, "nv12", "bt601") for p in make_planes(dev, B, seed, "nv12")]
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    det = eng.new_det_buffers(B)
    for t in det:
        t.zero_()
    return {"resize_nv12": lambda: eng.resize_frames_yuv(frames, out=out), "detect_nv12": lambda: eng.detect_frames_yuv(frames, 0.3, 0.4, out=det, check=False)}


def run_rounds(sides, args):
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():     # alternating: every round times each side once
            ms[k].append(timed(fn, args.iters))
    return ms


def ab(args):
    """alternating fresh processes of the in-tree build and of args.ab, each an --nv12-session"""
    other = os.path.abspath(args.ab)
    sessions = {"in_tree": [], "other": []}
    for _ in range(args.sessions):
        for who, lib in (("in_tree", None), ("other", other)):
            env = dict(os.environ)
            env.pop("YFV2_LIB", None)
            if lib:
                env["YFV2_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--nv12-session", "--frames", str(args.frames), "--iters", str(args.iters), "--rounds", str(args.rounds),
                                "--warmup", str(args.warmup), "--seed", str(args.seed)], capture_output=True, text=True, timeout=300, env=env)
            if r.returncode != 0:
                raise RuntimeError("%s session failed (%d): %s" % (who, r.returncode, r.stderr[-2000:]))
            sessions[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {"other_library": os.path.basename(other), "sessions_per_build": args.sessions}
    for side in ("resize_nv12", "detect_nv12"):
        med = {who: [s[side]["median"] for s in ss] for who, ss in sessions.items()}
        lo, hi = min(med["other"]), max(med["other"])
        mine = statistics.median(med["in_tree"])
        res[side] = {"in_tree_session_medians_ms": med["in_tree"], "other_session_medians_ms": med["other"],
                     "in_tree_spread_ms": round(max(med["in_tree"]) - min(med["in_tree"]), 4), "other_spread_ms": round(hi - lo, 4),
                     "in_tree_median_ms": round(mine, 4), "other_median_ms": round(statistics.median(med["other"]), 4),
                     "in_tree_median_inside_other_sessions_range": bool(lo <= mine <= hi),
                     "abs_difference_of_medians_ms": round(abs(mine - statistics.median(med["other"])), 4)}
    res["outputs_equal"] = len({s["digest"] for ss in sessions.values() for s in ss}) == 1
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sessions", type=int, default=4)
    ap.add_argument("--ab", default=None, help="another build of libyfv2.so (the parent commit's): alternate all-NV12 sessions with it")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--nv12-session", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    B = args.frames
    eng = yfv2.Engine(dev, H, W, 80, 3, anchors=ANCHORS, max_batch=B, plan={})
    eng.load_state_dict(yfv2.random_state_dict(0))
    if args.nv12_session:               # one build's all-NV12 figures, and a digest of what it computed
        sides = nv12_sides(eng, dev, B, args.seed)
        ms = run_rounds(sides, args)
        out = sides["resize_nv12"]()
        torch.cuda.synchronize()
        print(json.dumps({"resize_nv12": spread(ms["resize_nv12"]), "detect_nv12": spread(ms["detect_nv12"]), "digest": int(out.to(torch.int64).sum())}))
        return

    planes = {f: make_planes(dev, B, args.seed, f) for f in FORMATS}
    frames = {f: [yfv2.YuvFrame(p, f, "bt601") for p in planes[f]] for f in FORMATS}
    mixed = [frames[FORMATS[b % len(FORMATS)]][b] for b in range(B)]
    bgr = [to_bgr(p, "i444") for p in planes["i444"]]
    outs = {f: torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for f in TIMED + ("mixed", "bgr")}
    dets = {f: eng.new_det_buffers(B) for f in TIMED + ("mixed",)}
    for d in dets.values():
        for t in d:
            t.zero_()
    sides = {}
    for f in TIMED:
        sides["resize_" + f] = lambda f=f: eng.resize_frames_yuv(frames[f], out=outs[f])
        sides["detect_" + f] = lambda f=f: eng.detect_frames_yuv(frames[f], 0.3, 0.4, out=dets[f], check=False)
    sides["resize_mixed"] = lambda: eng.resize_frames_yuv(mixed, out=outs["mixed"])
    sides["detect_mixed"] = lambda: eng.detect_frames_yuv(mixed, 0.3, 0.4, out=dets["mixed"], check=False)
    sides["resize_bgr"] = lambda: eng.resize_frames(bgr, out=outs["bgr"])
    if args.child:                      # what rocprofv3 traces: the resize loops
        for _ in range(args.warmup):
            for k, fn in sides.items():
                if k.startswith("resize_"):
                    fn()
        torch.cuda.synchronize()
        for k, fn in sides.items():
            if k.startswith("resize_"):
                timed(fn, args.iters)
        return

    ms = run_rounds(sides, args)
    same = {}                           # each format's resize against the B, G, R resize of the converted frames, 32 frames at a time
    for f in TIMED:
        ok = True
        for b0 in range(0, B, 32):
            ref = eng.resize_frames([to_bgr(p, f) for p in planes[f][b0:b0 + 32]])
            ok = ok and bool(torch.equal(ref, outs[f][b0:b0 + ref.shape[0]]))
        same[f] = ok
    nv12_in_mixed = all(bool(torch.equal(outs["mixed"][b], outs["nv12"][b])) for b in range(0, B, len(FORMATS)))
    props = torch.cuda.get_device_properties(dev)
    med = {k: statistics.median(v) for k, v in ms.items()}
    staged = {f: round(sum(bytes_staged(tuple(p[0].shape) if f not in ("yuyv", "uyvy") else (p[0].shape[0], p[0].shape[1] // 2), f) for p in planes[f]) / B) for f in TIMED}
    staged["bgr"] = round(sum(bytes_staged(tuple(p.shape[:2]), "bgr") for p in bgr) / B)
    res = {"tool": "yuv_any_probe", "frames": B, "mix": ["%dx%d" % (w, h) for h, w in SIZES], "formats": list(TIMED), "iters": args.iters, "rounds": args.rounds,
           "box": {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "compute_units": props.multi_processor_count,
                   "torch": torch.__version__, "hip": torch.version.hip},
           "resize_equals_resize_bgr_of_converted": same, "nv12_frames_of_the_mixed_batch_equal_the_all_nv12_call": nv12_in_mixed,
           "ms": {k: spread(v) for k, v in ms.items()},
           "resize_over_resize_nv12": {k[7:]: round(med[k] / med["resize_nv12"], 4) for k in med if k.startswith("resize_")},
           "detect_over_detect_nv12": {k[7:]: round(med[k] / med["detect_nv12"], 4) for k in med if k.startswith("detect_")},
           "detect_fps": {k[7:]: round(B / med[k] * 1e3) for k in med if k.startswith("detect_")},
           "bytes_staged_per_frame": staged, "bytes_written_per_frame": 3 * H * W}
    if not args.no_trace:
        st = trace_stats(args, os.path.abspath(__file__))
        res["kernels"] = {name: {"calls": calls, "us": round(ns / 1e3, 2)} for name, (calls, ns) in st.items() if "resize_frames_" in name}
        res["kernels_note"] = "rocprofv3 averages per kernel NAME: the general instantiation's figure is the mean over the six formats' and the mixed batch's launches"
    if args.ab:
        res["all_nv12_in_tree_against_other_build"] = ab(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
