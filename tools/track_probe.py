#!/usr/bin/env python3
"""The per-stream IoU tracker (tracking.Tracker, include/yfv2.h yfv2_track_update) against the round trip it replaces and against
the detect call it follows, in ONE process.

Workload: --streams video streams (default 256), R = 300 rows per frame, M = 256 slots per stream, --frames frames (default 30) of
seeded boxes that drift a few pixels per frame; each frame a tenth of the objects is not seen and the rows come in a new order.  Two
runs: every row of the frame live (count = 300, of 333 objects) and a tenth of that (count = 30 of 33, as after NMS on real video).
  track_update   one call per frame on a fresh tracker, after one whole sequence as a warm-up: device events around every call,
                 the median / min / max over the frames and the first frame's time (births only)
  round trip     what a caller does without it: dets and count to the host (which waits for the device) and the numpy model's
                 update (tests/track_model.py: the edges vectorised, the walk over the edges in Python); wall-clock over the first
                 --host-frames frames, whose state and outputs are compared with the device's bit for bit
  detect_frames  the call that produces such a batch: --streams frames of a 1080p / 720p / 480p / 352 mix through Engine.detect_frames
                 (random weights; the time does not depend on them), device events, median of --iters
Prints one JSON line and writes it to --json (default profiles/track_probe.json).

--motion: the motion form (Tracker(motion=True), yfv2_track_update_motion) NEXT TO the plain one on the same two sequences in this
process: --reps passes over the sequence, the two forms alternating, a fresh tracker each pass, device events around every call;
per form the median / min / max over all frames of all passes, and motion / plain of the medians.  The motion form's state and
outputs of the first --host-frames frames are compared with tests/track_motion_model.py bit for bit.  Default --json:
profiles/track_motion_probe.json.

--two-pass: the two-pass form (Tracker(two_pass=True), yfv2_track_update_two_pass) NEXT TO the one-pass form of the same layout
(--motion chooses it) on the same two sequences, in which --low-share of the rows (default 0.3) carry a conf in [0.1, 0.5) - LOW
rows; the others stay in [0.5, 1.0].  Passes, alternation and statistics as for --motion.  The two-pass form's state and outputs of
the first --host-frames frames are compared with tests/track_two_pass_model.py bit for bit.  The rounds of each pass are the model's
parallel form's over ALL --frames frames of the first --round-streams streams (default 8; on the host, nothing timed), reported
without the first frame, which has no tracks and so no round.  Default --json: profiles/track_two_pass_probe.json, with --motion
profiles/track_two_pass_motion_probe.json.

--appearance: the appearance form (Tracker(appearance=dict(dim=--dim)), yfv2_track_update_appearance; fp32 embeddings of one width,
every object a unit vector of its own plus noise) on the same regime, in the plain and in the motion layout (--motion: the motion
layout only; --two-pass: two passes in every variant).  THREE variants alternate, a fresh tracker each pass: the shipped form of the
layout and pass count; the appearance form with app_thres = +inf - the rows' norms, the gating and the features' upkeep, with no
cosine ever counting; the appearance form at its defaults (prox_thres 0.5, app_thres 0.75, alpha 0.9).  Passes and statistics as for
--motion.  The state of the +inf variant must equal the shipped form's; the default variant's state, features and outputs of the
first --host-frames frames of the first streams are compared with tests/track_appearance_model.py bit for bit, and the model's
parallel form gives the first pass's rounds, the gated pairs (pairs whose cosine the first pass needs) and the matches valued by the
cosine per frame.  What the form does not do: embeddings other than fp32; more than one width per tracker; re-identification
after a track's death; a gallery of several features per track; appearance in the second pass; anything but the maximum of IoU and
cosine as the fused value (BoT-SORT's minimum of the two distances), which cannot separate a wrong pair at IoU ~1 from a right pair
at cosine ~1; it is not a DetectPipeline form and not in yfv2.hpp.  Default --json: profiles/track_appearance_probe.json.
usage: python tools/track_probe.py [--streams 256] [--frames 30] [--host-frames 2] [--iters 20] [--motion [--reps 5]]
                                   [--two-pass [--motion] [--low-share 0.3] [--reps 5] [--round-streams 8]]
                                   [--appearance [--motion] [--two-pass] [--dim 128] [--reps 5] [--round-streams 8]]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import yolo_fastestv2_amd as yfv2  # noqa: E402

ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]  # data/coco.data:17
SIZES = [(1080, 1920), (720, 1280), (480, 640), (352, 352)]   # (h, w)
R, M = 300, 256


def sequence(rng, S, T, live, seen_n, low_share=0.0):
    """T arrays (S, R, 6) and counts (S): `live` objects per stream on a 1920 x 1080 canvas, drifting up to 3 pixels per frame, a
    random `seen_n` of them in each frame; low_share of a frame's rows get a conf in [0.1, 0.5), the others one in [0.5, 1.0]"""
    pos = rng.uniform(0, [1800, 1000], (S, live, 2))
    size = rng.uniform(30, 120, (S, live, 2))
    cls = rng.integers(0, 80, (S, live)).astype(np.float32)
    out = []
    for _ in range(T):
        pos += rng.uniform(-3, 3, pos.shape)
        dets = np.zeros((S, R, 6), np.float32)
        count = np.zeros(S, np.int32)
        for s in range(S):
            seen = rng.permutation(live)[:seen_n]
            conf = np.sort(rng.uniform(0.3, 1.0, len(seen)))[::-1]
            if low_share > 0.0:
                n_low = int(round(low_share * len(seen)))
                conf = np.sort(np.concatenate([rng.uniform(0.5, 1.0, len(seen) - n_low), rng.uniform(0.1, 0.5, n_low)]))[::-1]
            dets[s, :len(seen)] = np.concatenate([pos[s, seen], pos[s, seen] + size[s, seen], conf[:, None], cls[s, seen, None]], axis=1)
            count[s] = len(seen)
        out.append((dets, count))
    return out


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def run(eng, dev, seq, host_frames):
    import track_model
    S = seq[0][0].shape[0]
    rule = dict(max_tracks=M, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30, confirm_hits=3)
    dseq = [(torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev)) for d, c in seq]
    out = (torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R, 6), device=dev),
           torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S,), device=dev, dtype=torch.int32))
    warm = yfv2.Tracker(eng, S, **rule)
    for d, c in dseq:
        warm.update(d, c, fresh=True, out=out)
    torch.cuda.synchronize()
    tr = yfv2.Tracker(eng, S, **rule)
    ms, fresh = [], 0
    for d, c in dseq:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.update(d, c, fresh=True, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        fresh += int(out[4].sum())
    same = bool(torch.equal(tr.state, warm.state))
    # the round trip on the first frames, compared with a third tracker stepped alongside
    model, chk = track_model.Model(S, **rule), yfv2.Tracker(eng, S, **rule)
    host_ms = []
    for d, c in dseq[:host_frames]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = model.update(d.cpu().numpy(), c.cpu().numpy())
        host_ms.append((time.perf_counter() - t0) * 1e3)
        got = chk.update(d, c, fresh=True, out=out)
        same = (same and bool(torch.equal(chk.state.cpu(), torch.from_numpy(model.state))) and bool(torch.equal(got[0].cpu(), torch.from_numpy(want["track_id"])))
                and bool(torch.equal(got[1].cpu(), torch.from_numpy(want["track_hits"]))) and bool(torch.equal(got[4].cpu(), torch.from_numpy(want["fresh_count"]))))
    head = tr.state[:, :6].sum(0).tolist()
    return {"rows_per_frame": int(round(float(np.mean([c.mean() for _d, c in seq])))), "track_update_ms": spread(ms), "first_frame_ms": round(ms[0], 4),
            "round_trip_ms": round(statistics.median(host_ms), 2), "equals_model": same, "fresh_rows": fresh,
            "issued": head[0], "live": head[1], "deaths": head[4], "dropped": head[5],
            "speedup": round(statistics.median(host_ms) / statistics.median(ms), 1)}


def run_motion(eng, dev, seq, host_frames, reps):
    import track_motion_model
    S = seq[0][0].shape[0]
    rule = dict(max_tracks=M, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30, confirm_hits=3)
    dseq = [(torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev)) for d, c in seq]
    outs = {False: (torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R, 6), device=dev),
                    torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S,), device=dev, dtype=torch.int32))}
    outs[True] = outs[False] + (torch.empty((S, R, 4), device=dev),)
    ms, states = {False: [], True: []}, {}
    for rep in range(reps + 1):                             # pass 0 is the warm-up of both forms
        for motion in (False, True):
            tr = yfv2.Tracker(eng, S, motion=motion or None, **rule)
            for d, c in dseq:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.update(d, c, fresh=True, box=motion, out=outs[motion])
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[motion].append(e0.elapsed_time(e1))
            same = motion not in states or bool(torch.equal(states[motion], tr.state))
            states[motion] = tr.state.clone()
            assert same, "two passes over one sequence left different states"
    # the motion form against its model on the first frames
    model, chk = track_motion_model.Model(S, **rule), yfv2.Tracker(eng, S, motion=True, **rule)
    same = True
    for d, c in dseq[:host_frames]:
        want = model.update(d.cpu().numpy(), c.cpu().numpy())
        got = chk.update(d, c, fresh=True, box=True, out=outs[True])
        same = (same and bool(torch.equal(chk.state.cpu(), torch.from_numpy(model.state))) and bool(torch.equal(got[0].cpu(), torch.from_numpy(want["track_id"])))
                and bool(torch.equal(got[5].cpu().view(torch.int32), torch.from_numpy(want["track_box"]).view(torch.int32)))
                and bool(torch.equal(got[4].cpu(), torch.from_numpy(want["fresh_count"]))))
    heads = {k: states[k][:, :6].sum(0).tolist() for k in states}
    return {"rows_per_frame": int(round(float(np.mean([c.mean() for _d, c in seq])))), "reps": reps,
            "track_update_ms": spread(ms[False]), "track_update_motion_ms": spread(ms[True]),
            "ratio": round(statistics.median(ms[True]) / statistics.median(ms[False]), 3), "motion_equals_model": same,
            "issued": {"plain": heads[False][0], "motion": heads[True][0]}, "live": {"plain": heads[False][1], "motion": heads[True][1]}}


def run_two_pass(eng, dev, seq, host_frames, reps, motion, round_streams):
    import track_model
    import track_two_pass_model
    S = seq[0][0].shape[0]
    rule = dict(max_tracks=M, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30, confirm_hits=3)
    dseq = [(torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev)) for d, c in seq]
    base = (torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R, 6), device=dev),
            torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S,), device=dev, dtype=torch.int32))
    box = (torch.empty((S, R, 4), device=dev),) if motion else ()
    outs = {False: base + box, True: base + box + (torch.empty((S, R), device=dev, dtype=torch.int32),)}
    ms, states = {False: [], True: []}, {}
    for rep in range(reps + 1):                             # pass 0 is the warm-up of both forms
        for two in (False, True):
            tr = yfv2.Tracker(eng, S, motion=motion or None, two_pass=two or None, **rule)
            for d, c in dseq:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.update(d, c, fresh=True, box=motion, passes=two, out=outs[two])
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[two].append(e0.elapsed_time(e1))
            same = two not in states or bool(torch.equal(states[two], tr.state))
            states[two] = tr.state.clone()
            assert same, "two passes over one sequence left different states"
    # the two-pass form against its model on the first frames
    model, chk = track_two_pass_model.Model(S, motion=motion or None, **rule), yfv2.Tracker(eng, S, motion=motion or None, two_pass=True, **rule)
    same = True
    for d, c in dseq[:host_frames]:
        want = model.update(d.cpu().numpy(), c.cpu().numpy())
        got = chk.update(d, c, fresh=True, box=motion, passes=True, out=outs[True])
        same = (same and bool(torch.equal(chk.state.cpu(), torch.from_numpy(model.state))) and bool(torch.equal(got[0].cpu(), torch.from_numpy(want["track_id"])))
                and bool(torch.equal(got[-1].cpu(), torch.from_numpy(want["track_pass"]))) and bool(torch.equal(got[4].cpu(), torch.from_numpy(want["fresh_count"]))))
    # the rounds of each pass: the model's parallel form over the whole sequence of the first streams, the trackless first frame left out
    K = min(round_streams, S)
    par = track_two_pass_model.Model(K, motion=motion or None, **rule)
    for d, c in seq:
        par.update(d[:K], c[:K], match=track_model.mutual_best)
    rounds = par.stats["rounds"][K:]
    heads = {k: states[k][:, :7].sum(0).tolist() for k in states}
    low = float(np.mean([((d[:, :, 4] < 0.5) & (np.arange(R)[None, :] < c[:, None])).sum() / max(int(c.sum()), 1) for d, c in seq]))
    return {"rows_per_frame": int(round(float(np.mean([c.mean() for _d, c in seq])))), "low_share": round(low, 3), "reps": reps,
            "one_pass_ms": spread(ms[False]), "two_pass_ms": spread(ms[True]),
            "ratio": round(statistics.median(ms[True]) / statistics.median(ms[False]), 3), "two_pass_equals_model": same,
            "model_rounds": {"streams": K, "frames": len(seq) - 1, "of": "every frame but the first of the first streams, host model",
                             "first_pass": {"max": max(r[0] for r in rounds), "mean": round(float(np.mean([r[0] for r in rounds])), 2)},
                             "second_pass": {"max": max(r[1] for r in rounds), "mean": round(float(np.mean([r[1] for r in rounds])), 2)}},
            "second_pass_matches": heads[True][6],
            "issued": {"one_pass": heads[False][0], "two_pass": heads[True][0]}, "live": {"one_pass": heads[False][1], "two_pass": heads[True][1]}}


def sequence_emb(rng, S, T, live, seen_n, D, noise=0.1):
    """sequence() with an embedding per row: every object has a unit vector of its own, a row's embedding is that vector plus
    noise of relative size `noise`.  -> T (dets (S, R, 6), count (S), emb (S, R, D))"""
    pos = rng.uniform(0, [1800, 1000], (S, live, 2))
    size = rng.uniform(30, 120, (S, live, 2))
    cls = rng.integers(0, 80, (S, live)).astype(np.float32)
    proto = rng.normal(size=(S, live, D)).astype(np.float32)
    proto /= np.linalg.norm(proto, axis=2, keepdims=True)
    out = []
    for _ in range(T):
        pos += rng.uniform(-3, 3, pos.shape)
        dets, emb = np.zeros((S, R, 6), np.float32), np.zeros((S, R, D), np.float32)
        count = np.zeros(S, np.int32)
        for s in range(S):
            seen = rng.permutation(live)[:seen_n]
            conf = np.sort(rng.uniform(0.3, 1.0, len(seen)))[::-1]
            dets[s, :len(seen)] = np.concatenate([pos[s, seen], pos[s, seen] + size[s, seen], conf[:, None], cls[s, seen, None]], axis=1)
            emb[s, :len(seen)] = proto[s, seen] + (noise / np.sqrt(D)) * rng.normal(size=(len(seen), D)).astype(np.float32)
            count[s] = len(seen)
        out.append((dets, count, emb))
    return out


def run_appearance(eng, dev, seq, host_frames, reps, motion, two, round_streams, D):
    """three variants alternating in one process: the shipped form of the layout and pass count, the appearance form with
    app_thres = +inf (the norms, the gating and the features' upkeep, no cosine ever counts) and the appearance form at its defaults"""
    import track_appearance_model
    import track_model
    S = seq[0][0].shape[0]
    rule = dict(max_tracks=M, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30, confirm_hits=3)
    dseq = [(torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(e).to(dev)) for d, c, e in seq]
    base = (torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S, R, 6), device=dev),
            torch.empty((S, R), device=dev, dtype=torch.int32), torch.empty((S,), device=dev, dtype=torch.int32))
    base += ((torch.empty((S, R, 4), device=dev),) if motion else ()) + ((torch.empty((S, R), device=dev, dtype=torch.int32),) if two else ())
    outs = {"shipped": base, "inf": base + (torch.empty((S, R), device=dev),), "defaults": base + (torch.empty((S, R), device=dev),)}
    apps = {"shipped": None, "inf": dict(dim=D, app_thres=float("inf")), "defaults": dict(dim=D)}
    ms, states = {k: [] for k in apps}, {}
    for rep in range(reps + 1):                             # pass 0 is the warm-up of the three forms
        for k, app in apps.items():
            tr = yfv2.Tracker(eng, S, motion=motion or None, two_pass=two or None, appearance=app, **rule)
            for d, c, e in dseq:
                kw = dict(emb=e, cos=True) if app else {}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.update(d, c, fresh=True, box=motion, passes=two, out=outs[k], **kw)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[k].append(e0.elapsed_time(e1))
            same = k not in states or bool(torch.equal(states[k], tr.state))
            states[k] = tr.state.clone()
            assert same, "two passes over one sequence left different states"
    # the appearance form at its defaults against its model, and the model's rounds and gated pairs, on the first streams
    K = min(round_streams, S)
    model = track_appearance_model.Model(K, appearance=apps["defaults"], second=two or None, motion=motion or None, **rule)
    chk = yfv2.Tracker(eng, K, motion=motion or None, two_pass=two or None, appearance=apps["defaults"], **rule)
    same = True
    for t, (d, c, e) in enumerate(seq):
        want = model.update(d[:K], c[:K], e[:K], match=track_model.mutual_best)
        if t < host_frames:
            got = chk.update(dseq[t][0][:K].contiguous(), dseq[t][1][:K].contiguous(), emb=dseq[t][2][:K].contiguous(), cos=True)
            same = (same and bool(torch.equal(chk.state.cpu(), torch.from_numpy(model.state))) and bool(torch.equal(chk.feat.cpu(), torch.from_numpy(model.feat)))
                    and bool(torch.equal(got[0].cpu(), torch.from_numpy(want["track_id"])))
                    and bool(torch.equal(got[-1].cpu().view(torch.int32), torch.from_numpy(want["track_cos"]).view(torch.int32))))
    rounds = model.stats["rounds"][K:]
    frames = K * (len(seq) - 1)
    heads = {k: states[k][:, :8].sum(0).tolist() for k in states}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"rows_per_frame": int(round(float(np.mean([c.mean() for _d, c, _e in seq])))), "reps": reps,
            "shipped_ms": spread(ms["shipped"]), "appearance_inf_ms": spread(ms["inf"]), "appearance_ms": spread(ms["defaults"]),
            "ratio_inf": round(med["inf"] / med["shipped"], 3), "ratio": round(med["defaults"] / med["shipped"], 3),
            "inf_state_equals_shipped": bool(torch.equal(states["inf"], states["shipped"])), "appearance_equals_model": same,
            "model": {"streams": K, "frames": len(seq) - 1, "of": "every frame but the first of the first streams, host model, parallel walk",
                      "first_pass_rounds": {"max": max(r[0] for r in rounds), "mean": round(float(np.mean([r[0] for r in rounds])), 2)},
                      "gated_pairs_per_frame": round(model.stats["gated"] / frames, 1),
                      "by_appearance_per_frame": round(model.stats["by_appearance"] / frames, 1)},
            "by_appearance": heads["defaults"][7], "issued": {k: heads[k][0] for k in heads}, "live": {k: heads[k][1] for k in heads}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--motion", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--two-pass", action="store_true")
    ap.add_argument("--low-share", type=float, default=0.3)
    ap.add_argument("--round-streams", type=int, default=8)
    ap.add_argument("--appearance", action="store_true")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.json is None and args.appearance:
        args.json = os.path.join(REPO, "profiles", "track_appearance%s%s_probe.json" % ("_two_pass" if args.two_pass else "", "_motion" if args.motion else ""))
    if args.json is None:
        args.json = os.path.join(REPO, "profiles", ("track_two_pass_motion_probe.json" if args.motion else "track_two_pass_probe.json") if args.two_pass else "track_motion_probe.json" if args.motion else "track_probe.json")

    dev = torch.device("cuda:0")
    S = args.streams
    eng = yfv2.Engine(dev, 352, 352, 80, 3, anchors=ANCHORS, max_batch=S, plan={})
    eng.load_state_dict(yfv2.random_state_dict(0))
    rng = np.random.default_rng(args.seed)
    if args.appearance:
        layouts = [True] if args.motion else [False, True]
        res = {"tool": "track_probe --appearance" + (" --motion" if args.motion else "") + (" --two-pass" if args.two_pass else ""), "streams": S, "R": R, "M": M,
               "D": args.dim, "frames": args.frames, "host_frames": args.host_frames, "passes": 2 if args.two_pass else 1,
               "appearance": dict(prox_thres=0.5, app_thres=0.75, alpha=0.9), "round_trip_ms_it_replaces": "profiles/track_probe.json round_trip_ms"}
        full, sparse = sequence_emb(rng, S, args.frames, 333, 300, args.dim), sequence_emb(rng, S, args.frames, 33, 30, args.dim)
        for motion in layouts:
            res["motion" if motion else "plain"] = {
                "full": run_appearance(eng, dev, full, args.host_frames, args.reps, motion, args.two_pass, min(args.round_streams, 4), args.dim),
                "sparse": run_appearance(eng, dev, sparse, args.host_frames, args.reps, motion, args.two_pass, min(args.round_streams, 4), args.dim)}
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
        return
    if args.two_pass:
        res = {"tool": "track_probe --two-pass" + (" --motion" if args.motion else ""), "streams": S, "R": R, "M": M, "frames": args.frames,
               "host_frames": args.host_frames, "layout": "motion" if args.motion else "plain",
               "full": run_two_pass(eng, dev, sequence(rng, S, args.frames, 333, 300, args.low_share), args.host_frames, args.reps, args.motion, args.round_streams),
               "sparse": run_two_pass(eng, dev, sequence(rng, S, args.frames, 33, 30, args.low_share), args.host_frames, args.reps, args.motion, args.round_streams)}
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
        return
    if args.motion:
        res = {"tool": "track_probe --motion", "streams": S, "R": R, "M": M, "frames": args.frames, "host_frames": args.host_frames,
               "full": run_motion(eng, dev, sequence(rng, S, args.frames, 333, 300), args.host_frames, args.reps),
               "sparse": run_motion(eng, dev, sequence(rng, S, args.frames, 33, 30), args.host_frames, args.reps)}
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
        return
    res = {"tool": "track_probe", "streams": S, "R": R, "M": M, "frames": args.frames, "host_frames": args.host_frames,
           "full": run(eng, dev, sequence(rng, S, args.frames, 333, 300), args.host_frames),
           "sparse": run(eng, dev, sequence(rng, S, args.frames, 33, 30), args.host_frames)}
    # the call that produces such a batch
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    order = np.random.default_rng(args.seed).permutation(np.arange(S) % len(SIZES))
    frames = [torch.randint(0, 256, SIZES[k] + (3,), generator=gen, device=dev, dtype=torch.uint8) for k in order]
    bufs = eng.new_det_buffers(S)
    for _ in range(3):
        eng.detect_frames(frames, 0.3, 0.4, out=bufs, check=False)
    torch.cuda.synchronize()
    det_ms = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.detect_frames(frames, 0.3, 0.4, out=bufs, check=False)
        e1.record()
        torch.cuda.synchronize()
        det_ms.append(e0.elapsed_time(e1))
    res["detect_frames_ms"] = spread(det_ms)
    for k in ("full", "sparse"):
        res[k]["fraction_of_detect"] = round(res[k]["track_update_ms"]["median"] / res["detect_frames_ms"]["median"], 3)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
