#!/usr/bin/env python3
"""bench.py - images/sec of the Yolo-FastestV2 hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: one rank per GPU over RCCL.  Under torch.distributed.run the ranks read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*;
     called PLAIN with --gpus N > 1, bench.py launches itself: it re-executes under `python -m torch.distributed.run --nnodes=1
     --nproc-per-node N --master-addr 127.0.0.1 --master-port <free port>` and rank 0 prints the one JSON line.)

A "step" is one pass of the whole hot path - forward (backbone + FPN + heads) ->
anchor decode -> class-aware NMS - over one batch of 256 synthetic 352x352x3 fp32
images per GPU that are already resident in HBM, plus (N > 1) the RCCL
all-gather of the padded detections.  BASELINE.json configs[1] (forward only) is
a strict subset of the timed work; its rate is reported as `forward_only_img_s`.
Weights are seeded random-init of the reference architecture (no checkpoint
download is possible) and data is torch.rand: with those, every image yields the
maximum of 300 detections, i.e. NMS runs its WORST case inside `value`.
Consecutive steps are independent batches: they rotate over three handles
(own workspaces) on three HIP streams, so that one step's launches fill the
under-filled tails of its neighbours' (all K steps complete inside the timed
region); `single_stream_img_s` (--full) is the same K steps on one handle and one stream.
Order of a run: set-up (handles, one call per handle) -> SPIN-UP: the device is held under load for --spinup-seconds (2 s)
of the same steps, because a fresh process runs its first steps 8-10 % slower until the device has left its idle power state
(reported as `spinup` by --full, not as warm-up) -> exactly W warm-up steps -> ONE timed block of EXACTLY K steps, bracketed by
barrier + device synchronize: `value` / `ms_per_step` -> with --dump-outputs DIR, the last timed step's detections (what a
caller of Engine.detect receives) as DIR/*.npy -> the JSON line.  The inputs are seeded, so the same arguments give the same
outputs from run to run.  A plain run stops there and prints only the headline fields.

--full measures everything else, after the same headline: --blocks (15) back-to-back timed blocks of EXACTLY K steps in all,
the headline's first; every block's rate, the min / max / median ride along (`blocks`), so that a clock ramp or a noisy box
is visible instead of guessed.  `box` records what the
run ran at: the effective shader clock measured by the shader itself (s_memtime against the constant reference clock) under
an all-CU vector load before and after the timed blocks and - by sleeping probe waves on a side stream - WHILE the timed kind
of step loop and the per-kernel profile run, plus whatever rocm-smi / sysfs give on the box (performance level, power cap,
partition modes).  `kernel_table` carries shader cycles next to milliseconds.
The configs[2] variant the survey specifies (COCO weights, a 256-batch built from
the shipped JPEGs, thresholds 0.3/0.4 and 0.01/0.4) is timed as well and reported
in `coco_e2e` (extra fields, never `value`).

Prints ONE JSON line on rank 0 (see README / DESIGN.md for the field meanings):
  value      whole-job images/s (all ranks' images / max-over-ranks time of the K timed steps), consecutive steps (= batches
             of 256) pipelined over three handles / HIP streams: up to three batches are in flight at any time
  ms_per_step  milliseconds per timed step (the same block)
--full adds:
  single_stream_img_s   the same steps strictly one batch at a time on one handle and one stream
  fp32_mfma_plan   the same two figures with every contraction on the fp32 matrix instructions (YFV2_BF6=0) instead of fp16x3
  roofline   the kernel that owns the most forward time (sum over its launches, the
             top row of a rocprofv3 --stats table): algorithmic bytes (SURVEY.md 8(d):
             EXTERNAL reads + writes for a fused launch) and flops of its launches /
             their summed duration, measured with HIP events on the launch stream inside
             this process (yfv2_profile_forward: every launch records its OWN begin and end
             into a hipEvent pair - hipExtLaunchKernel's start / stop events, the dispatch
             timestamps a rocprofv3 trace reports; events recorded in front of and behind
             a launch read 3-12 us more); `bound` follows its arithmetic
             intensity.  `traffic` = HBM bytes per launch from the PMC passes under
             profiles/ (tools/gpu_traffic.sh) IF that profile was taken on this very
             source tree (fingerprint match), else null.
  kernel_table  the same figures for every kernel of the forward: hbm_frac_external (of the nominal
             8 TB/s) and hbm_frac_of_achievable (of the ~6.3 TB/s the guide calls achievable);
             mfma_pipe_frac = matrix-pipe flops issued / that pipe's dense peak - on the default
             plan 3 x algorithmic flops / 2.5 PFLOP/s (fp16x3: three f16 products per MAC; the
             depthwise flops, which run on the VALU, are included in `flops`: an upper bound) -
             next to mfma_busy from the SQ counter pass (same fingerprint rule); no fraction
             can exceed 1
  cpu_baseline  the CPU oracle (same ATen CPU ops as the reference + numpy
             decode/NMS) timed on this box's host cores on a bounded sample
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec ...
HBM_ACHIEVABLE_GBS = 6300.0    # ... of which ~6.3 TB/s are achievable (same guide, HBM section)
MFMA_F32_PEAK_TF = 157.3       # dense fp32 MFMA peak (= fp32 vector peak): the pipe of the YFV2_BF6=0 plan
MFMA_F16_PEAK_TF = 2500.0      # dense fp16 MFMA peak: the pipe the default plan's fp16x3 contractions run on
# The default plan spends THREE f16 products per algorithmic MAC (w1 x2 + w2 x1 + w1 x1), so its ceiling in algorithmic
# flops is a third of the f16 peak; the ridge that decides `bound` follows from that ceiling.
# the plan of the measured handles: the default one unless the caller's environment asks for another (YFV2_BF6=0 etc. - the library itself
# reads no environment; yolo_fastestv2_amd._lib.plan_from_env maps these onto yfv2_plan)
FP16X3 = os.environ.get("YFV2_BF6", "1") != "0"
PIPE_PEAK_TF, PIPE_COST = (MFMA_F16_PEAK_TF, 3.0) if FP16X3 else (MFMA_F32_PEAK_TF, 1.0)
RIDGE_FLOP_PER_BYTE = (PIPE_PEAK_TF / PIPE_COST) * 1e12 / (HBM_PEAK_GBS * 1e9)   # 104 flop/B (fp16x3), 19.7 (fp32 MFMA)
sys.path.insert(0, os.path.join(REPO, "tools"))
from srchash import source_hash  # noqa: E402


def newest_profile(suffix, src_hash):
    """profiles/*<suffix> with the newest name whose `src_hash` equals this tree's fingerprint, or None"""
    import glob
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "*" + suffix)), reverse=True):
        try:
            with open(f) as fh:
                j = json.load(fh)
        except (OSError, ValueError):
            continue
        if j.get("src_hash") == src_hash:
            j["_file"] = os.path.basename(f)
            return j
    return None


def profile_lookup(prof, kernel, field, launches, mean=False):
    """Sum (or mean) of `field` over the profile rows whose kernel name contains one of the '+'-separated prefixes of
    `kernel` (bench groups by symbol-name prefix, e.g. 'pw_kernel<192,' or 's2px_proj_kernel + s2px_main_kernel')."""
    if not prof:
        return None
    vals = []
    for part in kernel.split(" + "):
        hit = [(v.get("n", 0), v[field]) for k, v in prof["kernels"].items() if part in k and field in v]
        if len(hit) > 1:      # several instantiations of one template in the profile (front2_kernel<0, false> / <0, true>: the fp32 and
            hit.sort(reverse=True)   # the uint8 form): the one the timed loop ran is the one with by far the most launches
            if hit[0][0] < 20 * max(1, hit[1][0]):
                return None
        if not hit:
            return None
        vals.append(hit[0][1])
    if mean:
        return round(sum(vals) / len(vals), 2)
    return sum(vals) * launches      # per-launch means -> bytes per forward (a '+' step launches each of its kernels once)
PLAN = {}
ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]  # data/coco.data:17


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU (BASELINE.json: 256)")
    ap.add_argument("--conf", type=float, default=0.3)
    ap.add_argument("--iou", type=float, default=0.4)
    ap.add_argument("--full", action="store_true", help="after the headline, measure everything else: timed blocks, clocks, one stream, forward only, "
                                                        "roofline, fp32 plan, COCO, CPU baseline, training (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's detections, counts and survivor indices as DIR/<name>.npy")
    ap.add_argument("--profile-iters", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=15, help="--full: back-to-back timed blocks of --steps steps each, the headline's first (`blocks`)")
    ap.add_argument("--inputs", type=int, default=3, help="distinct resident input batches the steps rotate over (3 x 381 MB exceeds the 256 MB Infinity Cache: "
                                                          "the streaming front end provably reads HBM)")
    ap.add_argument("--spinup-seconds", type=float, default=2.0, help="set-up: hold the device under load this long before the warm-up (a fresh process runs its first steps 8-10 %% slower until the device has left its idle power state)")
    ap.add_argument("--pipeline", type=int, default=3, help="handles / HIP streams consecutive steps rotate over (1 = one handle, one stream)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target wall time of the CPU baseline leg (one instance; the concurrent-instances figure takes about as long again)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the fp32-plan, COCO and training extras (counter passes)")
    ap.add_argument("--weights", choices=("random", "coco"), default="random")
    ap.add_argument("--launcher-selftest", action="store_true",
                    help="NOT a measurement: run the launch / sharding / gather logic of this script on CPU tensors with gloo and a stand-in "
                         "engine (tests/test_abi_and_host.py: `bench.py --gpus 2 --launcher-selftest` must self-launch and print one line)")
    return ap.parse_args()


def batch_from_reference_images(images_u8, n, seed):
    """BASELINE configs[2] input: a batch built from the shipped JPEGs with deterministic variants
    (h-flip, +-16 px roll, gain in [0.8, 1.2]) so that it contains real objects (same recipe as tests/test_gpu_parity.py)."""
    base = torch.from_numpy(images_u8).float() / 255.0
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        x = base[i % base.shape[0]]
        if int(torch.randint(0, 2, (1,), generator=g)):
            x = x.flip(-1)
        dy, dx = (int(v) for v in torch.randint(-16, 17, (2,), generator=g))
        x = torch.roll(x, shifts=(dy, dx), dims=(-2, -1))
        gain = 0.8 + 0.4 * float(torch.rand(1, generator=g))
        out.append((x * gain).clamp(0, 1))
    return torch.stack(out)


def _cpu_instance(args):
    """cpu_baseline's concurrent-instances leg: ONE oracle instance of `threads` threads in its own process (spawned: no GPU state),
    batches of `bs` seeded synthetic images through forward (ATen CPU) + decode + NMS for about `seconds`.  Returns (images, seconds)
    of its own loop (after its own warm-up): the instances' rates are summed."""
    threads, seconds, bs, conf, iou, seed = args
    import torch as T
    T.set_num_threads(threads)
    sys.path.insert(0, REPO)
    import yolo_fastestv2_amd as yfv2
    from oracle import yfv2_oracle as oracle
    sd = yfv2.random_state_dict(0)
    x = T.rand(bs, 3, 352, 352, generator=T.Generator().manual_seed(seed))
    oracle.forward(sd, x[:4])
    n, t0 = 0, time.perf_counter()
    while True:
        oracle.detect(sd, x, ANCHORS, 352, conf, iou)
        n += bs
        el = time.perf_counter() - t0
        if el >= seconds:
            return n, el


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(path, dets, idx, cnt):
    """--dump-outputs: what Engine.detect hands its caller, as .npy files - detections (B,300,6) float32, survivor_indices (B,300)
    and counts (B,) float64.  Only the first counts[b] rows of an image are results: the padding is written as 0 (indices -1), so
    that two builds compare file for file.  A batch too large for DUMP_MAX_BYTES keeps a fixed, seeded sample of its images
    (image_index.npy says which)."""
    import numpy as np
    n = cnt.cpu().numpy().astype(np.int64)
    d, i = dets.cpu().numpy(), idx.cpu().numpy()
    valid = np.arange(d.shape[1])[None, :] < n[:, None]
    out = {"detections": np.where(valid[..., None], d, 0.0).astype(np.float32), "survivor_indices": np.where(valid, i, -1).astype(np.float64),
           "counts": n.astype(np.float64)}
    per_image = sum(v[0].nbytes for v in out.values())
    if per_image * len(n) > DUMP_MAX_BYTES:
        keep = np.sort(np.random.default_rng(0).choice(len(n), DUMP_MAX_BYTES // per_image - 1, replace=False))
        out = {k: v[keep] for k, v in out.items()}
        out["image_index"] = keep.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, v in out.items():
        np.save(os.path.join(path, k + ".npy"), v)


def timed(fn, steps, sync, barrier, finish=None):
    barrier(); sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    if finish is not None:
        finish()          # collectives still in flight belong to the timed steps
    sync(); barrier()
    return time.perf_counter() - t0


def self_launch(a):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: become `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py <the same arguments>` (exec: same pid, same stdout -
    rank 0's JSON line is this process's output).  The port is one the kernel just handed out."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on these hosts (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", "8")
    sys.stdout.flush(); sys.stderr.flush()
    os.execve(sys.executable, cmd, env)


def sysfs_power_clock(pci=None, root="/sys/class/drm"):
    """{card: {power_w, sclk_mhz}} from sysfs hwmon (a handful of file reads: cheap enough to take WHILE steps are queued on the
    device).  The box exposes every GPU of the node; `pci` (the HIP device's bus id, when torch reports it) marks ours."""
    import glob
    out = {}
    for card in sorted(glob.glob(os.path.join(root, "card[0-9]*", "device"))):
        name = os.path.basename(os.path.dirname(card))
        rec = {}
        for hw in glob.glob(os.path.join(card, "hwmon", "hwmon*")):
            for key, fn, scale in (("power_w", "power1_input", 1e-6), ("power_w", "power1_average", 1e-6), ("sclk_mhz", "freq1_input", 1e-6)):
                try:
                    with open(os.path.join(hw, fn)) as fh:
                        rec.setdefault(key, round(float(fh.read().strip()) * scale, 1))
                except (OSError, ValueError):
                    pass
        if pci:
            try:
                rec["ours"] = pci.lower() in os.path.realpath(card).lower()
            except OSError:
                pass
        if rec.get("power_w") is not None or rec.get("sclk_mhz") is not None:
            out[name] = rec
    mine = {k: v for k, v in out.items() if v.get("ours")}
    return mine if mine else out          # ours when the bus id identifies it, else every GPU of the node that reports


def smi_snapshot(index, pci=None):
    """Best effort: what the box's management interface says about the device (performance level, power cap, clocks, partition
    modes).  Containers of this pool often expose little; whatever is readable is recorded, nothing is required."""
    import glob
    import subprocess
    out = {}
    try:
        r = subprocess.run(["rocm-smi", "-d", str(index), "--showperflevel", "--showmaxpower", "--showpower", "--showclocks", "--showsclkrange",
                            "--showcomputepartition", "--showmemorypartition", "--json"], capture_output=True, text=True, timeout=30)
        j = json.loads(r.stdout[r.stdout.index("{"):]) if "{" in r.stdout else {}
        for card, kv in j.items():
            if isinstance(kv, dict):
                out["rocm_smi"] = {k: v for k, v in kv.items() if any(t in k.lower() for t in ("perf", "power", "sclk", "mclk", "fclk", "partition", "socclk"))}
                break
    except Exception as e:                      # noqa: BLE001 - telemetry only
        out["rocm_smi_error"] = repr(e)[:120]
    sysfs = {}
    for card in sorted(glob.glob("/sys/class/drm/card[0-9]*/device")):
        if pci:
            try:
                if pci.lower() not in os.path.realpath(card).lower():
                    continue                     # another GPU of the node
            except OSError:
                pass
        for name in ("power_dpm_force_performance_level", "current_compute_partition", "current_memory_partition", "pp_dpm_sclk", "pp_dpm_mclk"):
            try:
                with open(os.path.join(card, name)) as fh:
                    sysfs.setdefault(os.path.basename(os.path.dirname(card)), {})[name] = fh.read().strip()[:200]
            except OSError:
                pass
        for hw in glob.glob(os.path.join(card, "hwmon", "hwmon*")):
            for name in ("power1_cap", "power1_cap_max", "power1_average", "power1_input", "freq1_input"):
                try:
                    with open(os.path.join(hw, name)) as fh:
                        sysfs.setdefault(os.path.basename(os.path.dirname(card)), {})[name] = fh.read().strip()[:40]
                except OSError:
                    pass
    if sysfs:
        out["sysfs"] = sysfs
    return out


class _StandInEngine:
    """--launcher-selftest only: the call shape of Engine.detect on CPU tensors; detections are a function of the rank and the
    step, so that the gathered buffer can be checked word for word."""

    def __init__(self, rank):
        self.rank, self.calls = rank, 0

    def detect(self, x, conf_thres, iou_thres, out=None, check=True):
        d, i, c = out
        self.calls += 1
        d.fill_(float(self.rank) + 0.001 * self.calls); i.fill_(self.rank); c.fill_(self.calls % 300)
        return d, i, c


class _StandInPipe:
    def __init__(self, rank, B, depth):
        import contextlib
        from yolo_fastestv2_amd.sharded import packed_det_buffers
        self.depth, self.engines, self.streams = depth, [_StandInEngine(rank) for _ in range(depth)], [None] * depth
        self.buffers = [packed_det_buffers(B, "cpu") for _ in range(depth)]
        self._n = 0

        @contextlib.contextmanager
        def slot():
            j = self._n % depth
            self._n += 1
            yield j, self.engines[j], self.buffers[j]
        self.slot = slot


def launcher_selftest(a, rank, world):
    """The N > 1 control flow of main() - environment, process group, rotation over buffer sets, one asynchronous packed
    all-gather per step, host-side completion, the timed blocks, max-over-ranks, ONE line from rank 0 - on CPU tensors over gloo.
    Prints a line marked `selftest`; never a measurement."""
    import torch.distributed as dist
    import yolo_fastestv2_amd as yfv2
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if world > 1 or "MASTER_PORT" in os.environ:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    use_dist = dist.is_initialized()
    B = min(a.batch, 8)
    pipe = _StandInPipe(rank, B, max(1, a.pipeline))
    recv = [torch.empty(world * B * (300 * 7 + 1)) for _ in pipe.buffers] if use_dist else []
    works = [None] * pipe.depth
    x = torch.zeros(B, 3, 32, 32)

    def step():
        with pipe.slot() as (j, e, bufs):
            if works[j] is not None:
                works[j].wait_host(); works[j] = None
            d, i, c = e.detect(x, a.conf, a.iou, out=bufs)
            if use_dist:
                works[j] = yfv2.gather_detections(d, i, c, force=True, async_op=True, out=recv[j])

    def finish():
        for j, w in enumerate(works):
            if w is not None:
                w.wait(unpack=False); works[j] = None

    def barrier():
        if use_dist:
            dist.barrier()
    for _ in range(a.warmup):
        step()
    finish()
    dts = [timed(step, a.steps, lambda: None, barrier, finish) for _ in range(max(1, a.blocks))]
    t = torch.tensor(dts, dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        from yolo_fastestv2_amd.sharded import rank_views
        for j in range(pipe.depth):          # every rank holds every rank's last result of that slot, in rank order
            for r, (d, i, c) in enumerate(rank_views(recv[j], world, B)):
                assert int(i[0, 0]) == r and abs(float(d[0, 0, 0]) - r) < 0.5, (rank, j, r)
    dt = float(t.median())
    if rank == 0:
        print(json.dumps({"metric": "launcher self-test (CPU stand-in engine over gloo; NOT a measurement)", "selftest": True,
                          "value": round(world * B * a.steps / dt, 1), "unit": "stand-in images/s", "n_gpus": world, "steps": a.steps,
                          "warmup": a.warmup, "blocks": len(dts), "scaling": "weak", "data": "stand-in",
                          "launched_by": "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else "plain"}), flush=True)
    barrier()
    if use_dist:
        dist.destroy_process_group()


def main():
    a = parse()
    if a.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        self_launch(a)                      # does not return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        a.gpus = world                      # under a launcher the launcher's world size is the truth
    if a.launcher_selftest:
        return launcher_selftest(a, rank, world)
    import torch.distributed as dist
    import yolo_fastestv2_amd as yfv2
    from yolo_fastestv2_amd._lib import plan_from_env
    global PLAN
    PLAN = plan_from_env()

    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback exists)"
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    under_launcher = "RANK" in os.environ and "MASTER_PORT" in os.environ
    if world > 1 or under_launcher:  # under torch.distributed.run even N=1 goes through RCCL (exercises the N>1 code path)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    use_dist = dist.is_initialized()

    def barrier():
        if use_dist:
            dist.barrier()

    def sync():
        torch.cuda.synchronize(dev)

    # ---- model + data ---------------------------------------------------------------------
    if a.weights == "coco":
        import numpy as np
        z = np.load(os.path.join(REPO, "tests", "golden", "weights_coco.npz"))
        sd = {k: torch.from_numpy(z[k]) for k in z.files}
    else:
        sd = yfv2.random_state_dict(0)
    # Consecutive steps (batches) are independent: they rotate over a.pipeline handles (each with its own workspace) on as many
    # HIP streams (yolo_fastestv2_amd.DetectPipeline), so that a step's decode + NMS launch and the under-filled tail of every
    # launch (one workgroup per image, a last round of waves on a third of the SIMDs) overlap the neighbours' launches.
    # tools/pipeline_probe.py: 1 / 2 / 3 / 4 handles = 0.78-0.79 / 0.72-0.74 / 0.70-0.71 / 0.72-0.74 ms per step on one box.
    # `single_stream_img_s` reports the same steps on one handle and one stream.
    pipe = yfv2.DetectPipeline(dev, 352, 352, 80, 3, anchors=ANCHORS, max_batch=a.batch, depth=max(1, a.pipeline), plan=PLAN)
    pipe.load_state_dict(sd)
    eng, engs, streams = pipe.engines[0], pipe.engines, pipe.streams
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    # resident in HBM before timing.  SEVERAL distinct batches, rotated step by step: one 381 MB batch read again and again could sit in
    # the 256 MiB Infinity Cache (FETCH_SIZE counts L2 -> fabric requests, cache hits included); three of them cannot
    xs = [torch.rand(a.batch, 3, 352, 352, device=dev, generator=g) for _ in range(max(1, a.inputs))]
    x = xs[0]                                                       # (the single-input extras: profile pass, forward-only, fp32 plan)
    nx = [0]

    def next_x():
        nx[0] += 1
        return xs[nx[0] % len(xs)]
    det_bufs = pipe.buffers[0]
    logit_bufs = [torch.empty(s, device=dev) for s in eng.logit_shapes(a.batch)]
    side = torch.cuda.Stream(device=dev)      # the clock probe's stream

    # N > 1: a rank's padded detections (8.4 KB/image, one flat buffer) are all-gathered once per step on RCCL's own
    # stream, overlapped with the next step's kernels: two buffer sets, a set is reused only after its gather was waited for
    sets = pipe.buffers
    recv = [torch.empty(world * a.batch * (300 * 7 + 1), dtype=torch.float32, device=dev) for _ in sets] if use_dist else []
    works = [None] * len(sets)
    last = [None]        # (dets, idx, cnt) of the latest step: --dump-outputs

    def step():
        with pipe.slot() as (j, e, bufs):      # next handle in rotation, its stream current
            if works[j] is not None:
                works[j].wait_host()      # issued len(sets) steps ago; the gathered result stays packed in recv[j] (sharded.rank_views)
                works[j] = None
            d, i, c = e.detect(next_x(), a.conf, a.iou, out=bufs)     # (looks at the range guard first: Engine.detect check=True, a host memory read)
            last[0] = (d, i, c)
            if use_dist:
                works[j] = yfv2.gather_detections(d, i, c, force=True, async_op=True, out=recv[j])

    def step_single():
        eng.detect(next_x(), a.conf, a.iou, out=det_bufs)

    def finish():
        for j, w in enumerate(works):
            if w is not None:
                w.wait(unpack=False)
                works[j] = None

    def clock_busy(ms=25.0):
        """effective shader clock with every CU issuing dependent FMAs (two one-wave workgroups per CU), main stream"""
        eng.clock_probe_begin(2 * torch.cuda.get_device_properties(dev).multi_processor_count, ms, busy=True)
        return eng.clock_probe_end()

    def clock_during(fn, est_ms):
        """run fn() (which enqueues and may synchronise) while 16 sleeping probe waves sit on the side stream for ~est_ms: the
        clock the kernels of fn ran at.  The probe waves sleep between looks at the reference clock (no issue slots to speak of)."""
        sync()
        with torch.cuda.stream(side):
            eng.clock_probe_begin(16, max(0.2, est_ms), busy=False)
        r = fn()
        with torch.cuda.stream(side):
            c = eng.clock_probe_end()
        sync()
        return r, c

    for j in range(1, len(engs)):          # set-up, not a step: every extra handle's first call (lazy one-time initialisation)
        with torch.cuda.stream(streams[j]):
            engs[j].detect(x, a.conf, a.iou, out=sets[j])
    sync()
    props = torch.cuda.get_device_properties(dev)
    box = {"device": torch.cuda.get_device_name(dev), "cus": props.multi_processor_count}
    pci = None
    if getattr(props, "pci_bus_id", None) is not None:
        pci = "%04x:%02x:%02x" % (int(getattr(props, "pci_domain_id", 0)), int(props.pci_bus_id), int(getattr(props, "pci_device_id", 0)))
        box["pci"] = pci
    telemetry = a.full and rank == 0
    if telemetry:
        box.update(smi_snapshot(local, pci))
        box["sclk_cold"] = clock_busy()          # first look, before the device was held under load
    # SPIN-UP (set-up, not a step, not the warm-up): hold the device under load for --spinup-seconds of the same steps on one
    # handle (no collective: every rank decides by its own clock).  A fresh process runs its first steps 8-10 % slower than every
    # later one (round 3: 0.754 ms per step for the first 20 from a cold start, 0.68-0.70 for each following 20) - the device
    # leaving its idle power state - which would put a --warmup 5 --steps 20 run entirely inside the ramp.
    t_spin, n_spin = time.perf_counter(), 0
    while time.perf_counter() - t_spin < a.spinup_seconds:
        for _ in range(20):
            with pipe.slot() as (j, e, bufs):
                e.detect(next_x(), a.conf, a.iou, out=bufs)
        n_spin += 20
        if telemetry and "sysfs_under_pipelined_load" not in box and time.perf_counter() - t_spin > 0.6 * a.spinup_seconds:
            box["sysfs_under_pipelined_load"] = sysfs_power_clock(pci)     # the 20 steps just queued are still running
        sync()
    spin_s = time.perf_counter() - t_spin
    nx[0] = 0      # the warm-up and timed steps see the same inputs in every run, however many spin-up steps there were
    # (no probe between the spin-up and the timed blocks: the all-CU FMA kernel drains the pipeline, and the first timed block then
    # pays for refilling it - round 5's first form measured 368 k for block 1 against 385-392 k for blocks 2-5)
    # exactly W warm-up steps (with the collective), then the headline: ONE timed block of exactly K steps
    for _ in range(a.warmup):
        step()
    finish()
    sync()

    def slowest_rank(dts):
        if not dts:
            return []
        t = torch.tensor(dts, device=dev, dtype=torch.float64)
        if use_dist:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)       # per block: the slowest rank
        return [float(v) for v in t.cpu()]
    dt = slowest_rank([timed(step, a.steps, sync, barrier, finish)])[0]
    value = world * a.batch * a.steps / dt
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, *last[0])
    out = {"metric": "images/sec at 352x352 bs=256 per GPU (forward+decode+NMS)", "value": round(value, 1), "unit": "images/s",
           "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(1e3 * dt / a.steps, 4),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32 tensors; contractions fp16x3 (two-term fp16 split operands on v_mfma_f32_16x16x32_f16, fp32 accumulate); depthwise/BN/ReLU/decode/NMS fp32 VALU"
                    if FP16X3 else "f32 (fp32 MFMA contractions: YFV2_BF6=0 plan)",
           "data": "synthetic"}

    def close():
        barrier()
        if use_dist:
            dist.destroy_process_group()
    if not a.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        return close()

    # ---- --full: everything beyond the headline -------------------------------------------
    # --blocks back-to-back blocks of exactly K steps in all, the headline's first
    chrono = [dt] + slowest_rank([timed(step, a.steps, sync, barrier, finish) for _ in range(max(1, a.blocks) - 1)])
    dts = sorted(chrono)
    blocks = {"n": len(dts), "steps_each": a.steps, "img_s": [round(world * a.batch * a.steps / v, 1) for v in chrono],
              "img_s_min": round(world * a.batch * a.steps / dts[-1], 1), "img_s_max": round(world * a.batch * a.steps / dts[0], 1),
              "img_s_median": round(world * a.batch * a.steps / (dts[len(dts) // 2] if len(dts) % 2 else 0.5 * (dts[len(dts) // 2 - 1] + dts[len(dts) // 2])), 1),
              "value_is": "first block", "img_s_order": "chronological"}
    if rank == 0:
        box["sclk_after_timed"] = clock_busy()
        # the same kind of loop once more with the sleeping probe beside it: the clock the timed steps ran at
    def k_steps():
        for _ in range(a.steps):
            step()
        finish()
    if rank == 0:
        _, box["sclk_during_pipelined_steps"] = clock_during(k_steps, 0.85 * 1e3 * dt)
    else:
        k_steps()
    # the same K steps on one handle and one stream (no collective): what a caller that does not pipeline its batches gets
    for _ in range(2):
        step_single()
    dts_s = sorted(timed(step_single, a.steps, sync, barrier) for _ in range(max(1, a.blocks)))
    dt_s = dts_s[len(dts_s) // 2]
    if rank == 0:
        def k_single():
            for _ in range(a.steps):
                step_single()
        _, box["sclk_during_single_stream_steps"] = clock_during(k_single, 0.85 * 1e3 * dt_s)
        for i in range(1000):                # ~0.7 s of the one-stream loop; the hwmon sensor (a few hundred milliseconds of averaging) is
            step_single()                    # read while the device is 0.55 s into it and the host still enqueues
            if i == 800:
                box["sysfs_under_single_stream_load"] = sysfs_power_clock(pci)
        sync()

    # ONE call per batch on ONE handle whose calls cut the batch into two slices on internal streams (YFV2_LANES=2)
    eng_l = yfv2.Engine(dev, 352, 352, 80, 3, anchors=ANCHORS, max_batch=a.batch, plan=dict(PLAN, lanes=2))
    eng_l.load_state_dict(sd)
    for _ in range(3):
        eng_l.detect(x, a.conf, a.iou, out=det_bufs)
    dt_l = timed(lambda: eng_l.detect(x, a.conf, a.iou, out=det_bufs), a.steps, sync, barrier)
    del eng_l
    for _ in range(2):
        step_single()          # det_bufs again hold the one-handle result (detections_per_image below)

    # forward only (BASELINE.json configs[1]) - same batch, same buffers
    for _ in range(2):
        eng.forward(x, out=logit_bufs)
    dt_f = timed(lambda: eng.forward(x, out=logit_bufs), a.steps, sync, barrier)
    fwd_img_s = world * a.batch * a.steps / dt_f
    # ... and pipelined over the handles like `value`
    logit_sets = [logit_bufs] + [[torch.empty(s, device=dev) for s in eng.logit_shapes(a.batch)] for _ in engs[1:]]
    nf = [0]

    def fwd_step():
        j = nf[0] % len(engs)
        nf[0] += 1
        with torch.cuda.stream(streams[j]):
            engs[j].forward(x, out=logit_sets[j])
    for _ in range(2 * len(engs)):
        fwd_step()
    dt_fp = timed(fwd_step, a.steps, sync, barrier)
    del logit_sets[1:]
    # the same forward fed with uint8 (B,H,W,3) images (yfv2_forward_u8: test.py:34-38's pre-process inside the stem) -
    # an extra, never `value`: the contract's input is the fp32 tensor
    xu = (x.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    for _ in range(2):
        eng.forward(xu, out=logit_bufs)
    dt_u = timed(lambda: eng.forward(xu, out=logit_bufs), a.steps, sync, barrier)
    fwd_u8_img_s = world * a.batch * a.steps / dt_u
    del xu

    cnt_h = det_bufs[2].float().cpu()
    if rank == 0:
        # ---- roofline: per-launch hipEvent times grouped by kernel, the way a rocprofv3 --stats table groups them ----
        # Bytes are SURVEY.md 8(d)'s: a fused launch is charged its EXTERNAL reads + writes only (`yfv2_stage_info`'s third
        # figure: the chain of seven blocks = one read + one write of the activation); the per-layer figure of BASELINE.md
        # section 4 rides along as `per_layer_gbs` (how much traffic the fusion removed).  Counters (HBM bytes, MFMA busy)
        # cannot be read from inside the process: they come from the newest profiles/*_traffic.json / *_pmc.json whose
        # source fingerprint (tools/srchash.py) equals this tree's - else null.
        stages = eng.stages()
        # per-launch events on an otherwise EMPTY device.  (Round 5's first form kept the sleeping clock probe beside this pass: its 16
        # one-wave workgroups hold a few registers on 16 CUs, the stage-3 chain needs a CU's whole register file - 8 waves x 256
        # VGPRs - so 16 of its 256 workgroups waited for a second round and the launch read 119 us instead of 86.)  Cycles =
        # milliseconds x the clock measured beside the single-stream step loop above, the same launches in the same order.
        ms = eng.profile_forward(x, iters=a.profile_iters)
        sclk_prof = box["sclk_during_single_stream_steps"]["sclk_mhz_mean"]
        src_hash = source_hash()
        prof_t, prof_p = newest_profile("_traffic.json", src_hash), newest_profile("_pmc.json", src_hash)
        table = {}
        for st, m in zip(stages, ms):
            k = table.setdefault(st["kernel"], {"ms": 0.0, "launches": 0, "bytes": 0.0, "ext": 0.0, "flops": 0.0, "covers": []})
            k["ms"] += m; k["launches"] += 1
            k["bytes"] += st["bytes_per_image"] * a.batch; k["ext"] += st["external_bytes_per_image"] * a.batch
            k["flops"] += st["flops_per_image"] * a.batch
            k["covers"].append(st["name"].split(":")[0][:60])
        tot_ms = sum(k["ms"] for k in table.values())

        def row(name, k):
            sec = k["ms"] * 1e-3
            moved, tf = k["ext"] / sec / 1e9, k["flops"] / sec / 1e12
            ai = k["flops"] / k["ext"]
            traffic = profile_lookup(prof_t, name, "total_bytes", k["launches"])
            r = {"kernel": name, "launches": k["launches"], "ms": round(k["ms"], 4), "kcycles": round(k["ms"] * sclk_prof, 1), "share": round(k["ms"] / tot_ms, 4),
                 "external_bytes": k["ext"], "moved_gbs": round(moved, 1), "hbm_frac_external": round(moved / HBM_PEAK_GBS, 4),
                 "hbm_frac_of_achievable": round(moved / HBM_ACHIEVABLE_GBS, 4),
                 "per_layer_gbs": round(k["bytes"] / sec / 1e9, 1),
                 "tflops": round(tf, 2), "mfma_pipe_frac": round(PIPE_COST * tf / PIPE_PEAK_TF, 4),
                 "flop_per_external_byte": round(ai, 1), "bound": "mfma" if ai > RIDGE_FLOP_PER_BYTE else "hbm",
                 "mfma_busy": profile_lookup(prof_p, name, "mfma_busy_pct", 1, mean=True),
                 "traffic_bytes": traffic, "traffic_over_external": round(traffic / k["ext"], 3) if traffic else None}
            return r
        kernel_table = [row(name, k) for name, k in sorted(table.items(), key=lambda kv: -kv[1]["ms"])]
        dom_name, dom = max(table.items(), key=lambda kv: kv[1]["ms"])
        drow = kernel_table[0]
        # the bound quoted is the one the dominant kernel's arithmetic intensity (flops / external bytes) puts it under:
        # left of the fp32 ridge (157.3 TF / 8 TB/s = 19.7 flop/B) HBM, right of it the fp32 MFMA peak
        if drow["bound"] == "hbm":
            ach, peak, unit = drow["moved_gbs"], HBM_PEAK_GBS, "GB/s"
        else:     # matrix-pipe flops actually issued (3 per algorithmic flop on fp16x3) against that pipe's dense peak
            ach, peak, unit = round(PIPE_COST * drow["tflops"], 2), PIPE_PEAK_TF, "TFLOP/s"
        tot_ext = sum(k["ext"] for k in table.values()); tot_fl = sum(k["flops"] for k in table.values())
        roof = {"kernel": dom_name, "covers": dom["covers"], "launches_per_forward": dom["launches"], "bound": drow["bound"],
                "achieved": ach, "peak": peak, "unit": unit, "frac": round(ach / peak, 4),
                "traffic": (drow["traffic_bytes"] / dom["launches"]) if drow["traffic_bytes"] else None,
                "traffic_note": ("HBM bytes per launch by rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes, gfx950 x2 read correction): profiles/%s, same source fingerprint as this run" % prof_t["_file"])
                                if drow["traffic_bytes"] else "no profiles/*_traffic.json carries this tree's source fingerprint %s (PMC passes are separate runs: tools/gpu_traffic.sh)" % src_hash,
                "avg_launch_ms": round(dom["ms"] / dom["launches"], 4), "avg_launch_kcycles": round(dom["ms"] / dom["launches"] * sclk_prof, 1),
                "sclk_mhz_for_cycles": sclk_prof, "sum_ms_per_forward": round(dom["ms"], 4),
                "share_of_forward": round(dom["ms"] / tot_ms, 4),
                "algorithmic_bytes_per_launch": dom["ext"] / dom["launches"], "algorithmic_flops_per_launch": dom["flops"] / dom["launches"],
                "hbm_frac_external": drow["hbm_frac_external"], "hbm_frac_of_achievable": drow["hbm_frac_of_achievable"],
                "mfma_pipe_frac": drow["mfma_pipe_frac"],
                "mfma_pipe": ("f16 dense %.0f TFLOP/s, %g products per algorithmic MAC (fp16x3)" if FP16X3 else "fp32 dense %.1f TFLOP/s, %g product per MAC") % (PIPE_PEAK_TF, PIPE_COST),
                "mfma_busy": drow["mfma_busy"], "src_hash": src_hash,
                "whole_forward": {"external_gbs": round(tot_ext / (tot_ms * 1e-3) / 1e9, 1), "hbm_frac_external": round(tot_ext / (tot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                  "per_layer_gbs": round(sum(k["bytes"] for k in table.values()) / (tot_ms * 1e-3) / 1e9, 1),
                                  "hbm_frac_of_achievable": round(tot_ext / (tot_ms * 1e-3) / 1e9 / HBM_ACHIEVABLE_GBS, 4),
                                  "tflops": round(tot_fl / (tot_ms * 1e-3) / 1e12, 2),
                                  "mfma_pipe_frac": round(PIPE_COST * tot_fl / (tot_ms * 1e-3) / 1e12 / PIPE_PEAK_TF, 4)}}

        # ---- the literal-fp32 plan beside the headline: every contraction on v_mfma_f32_*_f32 (YFV2_BF6=0 at create time) - what the
        # reference's own arithmetic (fp32 convolutions, model/detector.py:21-47) costs on this box, same weights, same input, same run
        fp32 = None
        if world == 1 and FP16X3 and not a.no_extras:
            pipe32 = yfv2.DetectPipeline(dev, 352, 352, 80, 3, anchors=ANCHORS, max_batch=a.batch, depth=max(1, a.pipeline), plan=dict(PLAN, fp32_matrix=1))
            pipe32.load_state_dict(sd)

            def step32():
                with pipe32.slot() as (_, e, bufs):
                    e.detect(x, a.conf, a.iou, out=bufs)

            def single32():
                pipe32.engines[0].detect(x, a.conf, a.iou, out=pipe32.buffers[0])
            for _ in range(3 * pipe32.depth):
                step32()
            d32 = sorted(timed(step32, a.steps, sync, barrier) for _ in range(3))[1]
            for _ in range(2):
                single32()
            d32s = sorted(timed(single32, a.steps, sync, barrier) for _ in range(3))[1]
            for _ in range(2):
                pipe32.engines[0].forward(x, out=logit_bufs)
            d32f = timed(lambda: pipe32.engines[0].forward(x, out=logit_bufs), a.steps, sync, barrier)
            fp32 = {"img_s": round(a.batch * a.steps / d32, 1), "ms_per_step": round(1e3 * d32 / a.steps, 4),
                    "single_stream_img_s": round(a.batch * a.steps / d32s, 1), "single_stream_ms_per_step": round(1e3 * d32s / a.steps, 4),
                    "forward_only_ms": round(1e3 * d32f / a.steps, 4), "headline_over_fp32_plan": round(d32 / dt, 3),
                    "note": "YFV2_BF6=0: stem, stage 2, stage 4.0 and the towers on rounds 1-2's fp32-MFMA kernels, the chains and FPN reduces with fp32 MFMAs; "
                            "same steps, same pipelining, median of three blocks"}
            del pipe32

        # ---- BASELINE configs[2] as the survey specifies it: COCO weights, JPEG-derived batch, both threshold pairs ----
        coco = None
        gold = os.path.join(REPO, "tests", "golden")
        if world == 1 and not a.no_extras and os.path.exists(os.path.join(gold, "weights_coco.npz")):
            import numpy as np
            z = np.load(os.path.join(gold, "weights_coco.npz"))
            eng_c = yfv2.Engine(dev, 352, 352, 80, 3, anchors=ANCHORS, max_batch=a.batch)
            eng_c.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files})
            xc3 = batch_from_reference_images(np.load(os.path.join(gold, "images_u8.npz"))["images"], a.batch, seed=3).to(dev)
            coco = {"weights": "coco2017-0.241078ap-model.pth (tests/golden/weights_coco.npz)",
                    "input": "%d images derived from the 6 shipped JPEGs (flip / roll / gain variants, seed 3)" % a.batch}
            pipe.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files})     # the pipeline's handles, COCO weights from here on
            for tag, ct in (("conf0.30_iou0.40", 0.3), ("conf0.01_iou0.40", 0.01)):
                for _ in range(2):
                    eng_c.detect(xc3, ct, 0.4, out=det_bufs)
                dt_c = timed(lambda: eng_c.detect(xc3, ct, 0.4, out=det_bufs), a.steps, sync, barrier)
                cc = det_bufs[2].float().cpu()

                def coco_step():
                    with pipe.slot() as (_, e, bufs):
                        e.detect(xc3, ct, 0.4, out=bufs)
                for _ in range(2 * pipe.depth):
                    coco_step()
                dt_cp = timed(coco_step, a.steps, sync, barrier)
                coco[tag] = {"img_s": round(a.batch * a.steps / dt_cp, 1), "ms_per_step": round(1e3 * dt_cp / a.steps, 4),
                             "single_stream_img_s": round(a.batch * a.steps / dt_c, 1), "single_stream_ms_per_step": round(1e3 * dt_c / a.steps, 4),
                             "detections_per_image_mean": round(float(cc.mean()), 2), "detections_per_image_max": int(cc.max())}
            del eng_c, xc3

        # ---- CPU baseline: the oracle on this box's host cores, bounded sample ------------
        cpu = None
        if world == 1 and not a.no_cpu_baseline:
            from oracle import yfv2_oracle as oracle
            # the reference's CPU path is ATen/oneDNN on all host cores; on a 256-thread
            # box that oversubscribes these tiny convs badly, so probe a few thread counts
            # on a small batch and time the bounded sample with the fastest one
            ncores = os.cpu_count() or 1
            try:
                ncores = min(ncores, len(os.sched_getaffinity(0)))
            except AttributeError:
                pass
            bs = 64
            xc = x[:bs].cpu()
            cands = sorted({c for c in (8, 16, 32, 64, 128, ncores) if c <= ncores})
            best_t, best_rate = cands[0], 0.0
            for c in cands:
                torch.set_num_threads(c)
                oracle.forward(sd, xc[:4])  # warm-up at this thread count
                t0 = time.perf_counter()
                oracle.detect(sd, xc[:16], ANCHORS, 352, a.conf, a.iou)
                el = time.perf_counter() - t0
                if 16 / el > best_rate:
                    best_t, best_rate = c, 16 / el
                if el > 4.0:
                    break  # larger counts only get slower from here
            torch.set_num_threads(best_t)
            n_img, t0 = 0, time.perf_counter()
            while True:
                oracle.detect(sd, xc, ANCHORS, 352, a.conf, a.iou)
                n_img += bs
                el = time.perf_counter() - t0
                if el >= a.cpu_seconds or n_img >= 8192:
                    break
            # ... and what the HOST as a whole does with this path: floor(host threads / N) such instances at once, each in its own
            # process (the reference's CPU path has no batch-level parallelism of its own; a user with a queue of batches would
            # run several).  Bounded like the single instance; a stated baseline, never the target.
            many = None
            n_inst = min(max(1, ncores // best_t), 32)
            if n_inst > 1:
                try:
                    import concurrent.futures as cf
                    import multiprocessing as mp
                    with cf.ProcessPoolExecutor(max_workers=n_inst, mp_context=mp.get_context("spawn")) as ex:
                        res = list(ex.map(_cpu_instance, [(best_t, min(a.cpu_seconds, 10.0), 32, a.conf, a.iou, 77 + k) for k in range(n_inst)]))
                    many = {"instances": n_inst, "threads_each": best_t, "images_s_sum": round(sum(n / t for n, t in res), 1),
                            "images_s_per_instance": [round(n / t, 1) for n, t in res]}
                except Exception as e:      # noqa: BLE001 - a baseline, best effort
                    many = {"error": repr(e)[:200]}
            cpu = {"value": round(n_img / el, 1), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
                   "host_threads_available": ncores,
                   "what": "ONE %d-thread instance of the CPU oracle (of the %d host threads this process may use)" % (best_t, ncores),
                   "concurrent_instances": many,
                   "sample": "ONE %d-thread instance: %d synthetic images in batches of %d through oracle forward(ATen CPU)+decode+NMS, %.1f s, "
                             "thread count chosen by a 16-image probe over %s (more threads per instance only get slower: these convs are tiny); "
                             "`concurrent_instances` = floor(host threads / %d) such instances at once, one process each, rates summed; "
                             "kind 'port' because /root/reference does not exist on "
                             "the GPU box - the oracle runs the same ATen CPU ops and is bit-identical to the reference's own modules "
                             "where both exist (asserted by tests/golden/make_golden.py)" % (best_t, n_img, bs, el, cands, best_t)}

        # ---- BASELINE configs[4]: one train.py iteration at batch 64 - train-mode forward, compute_loss,
        # backward to all 225 parameters, SGD - through the drop-in surface; an extra, never `value`
        train = None
        if world == 1 and not a.no_extras:
            import numpy as np
            cfg_t = {"anchor_num": 3, "classes": 80, "width": 352, "height": 352, "anchors": ANCHORS}
            model = yfv2.Detector(80, 3, True).to(dev)
            model.load_state_dict(yfv2.random_state_dict(1))
            model.train()
            opt = yfv2.SGD(params=model.parameters(), lr=1e-3, momentum=0.949, weight_decay=0.0005)
            Bt = 64
            rng = np.random.default_rng(Bt)
            xt = torch.from_numpy(rng.random((Bt, 3, 352, 352), dtype=np.float32)).to(dev)
            tg = np.zeros((4 * Bt, 6), np.float32)
            tg[:, 0] = rng.integers(0, Bt, 4 * Bt); tg[:, 1] = rng.integers(0, 80, 4 * Bt)
            tg[:, 2:4] = rng.random((4 * Bt, 2)) * 0.9 + 0.05; tg[:, 4:6] = rng.random((4 * Bt, 2)) * 0.5 + 0.03
            tgt = torch.from_numpy(tg).to(dev)

            def train_step():
                loss = yfv2.compute_loss(model(xt), tgt, cfg_t, dev)[3]
                loss.backward(); opt.step(); opt.zero_grad()
            for _ in range(3):
                train_step()
            dt_t = timed(train_step, 10, sync, barrier)
            fl = 3.0 * 212764464.0 * Bt          # forward + data gradients + weight gradients: 3 x SURVEY.md 8(d)'s 212.8 MFLOP per image
            train = {"batch": Bt, "ms_per_iteration": round(1e3 * dt_t / 10, 3), "img_s": round(Bt * 10 / dt_t, 1),
                     "algorithmic_tflops": round(fl / (dt_t / 10) / 1e12, 2), "frac_of_fp32_mfma_peak": round(fl / (dt_t / 10) / 1e12 / MFMA_F32_PEAK_TF, 4),
                     "note": "train.py:96-123 on the device (Detector.train(), compute_loss, backward, yfv2.SGD), fp32 MFMA for the pointwise convs; "
                             "launch- and pass-count bound (about 900 kernels per iteration: DESIGN.md 4.3), not a throughput path"}
            del model, opt, xt

        out.update({
            "single_stream_img_s": round(a.batch * a.steps / dt_s, 1),
            "arithmetic": "fp32 tensors, fp32 accumulation everywhere.  Depthwise convs, BatchNorm, ReLU, max-pool, decode: fp32 VALU.  Every "
                          "convolution with a channel contraction - stem (fp32 input), stage 2, stage3.0, the stage-3 chain, stage4.0, the stage-4 chain, "
                          "the FPN reduces, the towers and the output convs - is fp16x3: both operands split into two fp16 terms whose sum "
                          "reproduces them to 2^-24 (filters on the host, scaled by a power of two; activations scaled by 2^4 / 2^8), the three products "
                          "w1 x2 + w2 x1 + w1 x1 (each exact) accumulated in fp32 by v_mfma_f32_16x16x32_f16, the powers of two undone exactly; error vs "
                          "float64 within 2x of a plain fp32 convolution's (tests/test_stem16_host_model.py), valid for |activation| < 4094 (|pixel| < "
                          "255.9; guarded: yfv2_nonfinite).  The uint8 stem is fp16x2 (a pixel 0..255 is one exact fp16 term); the YFV2_BF6=0 plan runs the fp32 MFMA "
                          "(timed beside the headline in fp32_mfma_plan).  Every parity test (logits 1e-4, scores 1e-5, identical NMS survivors) runs on this arithmetic.",
            "config": {"workload": "batch %d/GPU synthetic 352x352x3 fp32 (torch.rand), seeded random-init weights, "
                                   "Detector forward + anchor decode + class-aware NMS(conf %.2f, iou %.2f; 300 detections/image = NMS worst case)%s; "
                                   "`value` keeps UP TO %d BATCHES OF %d IN FLIGHT (consecutive steps rotate over %d handles / HIP streams, every step complete inside its timed block); "
                                   "the strict one-batch-at-a-time rate is single_stream_img_s.  "
                                   "BASELINE.json configs[1] (forward only) is the subset reported in forward_only_img_s, configs[2] "
                                   "(COCO weights, JPEG-derived batch) in coco_e2e"
                                   % (a.batch, a.conf, a.iou, " + one RCCL all-gather of the padded detections per step, overlapped with the next step" if use_dist else "",
                                      len(engs), a.batch, len(engs)),
                       "global_batch": world * a.batch, "batches_in_flight": len(engs), "single_stream_img_s": round(a.batch * a.steps / dt_s, 1),
                       "weights": a.weights + (" (yfv2.random_state_dict(0))" if a.weights == "random" else ""), "parallelism": "batch-sharded x%d" % world,
                       "distinct_input_batches": len(xs)},
            "blocks": blocks,
            "spinup": {"seconds": round(spin_s, 2), "steps": n_spin, "why": "set-up, before the W warm-up steps: the device is held under load until it has left its idle power state"},
            "box": box,
            "pipelining": "consecutive steps rotate over %d handles (own workspaces) on as many HIP streams; all K steps of a block complete inside its timed region" % len(engs),
            "forward_only_pipelined_img_s": round(world * a.batch * a.steps / dt_fp, 1), "forward_only_pipelined_ms": round(1e3 * dt_fp / a.steps, 4),
            "single_stream_ms_per_step": round(1e3 * dt_s / a.steps, 4),
            "single_call_two_lanes_img_s": round(a.batch * a.steps / dt_l, 1), "single_call_two_lanes_ms_per_step": round(1e3 * dt_l / a.steps, 4),
            "forward_only_img_s": round(fwd_img_s, 1), "forward_only_ms": round(1e3 * dt_f / a.steps, 4),
            "forward_only_note": "BASELINE.json configs[1] names `random-init weights`; timed here: yfv2.random_state_dict(0) (He-style seeded init of every tensor, "
                                 "the same shapes) - NOT the literal Detector(80, 3, load_param=False), which loads model/backbone/backbone.pth for the backbone "
                                 "(/root/reference/model/backbone/shufflenetv2.py:111-114; that file is not in this repository).  Speed does not depend on the values.",
            "forward_from_uint8_hwc_img_s": round(fwd_u8_img_s, 1), "forward_from_uint8_hwc_ms": round(1e3 * dt_u / a.steps, 4),
            "fp32_mfma_plan": fp32,
            "roofline": roof, "cpu_baseline": cpu,
            "detections_per_image": {"mean": round(float(cnt_h.mean()), 1), "max": int(cnt_h.max())},
            "forward_launches": len(stages), "forward_sum_of_launch_ms": round(tot_ms, 4), "kernel_table": kernel_table,
            "coco_e2e": coco, "train_iteration": train,
        })
        print(json.dumps(out), flush=True)
    close()


if __name__ == "__main__":
    main()
