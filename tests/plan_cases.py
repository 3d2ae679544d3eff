"""The shapes every alternative plan (include/yfv2.h yfv2_plan) is pinned at: ONE table, as data, read by the CPU coverage test
(tests/test_plan_cases_host.py), the GPU test (tests/test_gpu_plans.py) and its driver (tests/gpu_cases/plan_shapes.py).

A plan switch changes which kernels compute the path.  Which launches a (plan, classes, H, W) gets is decided on the host
(PlanBuilder), so the host-only dry run (yfv2_debug_plan_image_ex) names them without a device: `launch_sequence` below is that
list with the HxW figures removed - two configurations with the same sequence run the same kernels in the same order, at other
geometry.  The table holds at least one case per sequence that occurs over SIZES x CLASS_COUNTS; the CPU test fails when a
change of a static bound creates a sequence no case has.

No device is touched here: importing this module needs neither a GPU nor the native library (the dry run loads it lazily)."""
import collections
import re

Case = collections.namedtuple("Case", "kind plan H W classes B weight_seed image_seed")

# the lists the sequences are counted over (every size the default plan is tested at, every class tier)
SIZES = ((352, 352), (320, 320), (288, 384), (96, 384), (32, 32), (64, 96), (128, 64), (64, 128), (96, 160), (352, 32), (32, 512), (416, 416),
         (384, 384), (512, 512), (640, 384), (96, 1024))
CLASS_COUNTS = (1, 5, 15, 16, 80, 93, 94, 100, 255)

FP32 = {"fp32_matrix": 1}
LBL = {"layer_by_layer": 1}
LBL_FP32 = {"layer_by_layer": 1, "fp32_matrix": 1}
UNPAIRED = {"towers_unpaired": 1}
POST2 = {"post_two_launches": 1}
COVERED_PLANS = (FP32, LBL, LBL_FP32)        # every sequence over SIZES x CLASS_COUNTS has a case
WEIGHT_SEED = 7                              # with image seed H + W every image keeps a detection at conf 0.01 (checked on the CPU oracle)


def _fwd(plan, H, W, classes, B=3):
    return Case("forward", plan, H, W, classes, B, WEIGHT_SEED, H + W)


def _batch(plan, H, W, classes, B):
    return Case("batch", plan, H, W, classes, B, WEIGHT_SEED, H + W)


def _post(H, W, classes):
    return Case("post", POST2, H, W, classes, 3, WEIGHT_SEED, H + W)


CASES = (
    # ---- fp32_matrix: the smallest member of each size class, the <= 93-class cases spread over the head-tile forms of
    # tower2_kernel (0 / 1 / 6 tiles) at <= 128 pixels and above, then the three size families at 94 / 100 / 255 classes
    _fwd(FP32, 32, 32, 1),
    _fwd(FP32, 32, 32, 16),
    _fwd(FP32, 64, 128, 5),       # the smallest shape s1px_kernel accepts: 8x16 stage-2 map, one strip, R = 2, the fifth band empty
    _fwd(FP32, 96, 160, 15),      # a 20-column map: two strips
    _fwd(FP32, 96, 384, 80),
    _fwd(FP32, 96, 384, 16),
    _fwd(FP32, 352, 32, 93),
    _fwd(FP32, 32, 512, 5),
    _fwd(FP32, 96, 1024, 16),
    _fwd(FP32, 320, 320, 80),
    _fwd(FP32, 320, 320, 15),
    _fwd(FP32, 384, 384, 1),
    _fwd(FP32, 384, 384, 93),
    _fwd(FP32, 416, 416, 80),
    _fwd(FP32, 416, 416, 5),
    _fwd(FP32, 32, 32, 94),       # class heads in slices (94: two, 100: two with a remainder tile, 255: three) x the three size families
    _fwd(FP32, 352, 32, 100),
    _fwd(FP32, 32, 32, 255),
    _fwd(FP32, 96, 384, 94),
    _fwd(FP32, 64, 128, 100),
    _fwd(FP32, 320, 320, 100),
    _fwd(FP32, 96, 1024, 255),
    _fwd(FP32, 384, 384, 94),
    _fwd(FP32, 416, 416, 100),
    _fwd(FP32, 384, 384, 255),
    _fwd(FP32, 512, 512, 100),    # the README's own example of the remedy for a tripped range guard
    # ---- layer_by_layer: every size class once, every class tier once, each tier at another size
    _fwd(LBL, 32, 32, 5),
    _fwd(LBL, 64, 128, 94),
    _fwd(LBL, 96, 384, 100),
    _fwd(LBL, 352, 32, 255),
    _fwd(LBL, 32, 512, 80),
    _fwd(LBL, 96, 1024, 16),
    _fwd(LBL, 320, 320, 93),
    _fwd(LBL, 384, 384, 15),
    _fwd(LBL, 416, 416, 80),
    # ---- layer_by_layer on the fp32 matrix instructions: the same, tiers at other sizes
    _fwd(LBL_FP32, 32, 32, 255),
    _fwd(LBL_FP32, 64, 128, 1),
    _fwd(LBL_FP32, 96, 384, 16),
    _fwd(LBL_FP32, 352, 32, 94),
    _fwd(LBL_FP32, 32, 512, 100),
    _fwd(LBL_FP32, 96, 1024, 80),
    _fwd(LBL_FP32, 320, 320, 15),
    _fwd(LBL_FP32, 384, 384, 93),
    _fwd(LBL_FP32, 416, 416, 5),
    # ---- towers_unpaired: the configurations whose sequence differs from the default plan's
    _fwd(UNPAIRED, 320, 320, 80),
    _fwd(UNPAIRED, 352, 32, 80),
    _fwd(UNPAIRED, 288, 384, 80),
    _fwd(UNPAIRED, 416, 416, 80),
    _fwd(UNPAIRED, 384, 384, 80),
    _fwd(UNPAIRED, 32, 512, 80),
    _fwd(UNPAIRED, 352, 352, 5),  # the one-tile head
    # ---- batches beyond the grid clamps: 256 workgroups (block_s2w / block_s1pool / block_s2) and, layer by layer, dw_kernel's 4096
    _batch(FP32, 32, 32, 5, 261),
    _batch(FP32, 64, 128, 5, 261),
    _batch(LBL, 32, 32, 5, 261),
    _batch(LBL, 64, 128, 5, 261),
    _batch(LBL_FP32, 32, 32, 5, 261),
    _batch(LBL_FP32, 64, 128, 5, 261),
    _batch(LBL, 352, 352, 80, 96),   # stage 2's depthwise: 11 616 work items per image
    # ---- decode + NMS as two launches against the fused launch of a default-plan handle (<= 96 classes, <= 2048 rows)
    _post(64, 128, 5),
    _post(352, 32, 80),
    _post(96, 384, 16),
    _post(320, 320, 93),
)


def plan_name(plan):
    return "+".join(sorted(k for k, v in plan.items() if v)) or "default"


def case_id(c):
    return "%s%s-%dx%d-c%d-b%d" % ("" if c.kind == "forward" else c.kind + "-", plan_name(c.plan), c.H, c.W, c.classes, c.B)


def strip_geometry(name):
    """a launch name without its HxW figures"""
    return re.sub(r"\d+x\d+", "", name)


_WEIGHTS = {}


def _tensor_descs(classes):
    """(ctypes array of yfv2_tensor_desc, the tensors that back it) for a random state_dict of `classes` classes; the dry run reads shapes
    and packs values, which launches it plans does not depend on the values"""
    if classes not in _WEIGHTS:
        import yolo_fastestv2_amd as yfv2
        from yolo_fastestv2_amd._lib import TensorDesc
        w = yfv2.random_state_dict(WEIGHT_SEED, classes=classes)
        host = {k: v.float().contiguous() for k, v in w.items() if v.is_floating_point()}
        arr = (TensorDesc * len(host))()
        for i, (k, t) in enumerate(host.items()):
            arr[i].name, arr[i].data, arr[i].numel = k.encode(), t.data_ptr(), t.numel()
        _WEIGHTS[classes] = (arr, host)
    return _WEIGHTS[classes]


def dry_run(plan, classes, H, W):
    """(rc, names of the IMAGE VIEW's steps) of the host-only dry run (include/yfv2.h yfv2_debug_plan_image_ex): where the front is
    fused the view has one more step than the handle has launches (the stem's image and stage2.0's, one launch)"""
    import ctypes as C

    from yolo_fastestv2_amd import _lib
    arr, host = _tensor_descs(classes)
    cfg = _lib.Config()
    cfg.classes, cfg.anchor_num, cfg.height, cfg.width, cfg.max_batch, cfg.device = classes, 3, H, W, 1, 0
    L = _lib.lib()
    p = _lib.make_plan(plan)
    ns, nb = C.c_int32(0), C.c_int64(0)
    rc = L.yfv2_debug_plan_dryrun_ex(C.byref(cfg), C.byref(p), arr, len(host), C.byref(ns), C.byref(nb))
    if rc != 0:
        return rc, []
    n = L.yfv2_debug_plan_image_ex(C.byref(cfg), C.byref(p), arr, len(host), -1, None, 0, None, 0)
    if n < 0:
        return int(n), []
    name = C.create_string_buffer(256)
    buf = (C.c_float * 4)()
    names = []
    for st in range(n):
        got = L.yfv2_debug_plan_image_ex(C.byref(cfg), C.byref(p), arr, len(host), st, name, 256, buf, 4)
        if got < 0:
            return int(got), names
        names.append(name.value.decode())
    return 0, names


_SEQUENCES = {}


def launch_sequence(plan, classes, H, W):
    key = (plan_name(plan), classes, H, W)
    if key not in _SEQUENCES:
        rc, names = dry_run(plan, classes, H, W)
        assert rc == 0, "dry run of %s at %dx%d, %d classes: rc %d" % (plan_name(plan), H, W, classes, rc)
        _SEQUENCES[key] = tuple(strip_geometry(n) for n in names)
    return _SEQUENCES[key]


def launch_sequences(configs):
    """launch_sequence of every (plan, classes, H, W) of `configs`, in order.  A dry run re-packs the weights for every name it is asked
    for; the calls share no state and ctypes releases the interpreter lock, so the configurations run on a few threads."""
    import concurrent.futures
    configs = list(configs)
    for nc in sorted({c[1] for c in configs}):
        _tensor_descs(nc)
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda c: launch_sequence(*c), configs))


def sequences_over_lists(plan):
    """{sequence: [(H, W, classes), ...]} over SIZES x CLASS_COUNTS"""
    cfgs = [(hw[0], hw[1], nc) for hw in SIZES for nc in CLASS_COUNTS]
    out = collections.OrderedDict()
    for c, s in zip(cfgs, launch_sequences((plan, c[2], c[0], c[1]) for c in cfgs)):
        out.setdefault(s, []).append(c)
    return out


def sequence_table():
    """the rows of DESIGN.md's table: (plan, distinct launch sequences over SIZES x CLASS_COUNTS, of them different from the
    default plan's at the same configuration, forward cases in CASES)"""
    default = {c: s for s, cs in sequences_over_lists({}).items() for c in cs}
    rows = []
    for plan in COVERED_PLANS + (UNPAIRED,):
        seqs = sequences_over_lists(plan)
        differing = sum(1 for s, cs in seqs.items() if any(default[c] != s for c in cs))
        rows.append((plan_name(plan), len(seqs), differing, sum(1 for c in CASES if c.kind == "forward" and c.plan == plan)))
    return rows


if __name__ == "__main__":      # DESIGN.md's table (section 4.2), regenerated
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("| plan | distinct launch sequences | differing from the default plan's | forward cases |\n|---|---|---|---|")
    for r in sequence_table():
        print("| `%s` | %d | %d | %d |" % r)
