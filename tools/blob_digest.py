"""Digest of everything the host packs, per configuration and plan - on the CPU, no device is opened.

For each entry of the matrix below: the dry run (yfv2_debug_plan_dryrun_ex) gives the launch count and the blob size; then
every step of the image view (yfv2_debug_plan_image_ex, step -1 = their number) and every job of a multi-job step
(step + 1000 * (job + 1)) is fetched with cap = the blob's size, i.e. from the image's start to the END of the blob, and
each launch name + returned slice goes into one sha256.  One line per entry: steps, blob floats, digest.

Two builds pack the same bits iff they print the same lines (YFV2_LIB=path selects the other build): the check a change
of the host packer has to pass.  The last line is the best of five wall times of the dry run at 80 classes, 352x352,
default plan; `--no-time` leaves it out (it is the one line that differs between two runs).

    python tools/blob_digest.py [--no-time] > digests.txt
"""
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import yolo_fastestv2_amd as yfv2  # noqa: E402
from oracle import yfv2_oracle as oracle  # noqa: E402
from yolo_fastestv2_amd import _lib  # noqa: E402
from yolo_fastestv2_amd._lib import Config, TensorDesc  # noqa: E402

CLASSES = (80, 20, 1, 100, 255)
SIZES = ((352, 352), (320, 320), (64, 96), (512, 512), (96, 1024))
PLANS = ("default", "fp32_matrix", "layer_by_layer", "front_two_launches", "towers_unpaired")


def descs(w):
    host = {k: v.float().contiguous() for k, v in w.items() if v.is_floating_point()}
    arr = (TensorDesc * len(host))()
    for i, (k, t) in enumerate(host.items()):
        arr[i].name, arr[i].data, arr[i].numel = k.encode(), t.data_ptr(), t.numel()
    return host, arr


def dryrun(cfg, plan, host, arr):
    ns, nb = C.c_int32(0), C.c_int64(0)
    rc = _lib.lib().yfv2_debug_plan_dryrun_ex(C.byref(cfg), C.byref(plan), arr, len(host), C.byref(ns), C.byref(nb))
    assert rc == 0, (rc, _lib.last_error())
    return ns.value, nb.value


def digest(w, classes, H, W, plan_name):
    host, arr = descs(w)
    cfg = Config()
    cfg.classes, cfg.anchor_num, cfg.height, cfg.width, cfg.max_batch, cfg.device = classes, 3, H, W, 4, 0
    plan = _lib.make_plan({} if plan_name == "default" else {plan_name: 1})
    L = _lib.lib()
    steps, blob = dryrun(cfg, plan, host, arr)
    buf = np.zeros(blob, np.float32)
    name = C.create_string_buffer(256)

    def image(step):
        return L.yfv2_debug_plan_image_ex(C.byref(cfg), C.byref(plan), arr, len(host), step, name, 256, buf.ctypes.data_as(C.c_void_p), blob)

    sha = hashlib.sha256()
    n_view = L.yfv2_debug_plan_image_ex(C.byref(cfg), C.byref(plan), arr, len(host), -1, None, 0, None, 0)
    assert steps <= n_view <= steps + 1, (steps, n_view)
    for st in range(n_view):
        job = 0
        n = image(st)
        assert n >= 0, (st, n)
        while n >= 0:                       # the step itself, then its jobs until "job out of range"
            sha.update(name.value)
            sha.update(buf[:n].tobytes())
            job += 1
            n = image(st + 1000 * job)
    return steps, blob, sha.hexdigest()


def main():
    for classes in CLASSES:
        w = yfv2.random_state_dict(1, classes=classes)
        for H, W in SIZES:
            for plan_name in PLANS:
                print("random classes=%d %dx%d %s: steps=%d blob=%d sha256=%s" % ((classes, H, W, plan_name) + digest(w, classes, H, W, plan_name)), flush=True)
    gold = os.path.join(REPO, "tests", "golden")
    w = oracle.load_weights(os.path.join(gold, "weights_coco.npz"))
    classes = int(np.load(os.path.join(gold, "cfg_coco.npz"))["classes"])
    for plan_name in PLANS[:3]:
        print("coco classes=%d 352x352 %s: steps=%d blob=%d sha256=%s" % ((classes, plan_name) + digest(w, classes, 352, 352, plan_name)), flush=True)
    if "--no-time" not in sys.argv[1:]:
        host, arr = descs(yfv2.random_state_dict(1, classes=80))
        cfg = Config()
        cfg.classes, cfg.anchor_num, cfg.height, cfg.width, cfg.max_batch, cfg.device = 80, 3, 352, 352, 4, 0
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            dryrun(cfg, _lib.make_plan({}), host, arr)
            times.append(time.perf_counter() - t0)
        print("dry run, 80 classes 352x352 default plan, five runs (ms): %s best %.2f" % (" ".join("%.2f" % (1e3 * t) for t in times), 1e3 * min(times)))


if __name__ == "__main__":
    main()
