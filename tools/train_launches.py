#!/usr/bin/env python3
"""The ordered kernel launches of ONE training iteration, for comparing two builds of the library (profiles/train_host_launches.txt).

  python tools/train_launches.py
      builds the detector on seeded weights and runs exactly one train-mode forward, compute_loss, backward and SGD.step at
      352x352 - for B = 2 with 20 classes (tests/golden/make_golden.py TRAIN_CASES[1]) and for B = 64 with 80 classes (bench.py's
      training batch; the two take different branches of pw_weight_grad's segment choice) - then exits.  Meant to run under
          rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/train_launches.py
      once per build (YFV2_LIB=path/to/the/other/libyfv2.so selects the other one), with no other tracing.

  python tools/train_launches.py --compare A_kernel_trace.csv B_kernel_trace.csv
      the two traces as ordered lists of (kernel name, grid, workgroup size): their lengths, the launches per kernel name, and
      every position at which they differ.  The device-side fill that a hipMemsetAsync becomes is listed apart: the two scratch
      memsets are sized by the build and may differ.  Exit status 1 if anything else differs."""
import argparse
import collections
import csv
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))


def one_iteration(yfv2, torch, np, dev, classes, weights, x, targets, anchors):
    cfg = {"anchor_num": 3, "classes": classes, "width": 352, "height": 352, "anchors": anchors}
    model = yfv2.Detector(classes, 3, True).to(dev)
    model.load_state_dict(weights)
    model.train()
    opt = yfv2.SGD(params=model.parameters(), lr=1e-3, momentum=0.949, weight_decay=0.0005)
    loss = yfv2.compute_loss(model(torch.from_numpy(x).to(dev)), torch.from_numpy(targets).to(dev), cfg, dev)[3]
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return float(loss.detach())


def run():
    import numpy as np
    import torch
    import make_golden
    import yolo_fastestv2_amd as yfv2
    dev = torch.device("cuda:0")
    anchors = [float(a) for a in np.load(os.path.join(REPO, "tests", "golden", "cfg_coco.npz"))["anchors"]]
    classes, B, T, seed, _ = make_golden.TRAIN_CASES[1]
    w, x, t = make_golden.train_case_inputs(classes, B, T, seed)
    print("B=%d classes=%d loss=%.6f" % (B, classes, one_iteration(yfv2, torch, np, dev, classes, w, x, t, anchors)))
    B = 64                                                     # bench.py's training batch, built the way bench.py builds it
    rng = np.random.default_rng(B)
    x = rng.random((B, 3, 352, 352), dtype=np.float32)
    t = np.zeros((4 * B, 6), np.float32)
    t[:, 0] = rng.integers(0, B, 4 * B); t[:, 1] = rng.integers(0, 80, 4 * B)
    t[:, 2:4] = rng.random((4 * B, 2)) * 0.9 + 0.05; t[:, 4:6] = rng.random((4 * B, 2)) * 0.5 + 0.03
    print("B=%d classes=%d loss=%.6f" % (B, 80, one_iteration(yfv2, torch, np, dev, 80, yfv2.random_state_dict(1), x, t, anchors)))


def launches(path):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ")) for r in rows]


def is_fill(name):
    return "fillBuffer" in name


def compare(path_a, path_b):
    a, b = launches(path_a), launches(path_b)
    ka, kb = [l for l in a if not is_fill(l[0])], [l for l in b if not is_fill(l[0])]
    fa, fb = [l for l in a if is_fill(l[0])], [l for l in b if is_fill(l[0])]
    print("A: %s\nB: %s" % (path_a, path_b))
    print("launches: A %d, B %d (of them device fills of a memset: A %d, B %d)" % (len(a), len(b), len(fa), len(fb)))
    differ = [(i, p, q) for i, (p, q) in enumerate(zip(ka, kb)) if p != q]
    print("kernels other than fills, in order, as (name, grid, workgroup): A %d, B %d, positions that differ: %d" % (len(ka), len(kb), len(differ)))
    for i, p, q in differ[:40]:
        print("  #%d\n    A %s\n    B %s" % (i, p, q))
    fdiffer = [(i, p, q) for i, (p, q) in enumerate(zip(fa, fb)) if p != q]
    print("fills, in order: positions that differ: %d" % len(fdiffer))
    for i, p, q in fdiffer:
        print("  fill #%d  A grid %s workgroup %s   B grid %s workgroup %s" % (i, p[1], p[2], q[1], q[2]))
    print("launches per kernel name (A; B where it differs):")
    ca, cb = collections.Counter(l[0] for l in a), collections.Counter(l[0] for l in b)
    for name in sorted(set(ca) | set(cb)):
        print("  %5d%s  %s" % (ca[name], "" if ca[name] == cb[name] else " / %d" % cb[name], name[:150]))
    same = len(ka) == len(kb) and not differ and len(fa) == len(fb)
    print("verdict: %s" % ("identical ordered launch lists" + (" apart from the sizes of %d memset fills" % len(fdiffer) if fdiffer else "") if same else "DIFFERENT"))
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run())
