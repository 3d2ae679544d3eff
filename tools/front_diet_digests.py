#!/usr/bin/env python3
"""One process = one build of the library (YFV2_LIB=path, else the tree's): sha256 of the six logit maps of the default plan, COCO
weights, at the shapes, batches and input types of tests/front_diet_cases.py.  Two builds print the same lines iff their logits are
bit-identical there; profiles/front_diet_digests.txt is the output of the build before the front end's instruction diet and
tests/test_gpu_front_diet.py holds every later build to it.   usage: [YFV2_LIB=..] python tools/front_diet_digests.py"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

import front_diet_cases as F  # noqa: E402
import yolo_fastestv2_amd as yfv2  # noqa: E402
from oracle import yfv2_oracle as oracle  # noqa: E402

dev = torch.device("cuda:0")
w = oracle.load_weights(os.path.join(REPO, "tests", "golden", "weights_coco.npz"))
for (H, W) in F.SHAPES:
    e = yfv2.Engine(dev, H, W, 80, 3, max_batch=3, plan={})
    e.load_state_dict(w)
    x8 = F.images_u8(H, W, 3)
    for B in F.BATCHES:
        for dtype in F.DTYPES:
            out = e.forward(F.as_input(x8[:B], dtype).to(dev))
            torch.cuda.synchronize()
            print("digest %s: %s" % (F.case_key(H, W, B, dtype), F.digest(out)), flush=True)
    assert not e.nonfinite()
    del e
