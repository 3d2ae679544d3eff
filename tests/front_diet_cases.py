"""The shapes tests/test_gpu_front_diet.py runs the streaming front end at, their seeded inputs and the digest of the six logit maps:
shared with tools/front_diet_digests.py, which printed profiles/front_diet_digests.txt from the build BEFORE the front end's
instruction diet (front2_kernel's folded scale and dropped selects, s1h_kernel's two fill steps).  No test in here."""
import hashlib
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(REPO, "profiles", "front_diet_digests.txt")

# (H, W): 32x32 one strip, one band, maps too small for the streaming stage-2 kernels; 64x96; 96x288: 18 output columns in stage 3, a full
# strip of 15 and a short one; 352x352 the bench shape; 512x384: two-band forms and a wide second strip.
# 96x272 (17 output columns in stage 3) was asked for and cannot run: yfv2_create refuses a width that is no multiple of 32 (REFUSED,
# tests/test_gpu_front_diet.py pins the refusal); 96x288 is the nearest width with a full strip and a short one behind it.
SHAPES = ((32, 32), (64, 96), (96, 288), (352, 352), (512, 384))
REFUSED = ((96, 272),)
BATCHES = (1, 3)
DTYPES = ("fp32", "uint8")
BIG = (32, 32)          # one batch larger than the CU count at this shape (cus + 1 images)


def images_u8(H, W, B):
    """(B, H, W, 3) uint8 from a CPU generator: the same bytes on every machine; the fp32 input is these / 255 in NCHW"""
    g = torch.Generator().manual_seed(1000 * H + W)
    return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)


def as_input(x8, dtype):
    return x8.contiguous() if dtype == "uint8" else (x8.permute(0, 3, 1, 2).float() / 255.0).contiguous()


def digest(logits):
    h = hashlib.sha256()
    for t in logits:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def case_key(H, W, B, dtype):
    return "%dx%d B=%d %s" % (H, W, B, dtype)


def recorded_digests():
    out = {}
    with open(DIGESTS) as f:
        for ln in f:
            if ln.startswith("digest "):
                key, _, hx = ln[len("digest "):].rpartition(": ")
                out[key] = hx.strip()
    return out
