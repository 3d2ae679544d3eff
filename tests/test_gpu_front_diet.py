"""The streaming front end after its instruction diet (yfv2_stage2h.hip: front2_kernel multiplies once by the stem's unscale times the
stride-2 block's 2^4, selects nothing where the value is already 0, takes its first tap row as one DPP block and ends a short last
band at its last row, as s3h2_kernel does; s1h_kernel's two fill steps issue no depthwise, pw2 or stores).  Every value still goes through the same operations on the
same operands in the same order, so at every shape of tests/front_diet_cases.py, batches 1 and 3, fp32 and uint8 input:
  * the default plan's six logit maps are bit-equal to the same weights on the front_two_launches plan (stem_h3 / stem_h3u + s2h_kernel,
    which the diet did not touch);
  * they are within LOGIT_ATOL of the CPU oracle (COCO weights);
  * their sha256 is the one the build before the diet gave (profiles/front_diet_digests.txt, tools/front_diet_digests.py).
One batch larger than the CU count at 32x32 must give every image the bits it has in the batch of three."""
import numpy as np
import pytest
import torch

import front_diet_cases as F
from oracle import yfv2_oracle as oracle

pytestmark = pytest.mark.gpu

LOGIT_KEYS = ("reg2", "obj2", "cls2", "reg3", "obj3", "cls3")
LOGIT_ATOL = 1e-4       # tests/test_gpu_parity.py's


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def shape_state(yfv2, dev, coco_weights):
    """per shape, made once: the three seeded images, the oracle's logits on them, one engine per plan (batches 1 and 3 share them)"""
    cache = {}

    def get(H, W):
        if (H, W) not in cache:
            x8 = F.images_u8(H, W, 3)
            ref = [t.detach() for t in oracle.forward(coco_weights, F.as_input(x8, "fp32"))]
            engines = []
            for plan in ({}, {"front_two_launches": 1}):
                e = yfv2.Engine(dev, H, W, 80, 3, max_batch=3, plan=plan)
                e.load_state_dict(coco_weights)
                engines.append(e)
            cache[(H, W)] = (x8, ref, engines)
        return cache[(H, W)]
    return get


@pytest.fixture(scope="module")
def recorded():
    return F.recorded_digests()


@pytest.mark.parametrize("dtype", F.DTYPES)
@pytest.mark.parametrize("B", F.BATCHES)
@pytest.mark.parametrize("hw", F.SHAPES, ids=["%dx%d" % s for s in F.SHAPES])
def test_default_plan_logits_are_those_of_the_two_launch_front_the_oracle_and_the_build_before(shape_state, recorded, dev, hw, B, dtype):
    H, W = hw
    x8, ref, (e_def, e_two) = shape_state(H, W)
    x = F.as_input(x8[:B], dtype).to(dev)
    got = [t.cpu() for t in e_def.forward(x)]
    two = [t.cpu() for t in e_two.forward(x)]
    assert not e_def.nonfinite() and not e_two.nonfinite()
    for k, a, b in zip(LOGIT_KEYS, got, two):
        assert torch.equal(a, b), "%s: %d of %d elements differ from the two-launch front" % (k, int((a != b).sum()), a.numel())
    for k, a, r in zip(LOGIT_KEYS, got, ref):
        err = float((a - r[:B]).abs().max())
        print("%s %s: max abs err against the oracle %.3g" % (F.case_key(H, W, B, dtype), k, err))
        assert err <= LOGIT_ATOL, "%s: max abs err %g" % (k, err)
    key = F.case_key(H, W, B, dtype)
    assert key in recorded, "no recorded digest for " + key
    assert F.digest(got) == recorded[key], "logit digest of %s differs from the build before the diet" % key


def test_a_width_that_is_no_multiple_of_32_is_refused(yfv2, dev):
    """96x272 would give stage 3 seventeen output columns; the library takes multiples of 32 only, so 96x288 stands in for it above"""
    for (H, W) in F.REFUSED:
        with pytest.raises(yfv2.Yfv2Error, match="multiples of 32"):
            yfv2.Engine(dev, H, W, 80, 3, max_batch=1, plan={})


@pytest.mark.parametrize("dtype", F.DTYPES)
def test_a_batch_beyond_the_cu_count_keeps_every_image_s_bits(yfv2, dev, coco_weights, shape_state, dtype):
    H, W = F.BIG
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    B = cus + 1
    x8, ref, (e_def, e_two) = shape_state(H, W)
    small = [t.cpu() for t in e_def.forward(F.as_input(x8, dtype).to(dev))]
    xb = F.as_input(x8.repeat((B + 2) // 3, 1, 1, 1)[:B], dtype).to(dev)
    outs = []
    for plan in ({}, {"front_two_launches": 1}):
        e = yfv2.Engine(dev, H, W, 80, 3, max_batch=B, plan=plan)
        e.load_state_dict(coco_weights)
        outs.append([t.cpu() for t in e.forward(xb)])
        assert not e.nonfinite()
    idx = torch.arange(B) % 3
    for k, a, b, s in zip(LOGIT_KEYS, outs[0], outs[1], small):
        assert torch.equal(a, b), "%s: default and two-launch front differ at B = %d" % (k, B)
        assert torch.equal(a, s[idx]), "%s: an image of the batch of %d differs from itself in the batch of three" % (k, B)
    for k, s, r in zip(LOGIT_KEYS, small, ref):
        assert float((s - r).abs().max()) <= LOGIT_ATOL, k
