"""Every plan switch (include/yfv2.h yfv2_plan) on the device at the shapes of tests/plan_cases.py: other sizes, batches and class
counts than the 352x352 / 80-class point test_gpu_parity.py::test_fallback_plans_match_oracle runs them at.  The alternative plans
run kernels of their own (stem_px_kernel, s2px / s1px on the fp32 MFMA, tower2_kernel, block_s2 / block_s2w / block_s1pool, the
pointwise and depthwise set of yfv2_conv.hip) with their own shape thresholds; tests/test_plan_cases_host.py shows on the CPU that
the table reaches every launch sequence they take, this file runs each case (tests/gpu_cases/plan_shapes.py: launch names against
the dry run, fp32 and uint8 logits within the noise floor of the oracle, decode, bit-exact NMS, detect == three calls, batch ==
chunks, two-launch post == fused post).  Each case runs in its own interpreter so that a device fault cannot take the rest of
the suite with it - but a crash, a hang or a mismatch FAILS."""
import json
import os
import subprocess
import sys

import pytest

import plan_cases as P

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_cases", "plan_shapes.py")


@pytest.mark.parametrize("index", range(len(P.CASES)), ids=[P.case_id(c) for c in P.CASES])
def test_plan_case_in_its_own_interpreter(index, record_parity):
    c = P.CASES[index]
    r = subprocess.run([sys.executable, SCRIPT, str(index)], capture_output=True, text=True, timeout=240)
    marks = [ln for ln in r.stdout.splitlines() if ln.startswith("[plan_shapes]")]
    assert r.returncode == 0, ("exit code %d after %r" % (r.returncode, marks[-1] if marks else "no marker"), r.stdout[-1500:], r.stderr[-3000:])
    assert "PLAN CASE OK %s" % P.case_id(c) in r.stdout
    figures = [ln for ln in r.stdout.splitlines() if ln.startswith("FIGURES ")]
    assert len(figures) == 1
    fig = json.loads(figures[0][len("FIGURES "):])
    assert fig.pop("case") == P.case_id(c)
    record_parity("plan_case " + P.case_id(c), **fig)
