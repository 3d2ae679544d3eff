"""The noise-floor rule of the GPU parity tests, shared by tests/test_gpu_parity.py and the drivers under tests/gpu_cases/.

Where an absolute tolerance does not apply - random-init weights give logits of magnitude 20-40 - the device is NOT granted a
tolerance scaled by the logit magnitude.  It is held to a small multiple of the error the REFERENCE's own fp32 arithmetic (= the
oracle's, pinned bit-equal) makes against a float64 evaluation of the same network on the same input:
|device - float64| <= K * |reference_fp32 - float64|, per tensor, for the largest and for the rms error.  K = 2 on large samples
(the bench regime: 16 images); K = 3 where a tensor has few elements and the largest error of either side is a noisy statistic.
FLOOR_MIN_REL: no fp32 execution is asked to be closer than two ulps of the tensor's magnitude on its worst element."""
import numpy as np

from oracle import yfv2_oracle as oracle

LOGIT_KEYS = ("reg2", "obj2", "cls2", "reg3", "obj3", "cls3")
FLOOR_K = 2.0
FLOOR_K_SMALL = 3.0
FLOOR_MIN_REL = 2.0 ** -22


def err_stats(got, exact):
    d = np.asarray(got, np.float64) - np.asarray(exact, np.float64)
    return float(np.abs(d).max()), float(np.sqrt((d * d).mean()))


def assert_logits_within_noise_floor(got, w, x, what="", k=FLOOR_K_SMALL, err_ref=None, refs=None):
    """got: six device logit maps for input x (CPU tensor) under weights w.  Returns {key: (dev max, dev rms, ref max, ref rms)}.
    refs: (float64 maps, fp32 maps) of the oracle on exactly (w, x) as numpy arrays, where the caller already has them."""
    p64 = [t.numpy() for t in oracle.forward64(w, x)] if refs is None else refs[0]
    p32 = ([t.numpy() for t in oracle.forward(w, x)] if refs is None else refs[1]) if err_ref is None else None
    out = {}
    for i, key in enumerate(LOGIT_KEYS):
        g = got[i].detach().cpu().numpy()
        assert g.shape == p64[i].shape, "%s %s: shape %s vs %s" % (what, key, g.shape, p64[i].shape)
        d_max, d_rms = err_stats(g, p64[i])
        r_max, r_rms = err_stats(p32[i], p64[i]) if err_ref is None else (float(err_ref[key][0]), float(err_ref[key][1]))
        floor = FLOOR_MIN_REL * max(1.0, float(np.abs(p64[i]).max()))
        out[key] = (d_max, d_rms, r_max, r_rms)
        assert d_max <= k * max(r_max, floor), "%s %s: device is %.3g from float64, the reference's fp32 %.3g (bound %gx)" % (what, key, d_max, r_max, k)
        assert d_rms <= k * max(r_rms, floor / 4), "%s %s: rms %.3g from float64, the reference's fp32 %.3g (bound %gx)" % (what, key, d_rms, r_rms, k)
    return out
