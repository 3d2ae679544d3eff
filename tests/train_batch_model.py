"""The numpy statement of the training-batch rule (include/yfv2.h yfv2_train_batch_frames_u8 / _yuv): what a resized uint8 batch
becomes under a frame's contrast / brightness pair and train.py:101's ``.float() / 255.0``.  Every step is an explicit float32
operation, so the roundings are the ones the header names: multiply, add (never fused), rint half-to-even, IEEE division.

This is OpenCV's scalar ``saturate_cast<uchar>(a * alpha + 0 * (1 - alpha) + beta)`` for 8-bit addWeighted with the zero image of
utils/datasets.py:13; parity with cv2 proper is unpinned (its vector body fuses the multiply-add, its tail does not).
"""
import numpy as np


def table(alpha, beta):
    """float32 (256,): entry a is what byte a of a frame with (alpha, beta) becomes"""
    a = np.arange(256, dtype=np.float32)
    alpha, beta = np.float32(alpha), np.float32(beta)
    with np.errstate(over="ignore"):
        t = (a * alpha).astype(np.float32)              # fl32(float(a) * alpha)
        t = (t + beta).astype(np.float32)               # fl32(... + beta): a second rounding, no fma
    q = np.rint(np.minimum(np.maximum(t, np.float32(0)), np.float32(255)))     # half to even, after the clamp
    return (q.astype(np.float32) / np.float32(255)).astype(np.float32)


def quantised(alpha, beta):
    """uint8 (256,): the byte contrast_and_brightness leaves (the table before the division)"""
    return np.rint(table(alpha, beta).astype(np.float64) * 255.0).astype(np.uint8)


def train_batch_ref(resized_u8, alpha=None, beta=None):
    """resized_u8: uint8 (B, H, W, 3), the output of resize_frames / resize_frames_yuv; alpha, beta: B numbers each or None (the
    identity) -> float32 (B, 3, H, W)"""
    x = np.asarray(resized_u8)
    assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[3] == 3
    B = x.shape[0]
    if alpha is None:
        alpha, beta = [1.0] * B, [0.0] * B
    out = np.empty((B, 3) + x.shape[1:3], np.float32)
    for b in range(B):
        out[b] = table(alpha[b], beta[b])[x[b]].transpose(2, 0, 1)
    return out
