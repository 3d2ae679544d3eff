"""The device side of the reference's ``utils/datasets.py``: from DECODED frames to the batch ``train.py`` trains on.

    batcher = TrainBatcher(engine, imgaug=True)                 # TensorDataset(..., imgaug=True) + collate_fn, minus the decoding
    imgs, targets = batcher(frames, labels)                     # fp32 (B,3,H,W) in [0,1] and (N,6) targets, both on the GPU
    preds = model(imgs); compute_loss(preds, targets, cfg, device)

What runs where.  ``TensorDataset.__getitem__`` (datasets.py:101-129) decodes an image, resizes it, augments it, transposes it and
reads its label file; ``collate_fn`` (:70-75) stacks and numbers the labels; ``train.py:101`` converts and divides by 255.  Here the
resize, the augmentation, the transpose and the conversion are ONE launch (Engine.train_batch_frames, include/yfv2.h
yfv2_train_batch_frames_u8 / _yuv).  The augmentation is ``contrast_and_brightness`` (:10-16), the only one ``img_aug`` runs -
``motion_blur``, ``random_resize`` and ``augment_hsv`` are commented out in the reference (:65-67) and are not here.  Decoding stays
the caller's, as for every other frame entry point: there is no file-list walk and no DataLoader here.
"""
import random

import numpy as np
import torch

from . import yuv

LDS_FULL = 160 * 1024


def draw_contrast_brightness(rng=random):
    """(alpha, beta) as datasets.py:11-12 draws them: two ``uniform(0.25, 1.75)`` calls, alpha first.  ``rng``: the ``random``
    module (the reference's generator, so ``random.seed(s)`` reproduces its draws) or any ``random.Random``."""
    alpha = rng.uniform(0.25, 1.75)
    beta = rng.uniform(0.25, 1.75)
    return alpha, beta


def read_label_file(path):
    """datasets.py:114-120: one ``class cx cy w h`` line per box -> float32 (n, 6) rows ``[0, class, cx, cy, w, h]`` (column 0 is
    the image index collate_targets fills in).  A file without lines gives (0, 6)."""
    label = []
    with open(path, "r") as f:
        for line in f.readlines():
            l = line.strip().split(" ")
            label.append([0, l[0], l[1], l[2], l[3], l[4]])
    label = np.array(label, dtype=np.float32)
    if label.shape[0]:
        assert label.shape[1] == 6, "> 5 label columns: %s" % path      # datasets.py:123
    return label.reshape(-1, 6)


def collate_targets(labels):
    """The label half of collate_fn (datasets.py:70-75): label array i (n_i, 6; numpy or tensor) gets i in column 0 where it has
    rows, then all are concatenated -> float32 (N, 6) CPU tensor.  The caller's arrays are not written."""
    out = []
    for i, l in enumerate(labels):
        l = torch.as_tensor(np.asarray(l), dtype=torch.float32).reshape(-1, 6).clone()
        if l.shape[0] > 0:
            l[:, 0] = i
        out.append(l)
    return torch.cat(out, 0) if out else torch.zeros((0, 6), dtype=torch.float32)


def _train_rows(w, W, is_yuv, bits, general=False):
    if bits not in (8, 10) or (bits == 10 and not is_yuv):
        raise ValueError("bits must be 8, or 10 for YUV frames (\"p010\", \"i010\"), got %r" % (bits,))
    if general:
        if not is_yuv or bits != 8:
            raise ValueError("general=True is the launch of 8-bit YUV frames of any sampling")
        return yuv.rows_lds_any(yuv.ROWS_TRAIN, w, W)
    return yuv.rows_lds(yuv.ROWS_TRAIN, is_yuv, w, W) if bits == 8 else yuv.rows_lds16(yuv.ROWS_TRAIN, w, W)


def train_batch_lds_bytes(w, W, is_yuv=False, bits=8, general=False):
    """LDS of one workgroup of the training-batch launch for a frame w pixels wide at network width W: the resize's staging slots
    rounded to 16 bytes, the table, three fp32 planes of W"""
    return _train_rows(w, W, is_yuv, bits, general)[0]


def max_frame_width(W, is_yuv=False, bits=8, general=False):
    """the widest frame Engine.train_batch_frames (is_yuv: train_batch_frames_yuv; bits = 10: "p010" / "i010" frames; general: a
    batch with an 8-bit frame that is not 4:2:0 - a JPEG set's "i444", "i422", "i440", "yuyv", "uyvy", "grey" - whose limit binds
    every frame of the batch) admits at network width W; never above resize_frames' own limit"""
    return _train_rows(1, W, is_yuv, bits, general)[1]


class TrainBatcher:
    """``TensorDataset(..., imgaug)`` + ``collate_fn`` + train.py:101 for frames that are already decoded and on the GPU.

    ``engine``: the Engine of the network size to train at (``preds[0]._yfv2_engine`` of a Detector forward, or one made for
    the purpose; it needs no weights).  ``imgaug``: draw a contrast / brightness pair per image (datasets.py:109-110), in batch
    order, from ``rng`` (default: the ``random`` module, the reference's generator); False is the validation loader's identity.

    ``batcher(frames, labels) -> (imgs, targets)``: ``frames`` is ONE kind per call - a list of uint8 (h, w, 3) B, G, R device
    tensors, or a list of ``YuvFrame`` (the two kinds are read by different kernels; mixing them would take a second launch) -
    and ``labels`` the per-image (n_i, 6) arrays of read_label_file.  ``imgs`` is the fp32 (B, 3, H, W) batch, ``targets`` the
    float32 (N, 6) tensor, both on the engine's device, ready for ``Detector.train()``'s forward and ``compute_loss``.  The
    pairs drawn for the last call are kept in ``last_alpha`` / ``last_beta``."""

    def __init__(self, engine, imgaug=False, rng=random):
        self.engine, self.imgaug, self.rng = engine, bool(imgaug), rng
        self.last_alpha = self.last_beta = None

    def __call__(self, frames, labels, out=None):
        if not isinstance(frames, (list, tuple)) or not frames:
            raise ValueError("frames must be a non-empty list or tuple")
        if len(labels) != len(frames):
            raise ValueError("%d label arrays for %d frames" % (len(labels), len(frames)))
        tensors = [torch.is_tensor(f) for f in frames]
        if any(tensors) and not all(tensors):
            raise ValueError("one kind of frame per call: all uint8 (h,w,3) tensors or all YuvFrame")
        alpha = beta = None
        if self.imgaug:
            pairs = [draw_contrast_brightness(self.rng) for _ in frames]
            alpha, beta = [p[0] for p in pairs], [p[1] for p in pairs]
        self.last_alpha, self.last_beta = alpha, beta
        make = self.engine.train_batch_frames if all(tensors) else self.engine.train_batch_frames_yuv
        imgs = make(frames, alpha, beta, out=out)
        return imgs, collate_targets(labels).to(self.engine.device)
