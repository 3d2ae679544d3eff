"""Engine: one libyfv2 handle on one GPU.  PyTorch is used for device memory,
streams and host<->device copies only; every arithmetic op runs in the HIP
kernels behind the C ABI (include/yfv2.h)."""
import ctypes as C

import torch

from . import _lib, tiling, tracking, yuv
from ._lib import MAX_DET, Config, TensorDesc, check
from .tracking import APPEARANCE_DEFAULTS as _APP, MOTION_DEFAULTS as _MOT, TWO_PASS_DEFAULTS as _TWO

LOGIT_ORDER = ("reg_2", "obj_2", "cls_2", "reg_3", "obj_3", "cls_3")  # detector.py:47


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ap_dict(res):
    """a yfv2_ap_result as Engine.ap_per_class returns it"""
    import numpy as np
    out = {"n_gt": np.array(res.n_gt, np.int64), "n_pred": np.array(res.n_pred, np.int64),
           "p": np.array(res.p, np.float64), "r": np.array(res.r, np.float64), "ap": np.array(res.ap, np.float64)}
    out["present"] = np.flatnonzero(out["n_gt"] > 0)
    out["bad_input"] = int(res.bad_input)
    out["classes_present"] = int(res.classes_present)
    out["means"] = (float(res.mean_p), float(res.mean_r), float(res.mean_ap), float(res.mean_f1))
    return out


class Engine:
    """Owns a yfv2 handle.  ``max_batch`` grows on demand (the handle is re-created
    and the weights re-uploaded)."""

    def __init__(self, device, height=352, width=352, classes=80, anchor_num=3, anchors=None, max_batch=1, plan=None):
        """plan: dict of yfv2_plan switches ({"fp32_matrix": 1}, {"layer_by_layer": 1}, {"lanes": 2} ...; include/yfv2.h), None = what the
        process environment asks for (YFV2_BF6=0 etc., _lib.plan_from_env: how the tools and the fallback-plan tests pick a plan) - with
        nothing set that is the default plan.  The native library itself reads no environment variable."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("yolo_fastestv2_amd runs on an MI355X only (got device %s); there is no CPU path" % device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.height, self.width = int(height), int(width)
        self.classes, self.anchor_num = int(classes), int(anchor_num)
        self.anchors = [float(a) for a in (anchors if anchors is not None else [0.0] * 12)]
        self._anchors_set = anchors is not None   # decode()/detect() refuse to run on the all-zero placeholder
        if len(self.anchors) != 12:
            raise ValueError("expected 12 anchor values (6 pairs), got %d" % len(self.anchors))
        self.max_batch = 0
        self._h = None
        self._weights = None  # host copies (name -> contiguous fp32 cpu tensor), kept for re-creation
        self.plan = dict(_lib.plan_from_env() if plan is None else plan)
        self._create(max_batch)

    # ---- lifetime -------------------------------------------------------------------------
    def _create(self, max_batch):
        L = _lib.lib()
        cfg = Config()
        cfg.classes, cfg.anchor_num = self.classes, self.anchor_num
        cfg.height, cfg.width = self.height, self.width
        for i, a in enumerate(self.anchors):
            cfg.anchors[i] = a
        cfg.max_batch = int(max_batch)
        cfg.device = self.device.index
        h = C.c_void_p()
        check(L.yfv2_create_ex(C.byref(h), C.byref(cfg), C.byref(_lib.make_plan(self.plan))))
        self.close()
        self._h, self.max_batch = h, int(max_batch)
        self._generation = getattr(self, "_generation", 0) + 1   # a NEW native handle: whatever was bound to the old one (yfv2_train_bind) is gone
        self.rows = int(L.yfv2_num_rows(self._h))
        if self._weights is not None:
            self._upload()

    def close(self):
        if self._h is not None:
            _lib.lib().yfv2_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ensure_batch(self, B):
        if B > self.max_batch:
            torch.cuda.synchronize(self.device)
            self._create(max(B, 2 * self.max_batch if self.max_batch < 64 else B))

    # ---- weights --------------------------------------------------------------------------
    def load_state_dict(self, state):
        """state: mapping reference-key -> tensor (any device/dtype); integer
        buffers (num_batches_tracked) are ignored."""
        host = {}
        for k, v in state.items():
            v = torch.as_tensor(v)
            if not v.is_floating_point():
                continue
            host[k] = v.detach().to("cpu", torch.float32).contiguous()
        self._weights = host
        self._upload()

    def _upload(self):
        names = list(self._weights)
        arr = (TensorDesc * len(names))()
        for i, k in enumerate(names):
            t = self._weights[k]
            arr[i].name = k.encode()
            arr[i].data = t.data_ptr()
            arr[i].numel = t.numel()
        check(_lib.lib().yfv2_load_weights(self._h, arr, len(names)), self._h)

    def set_anchors(self, anchors):
        anchors = [float(a) for a in anchors]
        if anchors != self.anchors:
            if len(anchors) != 12:
                raise ValueError("expected 12 anchor values (6 pairs), got %d" % len(anchors))
            self.anchors = anchors
        self._anchors_set = True
        check(_lib.lib().yfv2_set_anchors(self._h, (C.c_double * 12)(*self.anchors)), self._h)

    # ---- shapes ---------------------------------------------------------------------------
    def logit_shapes(self, B):
        A, nc = self.anchor_num, self.classes
        h2, w2, h3, w3 = self.height // 16, self.width // 16, self.height // 32, self.width // 32
        return [(B, 4 * A, h2, w2), (B, A, h2, w2), (B, nc, h2, w2), (B, 4 * A, h3, w3), (B, A, h3, w3), (B, nc, h3, w3)]

    def _check_x(self, x):
        """fp32 (B,3,H,W) in [0,1] (the reference's Detector input), or uint8 (B,H,W,3) in 0..255: the decoded,
        resized image BEFORE test.py:34-38's reshape/permute/float()/255, which the stem kernel then does itself."""
        if x.device != self.device:
            raise ValueError("input on %s, engine on %s" % (x.device, self.device))
        if x.dtype == torch.uint8:
            if x.dim() != 4 or tuple(x.shape[1:]) != (self.height, self.width, 3):
                raise ValueError("expected uint8 (B,%d,%d,3), got %s" % (self.height, self.width, tuple(x.shape)))
        elif x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (3, self.height, self.width):
            raise ValueError("expected fp32 (B,3,%d,%d) or uint8 (B,%d,%d,3), got %s %s" % (self.height, self.width, self.height, self.width, x.dtype, tuple(x.shape)))
        x = x.contiguous()
        if x.data_ptr() % 16:        # a view into the middle of a storage: the stem kernels load 16-byte (fp32) / 4-byte-aligned 12-byte (uint8) records
            x = x.clone()
        return x

    # ---- the hot path ---------------------------------------------------------------------
    def forward(self, x, out=None):
        x = self._check_x(x)
        B = x.shape[0]
        self.ensure_batch(B)
        if out is None:
            out = [torch.empty(s, device=self.device, dtype=torch.float32) for s in self.logit_shapes(B)]
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in out])
        fn = _lib.lib().yfv2_forward_u8 if x.dtype == torch.uint8 else _lib.lib().yfv2_forward
        check(fn(self._h, _ptr(x), B, ptrs, _stream(self.device)), self._h)
        return tuple(out)

    def _need_anchors(self, what):
        if not self._anchors_set:
            raise RuntimeError("Engine.%s: anchors were never given (constructor `anchors=` or set_anchors(cfg['anchors'])); "
                               "the all-zero placeholder would decode every box to zero size" % what)

    def decode(self, preds, out=None):
        self._need_anchors("decode")
        preds = [p.contiguous() for p in preds]
        B = preds[0].shape[0]
        for p, s in zip(preds, self.logit_shapes(B)):
            if tuple(p.shape) != s or p.dtype != torch.float32 or p.device != self.device:
                raise ValueError("logit tensor %s %s on %s, expected fp32 %s on %s" % (p.dtype, tuple(p.shape), p.device, s, self.device))
        self.ensure_batch(B)
        if out is None:
            out = torch.empty((B, self.rows, 5 + self.classes), device=self.device, dtype=torch.float32)
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in preds])
        check(_lib.lib().yfv2_decode(self._h, ptrs, B, _ptr(out), _stream(self.device)), self._h)
        return out

    def new_det_buffers(self, B):
        """(dets, idx, cnt) for `detect` / `nms`: three views of one flat buffer, so that the sharded path's all-gather
        moves a rank's result in one collective (sharded.gather_detections)."""
        from .sharded import packed_det_buffers
        return packed_det_buffers(B, self.device)

    def nms(self, boxes, conf_thres, iou_thres, classes=None, out=None):
        boxes = boxes.contiguous()
        B = boxes.shape[0]
        if tuple(boxes.shape[1:]) != (self.rows, 5 + self.classes) or boxes.dtype != torch.float32 or boxes.device != self.device:
            raise ValueError("decoded tensor %s %s on %s, expected fp32 (B,%d,%d) on %s" % (
                boxes.dtype, tuple(boxes.shape), boxes.device, self.rows, 5 + self.classes, self.device))
        self.ensure_batch(B)
        dets, idx, cnt = out if out is not None else self.new_det_buffers(B)
        if classes is not None:
            cl = [int(c) for c in classes]
            carr, ncl = (C.c_int32 * len(cl))(*cl), len(cl)
        else:
            carr, ncl = None, 0
        check(_lib.lib().yfv2_nms(self._h, _ptr(boxes), B, float(conf_thres), float(iou_thres), carr, ncl, _ptr(dets),
                                  _ptr(idx), _ptr(cnt), _stream(self.device)), self._h)
        return dets, idx, cnt

    def post(self, preds, conf_thres, iou_thres, out=None):
        """What detect() runs after its forward, on the caller's six logit maps (include/yfv2.h yfv2_debug_post): the fused
        decode + NMS launch where the plan and the shape allow it, else decode into compact rows + NMS.  Enqueue only."""
        self._need_anchors("post")
        preds = [p.contiguous() for p in preds]
        B = preds[0].shape[0]
        for p, s in zip(preds, self.logit_shapes(B)):
            if tuple(p.shape) != s or p.dtype != torch.float32 or p.device != self.device:
                raise ValueError("logit tensor %s %s on %s, expected fp32 %s on %s" % (p.dtype, tuple(p.shape), p.device, s, self.device))
        self.ensure_batch(B)
        dets, idx, cnt = out if out is not None else self.new_det_buffers(B)
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in preds])
        check(_lib.lib().yfv2_debug_post(self._h, ptrs, B, float(conf_thres), float(iou_thres), _ptr(dets), _ptr(idx), _ptr(cnt),
                                         _stream(self.device)), self._h)
        return dets, idx, cnt

    def detect(self, x, conf_thres, iou_thres, out=None, check=True):
        """forward + decode + NMS, enqueue only: the results are device tensors and nothing waits for the device.  check=True
        (default) LOOKS at the range-guard word first (yfv2_nonfinite_peek: a host memory read, no synchronisation) and raises if a
        call that has already completed on this handle tripped it - a loop that never synchronises with the host learns of
        invalid results one call late instead of never; `check_finite()` after a synchronisation is the exact query."""
        self._need_anchors("detect")
        if check and self.peek_nonfinite():
            self.check_finite("detect (an earlier call on this handle)")
        x = self._check_x(x)
        B = x.shape[0]
        self.ensure_batch(B)
        dets, idx, cnt = out if out is not None else self.new_det_buffers(B)
        fn = _lib.lib().yfv2_detect_u8 if x.dtype == torch.uint8 else _lib.lib().yfv2_detect
        _lib.check(fn(self._h, _ptr(x), B, float(conf_thres), float(iou_thres), _ptr(dets), _ptr(idx), _ptr(cnt), _stream(self.device)), self._h)
        return dets, idx, cnt

    def resize(self, frames, out=None):
        """uint8 (B, h, w, 3) frames on the GPU -> uint8 (B, height, width, 3): cv2.resize(..., INTER_LINEAR) of test.py:35 /
        utils/datasets.py:107 on the device; the result feeds forward()/detect() directly."""
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or frames.device != self.device:
            raise ValueError("frames must be uint8 (B,h,w,3) on %s" % self.device)
        frames = frames.contiguous()
        B, sh, sw = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if out is None:
            out = torch.empty((B, self.height, self.width, 3), device=self.device, dtype=torch.uint8)
        check(_lib.lib().yfv2_resize_u8(self._h, _ptr(frames), B, sh, sw, _ptr(out), _stream(self.device)), self._h)
        return out

    def _frame_table(self, frames):
        """list / tuple of uint8 (h_i, w_i, 3) device tensors -> (yfv2_frame array, the tensors it points into).  A tensor whose rows are
        packed pixels (stride(2) == 1, stride(1) == 3) with a row pitch stride(0) >= 3 w - a crop of a larger frame, any base
        address - is passed as it is; anything else is made contiguous first."""
        if not isinstance(frames, (list, tuple)) or not frames:
            raise ValueError("frames must be a non-empty list or tuple of uint8 (h,w,3) tensors")
        keep = []
        arr = (_lib.Frame * len(frames))()
        for i, f in enumerate(frames):
            if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.device != self.device or f.dim() != 3 or f.shape[2] != 3:
                raise ValueError("frame %d: expected a uint8 (h,w,3) tensor on %s, got %s" % (
                    i, self.device, "%s %s on %s" % (f.dtype, tuple(f.shape), f.device) if isinstance(f, torch.Tensor) else type(f).__name__))
            h, w = int(f.shape[0]), int(f.shape[1])
            packed = lambda t: t.stride(2) == 1 and (w <= 1 or t.stride(1) == 3) and (h <= 1 or t.stride(0) >= 3 * w)
            if not packed(f):
                f = f.contiguous()
            keep.append(f)
            arr[i].data, arr[i].height, arr[i].width = f.data_ptr(), h, w
            arr[i].row_pitch = f.stride(0) if h > 1 else 3 * w
        return arr, keep

    def _yuv_table(self, frames):
        return yuv.frame_table(frames, self.device)

    # The bodies of the frame entry points, one per operation.  `table`: self._frame_table or self._yuv_table, frames -> (the native
    # array, what it points into); `native`: the library function of that frame kind; `name`: the public method, for messages.
    def _resize_frames(self, table, native, frames, out):
        arr, keep = table(frames)
        B = len(keep)
        self.ensure_batch(B)
        if out is None:
            out = torch.empty((B, self.height, self.width, 3), device=self.device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (B, self.height, self.width, 3) or out.device != self.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 (%d,%d,%d,3) tensor on %s" % (B, self.height, self.width, self.device))
        check(native(self._h, arr, B, _ptr(out), _stream(self.device)), self._h)
        return out

    def _train_batch_frames(self, name, table, native, frames, alpha, beta, out):
        arr, keep = table(frames)
        B = len(keep)
        if (alpha is None) != (beta is None):
            raise ValueError("%s: alpha and beta must both be given or both be None" % name)
        pair = [None, None]
        for k, v in enumerate((alpha, beta)):
            if v is not None:
                v = [float(a) for a in (v.tolist() if hasattr(v, "tolist") else v)]
                if len(v) != B:
                    raise ValueError("%s: %s has %d entries for %d frames" % (name, ("alpha", "beta")[k], len(v), B))
                pair[k] = (C.c_float * B)(*v)
        self.ensure_batch(B)
        if out is None:
            out = torch.empty((B, 3, self.height, self.width), device=self.device, dtype=torch.float32)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, self.height, self.width) or out.device != self.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous fp32 (%d,3,%d,%d) tensor on %s" % (B, self.height, self.width, self.device))
        check(native(self._h, arr, B, pair[0], pair[1], _ptr(out), _stream(self.device)), self._h)
        return out

    def _detect_frames(self, name, table, native, frames, conf_thres, iou_thres, out, check):
        self._need_anchors(name)
        if check and self.peek_nonfinite():
            self.check_finite("%s (an earlier call on this handle)" % name)
        arr, keep = table(frames)
        B = len(keep)
        self.ensure_batch(B)
        dets, idx, cnt = out if out is not None else self.new_det_buffers(B)
        _lib.check(native(self._h, arr, B, float(conf_thres), float(iou_thres), _ptr(dets), _ptr(idx), _ptr(cnt), _stream(self.device)), self._h)
        return dets, idx, cnt

    def _detect_tiled(self, name, table, native, size_of, frames, tiles, conf_thres, iou_thres, merge_thres, metric, max_out, tile, overlap,
                      include_full, out, check):
        """size_of: a kept frame -> (height, width), what the tile plan needs"""
        self._need_anchors(name)
        code = tiling.metric_code(metric)
        max_out = int(max_out)
        if not 1 <= max_out <= 4096:
            raise ValueError("max_out must be in 1..4096, got %d" % max_out)
        if merge_thres is None:
            merge_thres = iou_thres
        if check and self.peek_nonfinite():
            self.check_finite("%s (an earlier call on this handle)" % name)
        farr, keep = table(frames)
        F = len(keep)
        if tiles is None:
            tiles = [t for f, fr in enumerate(keep) for t in tiling.plan_tiles(*size_of(fr), tile, overlap, include_full, frame=f)]
        tarr = tiling.tile_table(tiles)
        T = len(tarr)
        self.ensure_batch(T)
        dets, src, cnt = self._tiled_out(out, F, max_out)
        _lib.check(native(self._h, farr, F, tarr, T, float(conf_thres), float(iou_thres), float(merge_thres), code, max_out,
                          _ptr(dets), _ptr(src) if src is not None else None, _ptr(cnt), _stream(self.device)), self._h)
        return dets, src, cnt

    def resize_frames(self, frames, out=None):
        """A list of uint8 (h_i, w_i, 3) frames of any sizes on the GPU -> uint8 (B, height, width, 3): `resize` for a batch whose frames
        differ in size (test.py:34-35 per frame, include/yfv2.h yfv2_resize_frames_u8).  Frame b's output is bit-identical to
        resize() of that frame alone.  Grows max_batch like every batched call (the descriptor table has max_batch entries)."""
        return self._resize_frames(self._frame_table, _lib.lib().yfv2_resize_frames_u8, frames, out)

    def train_batch_frames(self, frames, alpha=None, beta=None, out=None):
        """The training batch of a list of decoded frames (what resize_frames takes): utils/datasets.py:107-111 and train.py:101 in one
        launch - each frame resized, its contrast / brightness pair applied (alpha[b], beta[b]: datasets.py:10-16, see
        datasets.draw_contrast_brightness; None, None: the identity, imgaug=False), transposed and divided by 255: the fp32
        (B, 3, height, width) tensor train_forward takes.  Bit-identical to resize_frames(frames) followed by the per-byte table of
        include/yfv2.h yfv2_train_batch_frames_u8 and permute(0, 3, 1, 2); no uint8 batch is written.  alpha / beta: B numbers each
        (sequence, numpy array or CPU tensor), finite.  Grows max_batch like resize_frames.  Enqueue only."""
        return self._train_batch_frames("train_batch_frames", self._frame_table, _lib.lib().yfv2_train_batch_frames_u8, frames, alpha, beta, out)

    def train_batch_frames_yuv(self, frames, alpha=None, beta=None, out=None):
        """`train_batch_frames` for a list of yuv.YuvFrame (what resize_frames_yuv takes): bit-identical to resize_frames_yuv(frames)
        followed by the same table and permute."""
        return self._train_batch_frames("train_batch_frames_yuv", self._yuv_table, _lib.lib().yfv2_train_batch_frames_yuv, frames, alpha, beta, out)

    def detect_frames(self, frames, conf_thres, iou_thres, out=None, check=True):
        """test.py:34-35,58-68 for a batch of frames of any sizes: resize each uint8 (h_i, w_i, 3) device frame to (height, width)
        (cv2.resize INTER_LINEAR, test.py:34-35), detect, then scale each box back to its frame - x by w_i / width, y by h_i / height,
        in double and rounded to fp32, as test.py:58-68 does with its Python floats (no clipping).  Returns (dets, idx, cnt) like
        detect(), dets in frame coordinates; conf, class, idx, cnt are what detect() returns for the resized batch.  Enqueue only:
        nothing waits for the device (the first call on a handle allocates its resize buffer and waits once); check= as in detect()."""
        return self._detect_frames("detect_frames", self._frame_table, _lib.lib().yfv2_detect_frames_u8, frames, conf_thres, iou_thres, out, check)

    # ---- tiled detection of large frames (include/yfv2.h yfv2_merge_tiles / yfv2_detect_tiled_u8) ----------------
    def new_tiled_buffers(self, F, max_out=MAX_DET):
        """(dets (F, max_out, 6) fp32, src (F, max_out) int32, count (F) int32) for detect_tiled / merge_tiles"""
        return (torch.empty((F, max_out, 6), device=self.device, dtype=torch.float32),
                torch.empty((F, max_out), device=self.device, dtype=torch.int32), torch.empty((F,), device=self.device, dtype=torch.int32))

    def _tiled_out(self, out, F, max_out):
        if out is None:
            return self.new_tiled_buffers(F, max_out)
        dets, src, cnt = out
        for t, shape, dt in ((dets, (F, max_out, 6), torch.float32), (src, (F, max_out), torch.int32), (cnt, (F,), torch.int32)):
            if t is None and shape == (F, max_out):
                continue            # src is optional
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError("out must be contiguous (dets %s fp32, src %s int32 or None, count %s int32) on %s" % (
                    (F, max_out, 6), (F, max_out), (F,), self.device))
        return dets, src, cnt

    def merge_tiles(self, tile_dets, tile_count, tiles, F, merge_thres, metric="iou", max_out=MAX_DET, out=None):
        """The merge alone: tile_dets (T, 300, 6) fp32 / tile_count (T) int32 on the device in detect_frames' layout (tile
        coordinates), tiles = T tuples (frame, x0, y0, width, height) with non-decreasing frame in [0, F).  Every frame's rows are
        moved into the frame, ordered by conf (stable over tile, row) and walked greedily: a row is dropped if a kept row of the
        same class matches it by more than merge_thres (metric "iou", or "ios" = intersection over the smaller box).  Returns
        (dets (F, max_out, 6), src (F, max_out) = tile * 300 + row of each kept row, count (F)); rows beyond count are not
        written.  Enqueue only."""
        code = tiling.metric_code(metric)
        arr = tiling.tile_table(tiles)
        T, F, max_out = len(arr), int(F), int(max_out)
        if (not torch.is_tensor(tile_dets) or tuple(tile_dets.shape) != (T, MAX_DET, 6) or tile_dets.dtype != torch.float32 or tile_dets.device != self.device
                or not torch.is_tensor(tile_count) or tuple(tile_count.shape) != (T,) or tile_count.dtype != torch.int32 or tile_count.device != self.device):
            raise ValueError("tile_dets must be fp32 (%d,%d,6) and tile_count int32 (%d,) on %s" % (T, MAX_DET, T, self.device))
        if F < 1 or not 1 <= max_out <= 4096:
            raise ValueError("F must be >= 1 and max_out in 1..4096")
        tile_dets, tile_count = tile_dets.contiguous(), tile_count.contiguous()
        dets, src, cnt = self._tiled_out(out, F, max_out)
        check(_lib.lib().yfv2_merge_tiles(self._h, _ptr(tile_dets), _ptr(tile_count), arr, T, F, float(merge_thres), code, max_out, _ptr(dets),
                                          _ptr(src) if src is not None else None, _ptr(cnt), _stream(self.device)), self._h)
        return dets, src, cnt

    def detect_tiled(self, frames, tiles=None, conf_thres=0.3, iou_thres=0.4, merge_thres=None, metric="iou", max_out=MAX_DET,
                     tile=(352, 352), overlap=(64, 64), include_full=False, out=None, check=True):
        """Detection on frames larger than the network's input: every tile (a crop of its frame, read in place) goes through
        detect_frames' path, the boxes move into frame coordinates and one greedy pass per frame removes the duplicates the
        overlaps produce - on the device, in one call.  frames: list of uint8 (h_i, w_i, 3) device tensors; tiles: list of
        (frame, x0, y0, width, height), frame non-decreasing - None plans every frame with `tile`, `overlap`, `include_full`
        (tiling.plan_tiles).  merge_thres None = iou_thres; metric "iou" or "ios" (intersection over the smaller box: merges an
        object cut by a tile edge with its whole view next door).  Returns (dets (F, max_out, 6), src (F, max_out), count (F));
        src = tile * 300 + row in that tile's detections.  The number of tiles is this call's batch: max_batch grows to it.
        Enqueue only (the first call on a handle allocates its tile workspaces and waits once); check= as in detect()."""
        return self._detect_tiled("detect_tiled", self._frame_table, _lib.lib().yfv2_detect_tiled_u8, lambda fr: (int(fr.shape[0]), int(fr.shape[1])),
                                  frames, tiles, conf_thres, iou_thres, merge_thres, metric, max_out, tile, overlap, include_full, out, check)

    # ---- decoder-format frames: YUV 4:2:0 planes read in place (include/yfv2.h yfv2_*_yuv) -----------------------
    def resize_frames_yuv(self, frames, out=None):
        """`resize_frames` for a list of yuv.YuvFrame (NV12 / NV21 / I420 planes on the GPU, any sizes, crops by x0 / y0 / width / height;
        a bare (y, uv) or (y, u, v) tuple is NV12 / I420 in BT.601 limited range).  The output is bit-identical to resize_frames of the
        frames converted to B, G, R by the integer formula of include/yfv2.h; no converted frame is ever written."""
        return self._resize_frames(self._yuv_table, _lib.lib().yfv2_resize_frames_yuv, frames, out)

    def detect_frames_yuv(self, frames, conf_thres, iou_thres, out=None, check=True):
        """`detect_frames` for a list of yuv.YuvFrame: the same path with the resize launch reading the YUV planes.  Bit-identical to
        detect_frames on the converted frames.  Enqueue only; check= as in detect()."""
        return self._detect_frames("detect_frames_yuv", self._yuv_table, _lib.lib().yfv2_detect_frames_yuv, frames, conf_thres, iou_thres, out, check)

    def detect_tiled_yuv(self, frames, tiles=None, conf_thres=0.3, iou_thres=0.4, merge_thres=None, metric="iou", max_out=MAX_DET,
                         tile=(352, 352), overlap=(64, 64), include_full=False, out=None, check=True):
        """`detect_tiled` for a list of yuv.YuvFrame: a tile is its frame's descriptor moved by the tile's origin, so tiles of any
        parity are read in place.  Bit-identical to detect_tiled on the converted frames; same arguments and results."""
        return self._detect_tiled("detect_tiled_yuv", self._yuv_table, _lib.lib().yfv2_detect_tiled_yuv, lambda fr: (fr.height, fr.width),
                                  frames, tiles, conf_thres, iou_thres, merge_thres, metric, max_out, tile, overlap, include_full, out, check)

    # ---- second-stage crops (include/yfv2.h yfv2_crop_detections_u8 / _yuv) ---------------------------------------
    def _crop_detections(self, name, table, native, frames, dets, count, out_size, pad, max_per_frame, classes, cap, out, tensor=None):
        """tensor: None - uint8 (cap, h, w, 3) crops; (a _lib.CropTensor, its torch dtype) - the (cap, 3, h, w) tensor of crop_tensors"""
        arr, keep = table(frames)
        B = len(keep)
        if (not torch.is_tensor(dets) or dets.dim() != 3 or dets.shape[0] != B or dets.shape[2] != 6 or dets.dtype != torch.float32 or dets.device != self.device
                or not dets.is_contiguous() or not torch.is_tensor(count) or tuple(count.shape) != (B,) or count.dtype != torch.int32
                or count.device != self.device or not count.is_contiguous()):
            raise ValueError("%s: dets must be contiguous fp32 (%d,R,6) and count contiguous int32 (%d,) on %s" % (name, B, B, self.device))
        R = int(dets.shape[1])
        out_h, out_w = (int(v) for v in out_size)
        pad_y, pad_x = (float(v) for v in pad) if isinstance(pad, (tuple, list)) else (float(pad), float(pad))
        max_per_frame = int(max_per_frame)
        rule = _lib.CropRule()
        rule.out_h, rule.out_w, rule.pad_x, rule.pad_y, rule.max_per_frame = out_h, out_w, pad_x, pad_y, max_per_frame
        if classes is not None:
            cl = [int(c) for c in classes]
            carr = (C.c_int32 * max(len(cl), 1))(*cl)
            rule.classes, rule.n_classes = C.cast(carr, C.POINTER(C.c_int32)), len(cl)
        if cap is None:
            cap = B * min(R, max(max_per_frame, 1))
        cap = int(cap)
        shapes = ((cap, out_h, out_w, 3) if tensor is None else (cap, 3, out_h, out_w), (cap,), (cap, 4), (B + 1,), (B,))
        dt0, sh0 = torch.uint8 if tensor is None else tensor[1], shapes[0]
        if out is None:
            if cap < 1 or out_h < 1 or out_w < 1:
                raise ValueError("%s: cap and out_size must be >= 1" % name)
            out = tuple(torch.empty(sh, device=self.device, dtype=dt0 if i == 0 else torch.int32) for i, sh in enumerate(shapes))
        else:
            if len(out) != 5:
                raise ValueError("%s: out must be (crops, crop_src, crop_rect, crop_offset, crop_skipped)" % name)
            for i, (t, sh) in enumerate(zip(out, shapes)):
                if t is None and i == 4:
                    continue            # crop_skipped is optional
                dt = dt0 if i == 0 else torch.int32
                if not torch.is_tensor(t) or tuple(t.shape) != sh or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                    raise ValueError("%s: out must be contiguous (%s, crop_src %s, crop_rect %s, crop_offset %s, crop_skipped %s or None, "
                                     "int32) on %s" % ((name, "crops %s uint8" % (sh0,) if tensor is None else "tensors %s %s" % (sh0, dt0)) + shapes[1:]
                                                       + (self.device,)))
        self.ensure_batch(B)
        crops, src, rect, offset, skipped = out
        extra = () if tensor is None else (C.byref(tensor[0]),)
        check(native(self._h, arr, B, _ptr(dets), _ptr(count), R, C.byref(rule), *extra, _ptr(crops), _ptr(src), _ptr(rect), _ptr(offset),
                     _ptr(skipped) if skipped is not None else None, cap, _stream(self.device)), self._h)
        return crops, src, rect, offset, skipped

    def crop_detections(self, frames, dets, count, out_size, pad=0.0, max_per_frame=MAX_DET, classes=None, cap=None, out=None):
        """The step behind detect_frames / detect_tiled in a cascade, on the device: every detection's box, grown by `pad` times its
        extent on each side and clipped to its frame, is cut out of the frame and resized to out_size = (h, w), w a multiple of 4.
        frames: the list of uint8 (h_i, w_i, 3) device tensors the rows were detected on; dets (B, R, 6) fp32 / count (B) int32 in
        frame coordinates (R = 300 from detect_frames, max_out from detect_tiled).  pad: one number or (pad_y, pad_x), in [0, 16];
        max_per_frame: at most that many crops per frame, the first in row order; classes: None or the classes to crop; cap: the
        capacity of the outputs, default B * min(R, max_per_frame).  Returns (crops (cap, h, w, 3) uint8, crop_src (cap) = b * R + r,
        crop_rect (cap, 4) = x0, y0, width, height, crop_offset (B + 1), crop_skipped (B)): frame b's crops are slots crop_offset[b]
        .. crop_offset[b + 1]; slots from min(crop_offset[B], cap) on are not written, and crop_offset[B] > cap says cap was too small.
        The rule, bit for bit: include/yfv2.h; each crop equals resize_frames of its view on an engine of size out_size.  Enqueue
        only (the first call, or a larger cap, allocates the handle's descriptor table and waits once); grows max_batch like every
        batched call."""
        return self._crop_detections("crop_detections", self._frame_table, _lib.lib().yfv2_crop_detections_u8, frames, dets, count, out_size, pad,
                                     max_per_frame, classes, cap, out)

    def crop_detections_yuv(self, frames, dets, count, out_size, pad=0.0, max_per_frame=MAX_DET, classes=None, cap=None, out=None):
        """`crop_detections` for a list of yuv.YuvFrame: rectangles are relative to each frame's own rectangle, and the result is
        bit-identical to crop_detections on the converted frames."""
        return self._crop_detections("crop_detections_yuv", self._yuv_table, _lib.lib().yfv2_crop_detections_yuv, frames, dets, count, out_size, pad,
                                     max_per_frame, classes, cap, out)

    # ---- second-stage crops as network input (include/yfv2.h yfv2_crop_tensors_u8 / _yuv) ------------------------------
    @staticmethod
    def _crop_tensor(name, mean, std, rgb, letterbox, fill, dtype):
        if dtype not in (torch.float32, torch.float16):
            raise ValueError("%s: dtype must be torch.float32 or torch.float16, got %s" % (name, dtype))
        t = _lib.CropTensor()
        t.dtype, t.rgb, t.letterbox = _lib.F32 if dtype == torch.float32 else _lib.F16, int(bool(rgb)), int(bool(letterbox))
        for what, src, dst, conv in (("mean", mean, t.mean, float), ("std", std, t.std, float), ("fill", fill, t.fill, int)):
            v = [conv(a) for a in (src.tolist() if hasattr(src, "tolist") else src)]
            if len(v) != 3 or (conv is int and not all(0 <= a <= 255 for a in v)):
                raise ValueError("%s: %s must be three %s" % (name, what, "integers in 0..255" if conv is int else "numbers"))
            dst[0], dst[1], dst[2] = v
        return t, dtype

    def crop_tensors(self, frames, dets, count, out_size, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), rgb=False, letterbox=False, fill=(0, 0, 0),
                     dtype=torch.float32, pad=0.0, max_per_frame=MAX_DET, classes=None, cap=None, out=None):
        """`crop_detections` with the crops written as a second network takes them, in the same launch: (cap, 3, h, w) fp32 or fp16
        (dtype), each byte a of the crop as ((a / 255) - mean[c]) / std[c] - torchvision's ToTensor and Normalize, every operation
        rounded to fp32 on its own, then once to half for fp16.  mean / std: by OUTPUT plane; rgb: planes R, G, B instead of the frames'
        B, G, R; letterbox: keep each rectangle's aspect ratio, centred in (h, w), the rest `fill` (B, G, R bytes, which go through
        the same formula).  Everything else - frames, dets, count, pad, max_per_frame, classes, cap - as crop_detections, and
        crop_src, crop_rect, crop_offset, crop_skipped are what it returns.  Returns (tensors, crop_src, crop_rect, crop_offset,
        crop_skipped).  The rule, bit for bit: include/yfv2.h; with letterbox=False the bytes behind the values are crop_detections'
        crops.  No uint8 crop is written.  Frames may be somewhat narrower than for crop_detections (the row is staged as three
        planes of w values).  Enqueue only."""
        return self._crop_detections("crop_tensors", self._frame_table, _lib.lib().yfv2_crop_tensors_u8, frames, dets, count, out_size, pad,
                                     max_per_frame, classes, cap, out, self._crop_tensor("crop_tensors", mean, std, rgb, letterbox, fill, dtype))

    def crop_tensors_yuv(self, frames, dets, count, out_size, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), rgb=False, letterbox=False,
                         fill=(0, 0, 0), dtype=torch.float32, pad=0.0, max_per_frame=MAX_DET, classes=None, cap=None, out=None):
        """`crop_tensors` for a list of yuv.YuvFrame: bit-identical to crop_tensors on the converted frames."""
        return self._crop_detections("crop_tensors_yuv", self._yuv_table, _lib.lib().yfv2_crop_tensors_yuv, frames, dets, count, out_size, pad,
                                     max_per_frame, classes, cap, out, self._crop_tensor("crop_tensors_yuv", mean, std, rgb, letterbox, fill, dtype))

    # ---- identity across frames: the per-stream IoU tracker (include/yfv2.h yfv2_track_update) -------------------
    def track_update(self, dets, count, streams, state, max_tracks, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30,
                     confirm_hits=3, fresh=False, out=None):
        """One update of a tracker's device state from a batch of detection rows (tracking.Tracker owns the state and calls this).
        dets (B, R, 6) fp32 / count (B) int32 on the device, in detect_frames' / detect_tiled's layout; streams: B distinct stream
        indices (host ints), frame b belongs to stream streams[b]; state: contiguous int32 (S, 8 + 10 * max_tracks) on the device,
        all zero = empty, updated in place.  Returns (track_id (B, R), track_hits (B, R)) int32 - 0 where a row has no track - and,
        with fresh=True, also (fresh_dets (B, R, 6), fresh_src (B, R), fresh_count (B)): the rows whose track reached confirm_hits in
        this frame, compacted in row order, which is the (dets, count) pair crop_detections takes.  out: the same tuple, preallocated.
        The rule, bit for bit: include/yfv2.h.  Enqueue only: one launch, no host wait."""
        rule = (match_thres, class_aware, init_conf, max_misses, confirm_hits)
        return tracking.update(self, "track_update", dets, count, streams, state, max_tracks, rule, fresh=fresh, out=out)

    def track_update_two_pass(self, dets, count, streams, state, max_tracks, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30,
                              confirm_hits=3, high_conf=_TWO["high_conf"], low_conf=_TWO["low_conf"], match_thres_low=_TWO["match_thres_low"],
                              tracked_only=_TWO["tracked_only"], motion=None, fresh=False, box=False, passes=False, out=None):
        """track_update / track_update_motion with two association passes (include/yfv2.h yfv2_track_update_two_pass):
        the rows with conf >= high_conf are matched first, the rows with low_conf <= conf < high_conf are then offered to the tracks
        still unmatched (tracked_only: only to those that were matched in their last frame) with IoU > match_thres_low, and start no
        track; rows below low_conf take no part.  motion: None - state is the plain (S, 8 + 10 * max_tracks); True or a dict with any
        of std_pos, std_vel, std_meas - the motion form's (S, 8 + 32 * max_tracks), and box=True is allowed.  Returns what the
        one-pass call of the layout returns and, with passes=True, last of all track_pass (B, R) int32: 1 for a row matched in the
        first pass or born, 2 for a row matched in the second pass, 0 for a row without a track."""
        name = "track_update_two_pass"
        motion = tracking.option(name, "motion", motion, _MOT)
        if box and motion is None:
            raise ValueError(name + ": box=True needs motion")
        rule = (match_thres, class_aware, init_conf, max_misses, confirm_hits)
        second = dict(high_conf=high_conf, low_conf=low_conf, match_thres_low=match_thres_low, tracked_only=tracked_only)
        return tracking.update(self, name, dets, count, streams, state, max_tracks, rule, motion=motion, second=second, fresh=fresh, box=box,
                               passes=passes, out=out)

    def track_update_motion(self, dets, count, streams, state, max_tracks, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30,
                            confirm_hits=3, std_pos=_MOT["std_pos"], std_vel=_MOT["std_vel"], std_meas=_MOT["std_meas"], fresh=False, box=False, out=None):
        """track_update with a motion model (include/yfv2.h yfv2_track_update_motion): every track carries a
        constant-velocity Kalman filter per coordinate cx, cy, w, h, a row is matched against the box the filter PREDICTS, and a track
        that is not seen coasts.  state: contiguous int32 (S, 8 + 32 * max_tracks).  std_pos, std_vel, std_meas: the filter's noise
        scales, relative to the track's width / height (finite, > 0).  Returns what track_update returns and, with box=True, after
        it track_box (B, R, 4) fp32: the filtered corners of each row's track, zero where a row has none."""
        rule = (match_thres, class_aware, init_conf, max_misses, confirm_hits)
        motion = dict(std_pos=std_pos, std_vel=std_vel, std_meas=std_meas)
        return tracking.update(self, "track_update_motion", dets, count, streams, state, max_tracks, rule, motion=motion, fresh=fresh, box=box, out=out)

    def track_update_appearance(self, dets, count, emb, streams, state, feat, max_tracks, match_thres=0.3, class_aware=True, init_conf=0.0,
                                max_misses=30, confirm_hits=3, dim=_APP["dim"], prox_thres=_APP["prox_thres"], app_thres=_APP["app_thres"], alpha=_APP["alpha"],
                                motion=None, two_pass=None, fresh=False, box=False, passes=False, cos=False, out=None):
        """The update of any layout and pass form with appearance association (include/yfv2.h yfv2_track_update_appearance;
        DESIGN.md 4.22).  emb: contiguous fp32 (B, R, dim) on the device, row r's embedding (a re-identification network's output for
        the row's crop; not necessarily normalised); feat: contiguous int32 (S, max_tracks * (4 + dim)), all zero = empty, the
        tracks' features, updated in place.  A first-pass edge whose IoU is above prox_thres takes the cosine of the row's embedding
        with the track's feature as its value when that is above app_thres and above the IoU; a matched row's embedding is blended
        into the feature with momentum alpha.  motion: None, True or a dict as for track_update_two_pass; two_pass: None - one pass -
        or True or a dict with any of high_conf, low_conf, match_thres_low, tracked_only.  Returns what the call of that layout and
        pass form returns (passes=True only with two_pass, box=True only with motion) and, with cos=True, last of all track_cos
        (B, R) fp32: the cosine of each matched row with its track's feature before this update, 0 elsewhere."""
        name = "track_update_appearance"
        motion = tracking.option(name, "motion", motion, _MOT)
        if box and motion is None:
            raise ValueError(name + ": box=True needs motion")
        second = tracking.option(name, "two_pass", two_pass, _TWO)
        if passes and second is None:
            raise ValueError(name + ": passes=True needs two_pass")
        dim = int(dim)
        if dim < 16 or dim > 2048 or dim % 16:
            raise ValueError(name + ": dim must be a multiple of 16 in 16..2048")
        rule = (match_thres, class_aware, init_conf, max_misses, confirm_hits)
        appearance = dict(dim=dim, prox_thres=prox_thres, app_thres=app_thres, alpha=alpha)
        return tracking.update(self, name, dets, count, streams, state, max_tracks, rule, motion=motion, second=second, appearance=appearance, emb=emb,
                               feat=feat, fresh=fresh, box=box, passes=passes, cos=cos, out=out)

    # ---- the ncnn sample's deployment path (include/yfv2.h yfv2_export_maps / yfv2_deploy_post) ------------------
    def map_shapes(self, B):
        C5 = 5 * self.anchor_num + self.classes
        return [(B, self.height // 16, self.width // 16, C5), (B, self.height // 32, self.width // 32, C5)]

    def export_maps(self, preds, out=None):
        """The six NCHW logit maps of forward() -> the two NHWC maps of Detector(export_onnx=True) (model/detector.py:33-44):
        (B, H/16, W/16, 15 + classes) and (B, H/32, W/32, 15 + classes), sigmoid(reg) | sigmoid(obj) | softmax(classes), in one launch.
        The obj and class channels are bit-identical to decode()'s columns 4 and 5.. .  Enqueue only."""
        preds = [p.contiguous() for p in preds]
        B = preds[0].shape[0]
        for p, s in zip(preds, self.logit_shapes(B)):
            if tuple(p.shape) != s or p.dtype != torch.float32 or p.device != self.device:
                raise ValueError("logit tensor %s %s on %s, expected fp32 %s on %s" % (p.dtype, tuple(p.shape), p.device, s, self.device))
        self.ensure_batch(B)
        if out is None:
            out = [torch.empty(s, device=self.device, dtype=torch.float32) for s in self.map_shapes(B)]
        for m, s in zip(out, self.map_shapes(B)):
            if tuple(m.shape) != s or m.dtype != torch.float32 or m.device != self.device or not m.is_contiguous():
                raise ValueError("out must be two contiguous fp32 tensors %s on %s" % (self.map_shapes(B), self.device))
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in preds])
        check(_lib.lib().yfv2_export_maps(self._h, ptrs, B, _ptr(out[0]), _ptr(out[1]), _stream(self.device)), self._h)
        return tuple(out)

    def new_deploy_buffers(self, B, max_out=None):
        """(boxes (B, max_out, 6) int32, count (B) int32) for deploy_post / detect_deploy_frames.  A record is yfv2_target_box: x1, y1,
        x2, y2, cate as int32 and the fp32 score's bits in column 5 (boxes[..., 5].view(torch.float32))."""
        max_out = self.rows if max_out is None else int(max_out)
        return (torch.empty((B, max_out, 6), device=self.device, dtype=torch.int32), torch.empty((B,), device=self.device, dtype=torch.int32))

    def _deploy_out(self, out, B, max_out):
        max_out = self.rows if max_out is None else int(max_out)
        if not 1 <= max_out <= self.rows:
            raise ValueError("max_out must be in 1..%d, got %d" % (self.rows, max_out))
        if out is None:
            return self.new_deploy_buffers(B, max_out) + (max_out,)
        boxes, cnt = out
        for t, shape in ((boxes, (B, max_out, 6)), (cnt, (B,))):
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous():
                raise ValueError("out must be contiguous int32 (boxes %s, count %s) on %s" % ((B, max_out, 6), (B,), self.device))
        return boxes, cnt, max_out

    def deploy_post(self, map0, map1, thresh=0.3, nms_thresh=0.25, scale=None, max_out=None, out=None):
        """The ncnn sample's predHandle + nmsHandle (sample/ncnn/src/yolo-fastestv2.cpp:58-183) on two export maps, for the whole
        batch in one launch: score = cls * obj > thresh, boxes scaled by `scale` ((B, 2) fp32 scaleW, scaleH on the device; None = 1)
        and truncated to int, greedy NMS on the integer boxes per class, no limit of 300; equal scores rank by row order.  Returns
        (boxes (B, max_out, 6) int32, count (B)): count is the full number of survivors, records beyond min(count, max_out) are
        zero.  Uses the engine's anchors (rounded to fp32, as the sample holds them).  Enqueue only; dropped() afterwards."""
        self._need_anchors("deploy_post")
        B = int(map0.shape[0])
        for m, s in zip((map0, map1), self.map_shapes(B)):
            if not torch.is_tensor(m) or tuple(m.shape) != s or m.dtype != torch.float32 or m.device != self.device:
                raise ValueError("maps must be fp32 %s on %s" % (self.map_shapes(B), self.device))
        map0, map1 = map0.contiguous(), map1.contiguous()
        if scale is not None:
            if not torch.is_tensor(scale) or tuple(scale.shape) != (B, 2) or scale.dtype != torch.float32 or scale.device != self.device:
                raise ValueError("scale must be an fp32 (%d, 2) tensor on %s" % (B, self.device))
            scale = scale.contiguous()
        self.ensure_batch(B)
        boxes, cnt, max_out = self._deploy_out(out, B, max_out)
        check(_lib.lib().yfv2_deploy_post(self._h, _ptr(map0), _ptr(map1), B, _ptr(scale) if scale is not None else None, float(thresh),
                                          float(nms_thresh), _ptr(boxes), _ptr(cnt), max_out, _stream(self.device)), self._h)
        return boxes, cnt

    def deploy_dropped(self):
        """Waits for the stream; the number of candidates the LAST deploy_post / detect_deploy_frames dropped because their box is
        not representable as int32 (non-finite reg values: the sample's (int) is undefined there).  0 for sane maps."""
        n = C.c_int32(0)
        check(_lib.lib().yfv2_deploy_dropped(self._h, C.byref(n), _stream(self.device)), self._h)
        return int(n.value)

    def detect_deploy_frames(self, frames, thresh=0.3, nms_thresh=0.25, max_out=None, out=None, check=True):
        """The ncnn sample's detection() (yolo-fastestv2.cpp:185-221) for a list of uint8 (h_i, w_i, 3) device frames of any sizes:
        resize_frames -> forward -> export_maps -> deploy_post with scaleW = fp32(w_i) / fp32(width), scaleH likewise, in one call and
        bit-identical to those four.  The resize is cv2's bilinear arithmetic, not ncnn's from_pixels_resize.  Returns (boxes, count)
        like deploy_post.  Enqueue only (the first call on a handle allocates its workspaces and waits once); check= as in detect()."""
        self._need_anchors("detect_deploy_frames")
        if check and self.peek_nonfinite():
            self.check_finite("detect_deploy_frames (an earlier call on this handle)")
        arr, keep = self._frame_table(frames)
        B = len(keep)
        self.ensure_batch(B)
        boxes, cnt, max_out = self._deploy_out(out, B, max_out)
        _lib.check(_lib.lib().yfv2_detect_deploy_frames_u8(self._h, arr, B, float(thresh), float(nms_thresh), _ptr(boxes), _ptr(cnt), max_out,
                                                           _stream(self.device)), self._h)
        return boxes, cnt

    def batch_statistics(self, dets, cnt, targets, iou_threshold, sync=True):
        """True-positive flags (B, 300) int32 for the padded detections of nms()/detect() against targets (T,6)
        [image index, label, x1, y1, x2, y2] - utils/utils.py:194-230 get_batch_statistics on the device.
        ``sync=False`` only enqueues (no host wait); call ``stats_overflowed()`` once after the last batch."""
        B = dets.shape[0]
        if tuple(dets.shape) != (B, MAX_DET, 6) or dets.dtype != torch.float32 or dets.device != self.device:
            raise ValueError("dets must be fp32 (B,%d,6) on %s" % (MAX_DET, self.device))
        targets = targets.to(self.device, torch.float32).reshape(-1, 6).contiguous()
        tp = torch.empty((B, MAX_DET), device=self.device, dtype=torch.int32)
        fn = _lib.lib().yfv2_batch_statistics if sync else _lib.lib().yfv2_batch_statistics_async
        check(fn(self._h, _ptr(dets.contiguous()), _ptr(cnt.contiguous()), B, _ptr(targets) if targets.numel() else None,
                 int(targets.shape[0]), float(iou_threshold), _ptr(tp), _stream(self.device)), self._h)
        return tp

    def batch_statistics_multi(self, dets, cnt, targets, thresholds, sync=True):
        """``batch_statistics`` at K = len(thresholds) IoU thresholds (1..32, any floats in any order) in one launch
        (include/yfv2.h yfv2_batch_statistics_multi): an int32 (B, 300) tensor whose bit k is exactly the flag ``batch_statistics``
        returns at ``thresholds[k]``; bits at and above K are 0 (so bit 31, the sign, is set only where K = 32).  ``sync`` as there."""
        import numpy as np
        B = dets.shape[0]
        if tuple(dets.shape) != (B, MAX_DET, 6) or dets.dtype != torch.float32 or dets.device != self.device:
            raise ValueError("dets must be fp32 (B,%d,6) on %s" % (MAX_DET, self.device))
        thr = np.ascontiguousarray(np.asarray(thresholds, np.float32).reshape(-1))
        K = int(thr.shape[0])
        targets = targets.to(self.device, torch.float32).reshape(-1, 6).contiguous()
        mask = torch.empty((B, MAX_DET), device=self.device, dtype=torch.int32)
        fn = _lib.lib().yfv2_batch_statistics_multi if sync else _lib.lib().yfv2_batch_statistics_multi_async
        check(fn(self._h, _ptr(dets.contiguous()), _ptr(cnt.contiguous()), B, _ptr(targets) if targets.numel() else None,
                 int(targets.shape[0]), thr.ctypes.data_as(C.POINTER(C.c_float)) if K else None, K, _ptr(mask), _stream(self.device)), self._h)
        return mask

    def loss(self, preds, targets, want_grad=False):
        """utils/loss.py:130-208 compute_loss on the device: (losses, grads) with losses a float32 (4,) device tensor
        [lbox, lobj, lcls, total] and grads the gradients of `total` w.r.t. the six logit maps (None unless want_grad)."""
        self._need_anchors("loss")
        preds = [p.detach().contiguous() for p in preds]
        B = preds[0].shape[0]
        for p, s in zip(preds, self.logit_shapes(B)):
            if tuple(p.shape) != s or p.dtype != torch.float32 or p.device != self.device:
                raise ValueError("logit tensor %s %s on %s, expected fp32 %s on %s" % (p.dtype, tuple(p.shape), p.device, s, self.device))
        self.ensure_batch(B)
        targets = torch.as_tensor(targets).to(self.device, torch.float32).reshape(-1, 6).contiguous()
        losses = torch.empty(4, device=self.device, dtype=torch.float32)
        grads = [torch.empty_like(p) for p in preds] if want_grad else None
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in preds])
        gptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in grads]) if want_grad else None
        check(_lib.lib().yfv2_loss(self._h, ptrs, B, _ptr(targets) if targets.numel() else None, int(targets.shape[0]), _ptr(losses),
                                   gptrs, _stream(self.device)), self._h)
        return losses, grads

    # ---- anchors from a label set: genanchors.py:67-102 on the device -------------------------------------------------
    def anchor_kmeans(self, wh, centroids, max_iter=1000, want_assign=True):
        """IoU k-means over label sizes (include/yfv2.h yfv2_anchor_kmeans): ``wh`` (N, 2) and ``centroids`` (k, 2) float64 tensors
        on this engine's device, ``centroids`` = the initial ones (not modified).  Returns ``(centroids, assign, avg_iou, info)``:
        the final (k, 2) centroids in the reference's order (unsorted), the (N,) int32 assignments (None unless ``want_assign``),
        the average IoU as a 0-d float64 device tensor and ``info`` = dict(iterations, converged, empty_cluster, bad_input).
        Waits for the stream.  Needs no weights and no anchors."""
        for name, t in (("wh", wh), ("centroids", centroids)):
            if not torch.is_tensor(t) or t.dtype != torch.float64 or t.device != self.device or t.dim() != 2 or t.shape[1] != 2:
                raise ValueError("%s must be a float64 (n, 2) tensor on %s" % (name, self.device))
        wh = wh.contiguous()
        cent = centroids.contiguous().clone()
        N, k = int(wh.shape[0]), int(cent.shape[0])
        assign = torch.empty(max(N, 1), device=self.device, dtype=torch.int32)[:N] if want_assign else None
        avg = torch.zeros((), device=self.device, dtype=torch.float64)
        info = _lib.KmeansInfo()
        info.struct_size = C.sizeof(_lib.KmeansInfo)
        check(_lib.lib().yfv2_anchor_kmeans(self._h, _ptr(wh) if N else None, N, _ptr(cent) if k else None, k, int(max_iter),
                                            _ptr(assign) if want_assign else None, _ptr(avg), C.byref(info), _stream(self.device)), self._h)
        return cent, assign, avg, {"iterations": int(info.iterations), "converged": int(info.converged),
                                   "empty_cluster": int(info.empty_cluster), "bad_input": int(info.bad_input)}

    def debug_kmeans_group(self, group):
        """Test hook: passes anchor_kmeans enqueues between two looks at the verdict (1..64, default 8); changes no output bit."""
        check(_lib.lib().yfv2_debug_kmeans_group(self._h, int(group)), self._h)

    # ---- average precision over a validation set: utils/utils.py:110-192 on the device ----------------------------------
    def ap_per_class(self, tp, conf, pred_cls, target_cls):
        """Per-class precision, recall and average precision (include/yfv2.h yfv2_ap_per_class): ``tp`` (N) int32, ``conf`` and
        ``pred_cls`` (N) float32, ``target_cls`` (T) float32, all tensors on this engine's device.  Returns a dict of numpy arrays
        indexed by class 0..255 - ``p``, ``r``, ``ap`` (float64), ``n_gt``, ``n_pred`` (int64) - with ``present`` (the ascending
        classes of target_cls), ``bad_input`` and ``means`` = (mean_p, mean_r, mean_ap, mean_f1) added class after class by the
        library.  Equal confidences rank by input index (np.argsort(-conf, kind="stable")).  Waits for the stream."""
        want = (("tp", tp, torch.int32), ("conf", conf, torch.float32), ("pred_cls", pred_cls, torch.float32), ("target_cls", target_cls, torch.float32))
        for name, t, dt in want:
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self.device or t.dim() != 1:
                raise ValueError("%s must be a 1-d %s tensor on %s" % (name, dt, self.device))
        tp, conf, pred_cls, target_cls = tp.contiguous(), conf.contiguous(), pred_cls.contiguous(), target_cls.contiguous()
        N, T = int(tp.shape[0]), int(target_cls.shape[0])
        if int(conf.shape[0]) != N or int(pred_cls.shape[0]) != N:
            raise ValueError("tp, conf and pred_cls must have one length (got %d, %d, %d)" % (N, conf.shape[0], pred_cls.shape[0]))
        res = _lib.ApResult()
        res.struct_size = C.sizeof(_lib.ApResult)
        check(_lib.lib().yfv2_ap_per_class(self._h, _ptr(tp) if N else None, _ptr(conf) if N else None, _ptr(pred_cls) if N else None, N,
                                           _ptr(target_cls) if T else None, T, C.byref(res), _stream(self.device)), self._h)
        return _ap_dict(res)

    def ap_per_class_multi(self, tpmask, conf, pred_cls, target_cls, K):
        """``ap_per_class`` at K thresholds in one pass (include/yfv2.h yfv2_ap_per_class_multi): ``tpmask`` (N) int32, bit k = tp at
        threshold k (what ``batch_statistics_multi`` returns, flattened); bits at and above K are ignored.  Returns a list of K dicts
        shaped like ``ap_per_class``'s; entry k equals ``ap_per_class`` on ``(tpmask >> k) & 1`` bit for bit.  The definition is the
        reference's ap_per_class at each threshold: no 101-point interpolation, no crowd flags, no area ranges.  Waits for the stream."""
        want = (("tpmask", tpmask, torch.int32), ("conf", conf, torch.float32), ("pred_cls", pred_cls, torch.float32), ("target_cls", target_cls, torch.float32))
        for name, t, dt in want:
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self.device or t.dim() != 1:
                raise ValueError("%s must be a 1-d %s tensor on %s" % (name, dt, self.device))
        tpmask, conf, pred_cls, target_cls = tpmask.contiguous(), conf.contiguous(), pred_cls.contiguous(), target_cls.contiguous()
        N, T, K = int(tpmask.shape[0]), int(target_cls.shape[0]), int(K)
        if int(conf.shape[0]) != N or int(pred_cls.shape[0]) != N:
            raise ValueError("tpmask, conf and pred_cls must have one length (got %d, %d, %d)" % (N, conf.shape[0], pred_cls.shape[0]))
        res = (_lib.ApResult * max(K, 1))()
        for r in res:
            r.struct_size = C.sizeof(_lib.ApResult)
        check(_lib.lib().yfv2_ap_per_class_multi(self._h, _ptr(tpmask) if N else None, _ptr(conf) if N else None, _ptr(pred_cls) if N else None, N,
                                                 _ptr(target_cls) if T else None, T, K, res, _stream(self.device)), self._h)
        return [_ap_dict(r) for r in res]

    # ---- training path: train.py:96-123 on the device -----------------------------------------
    def train_bind(self, tensors, grads):
        """tensors: name -> fp32 device tensor for every floating-point state_dict entry (weights, biases, BatchNorm running
        statistics); grads: name -> fp32 device buffer for every trainable parameter.  The library keeps the POINTERS."""
        def table(d):
            arr = (TensorDesc * len(d))()
            for i, (k, t) in enumerate(d.items()):
                if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError("train_bind: '%s' must be a contiguous fp32 tensor on %s" % (k, self.device))
                arr[i].name, arr[i].data, arr[i].numel = k.encode(), t.data_ptr(), t.numel()
            return arr
        self._train_keep = (tensors, grads)          # the tensors must outlive the binding
        ta, ga = table(tensors), table(grads)
        check(_lib.lib().yfv2_train_bind(self._h, ta, len(tensors), ga, len(grads)), self._h)

    def train_forward(self, x, out=None):
        """Detector.forward in train() mode (batch-statistics BatchNorm; running statistics updated in the bound buffers)."""
        x = self._check_x(x)
        if x.dtype != torch.float32:
            raise ValueError("train_forward takes the fp32 (B,3,H,W) tensor train.py:101 builds")
        B = x.shape[0]
        if out is None:
            out = [torch.empty(s, device=self.device, dtype=torch.float32) for s in self.logit_shapes(B)]
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in out])
        check(_lib.lib().yfv2_train_forward(self._h, _ptr(x), B, ptrs, _stream(self.device)), self._h)
        self._train_seq = getattr(self, "_train_seq", 0) + 1
        # the library does NOT copy the input: the backward's first-conv weight gradient re-reads it through the raw pointer
        # (yfv2_train.hip).  `x` may be a temporary made here (contiguous() / clone()) or by the caller: hold it until the next
        # train-mode forward replaces the tape, or the caching allocator hands the block to somebody else before backward runs
        self._train_x = x
        return tuple(out)

    def train_backward(self, grads6):
        """From the gradient of the loss w.r.t. the six logit maps down to every parameter: ADDS into the bound gradient buffers."""
        gs = [g.to(self.device, torch.float32).contiguous() for g in grads6]
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in gs])
        check(_lib.lib().yfv2_train_backward(self._h, ptrs, _stream(self.device)), self._h)

    def debug_train_relu_output(self, conv_name):
        """flat host tensor (B*C*H*W, NCHW order): what the ReLU after conv `conv_name` wrote in the last train_forward"""
        L = _lib.lib()
        n = L.yfv2_debug_train_relu_output(self._h, conv_name.encode(), None, 0)
        if n < 0:
            check(-1, self._h)
        host = torch.empty(n, dtype=torch.float32)
        if L.yfv2_debug_train_relu_output(self._h, conv_name.encode(), C.c_void_p(host.data_ptr()), n) != n:
            check(-1, self._h)
        return host

    TRAIN_TENSOR = {"y": 0, "out": 1, "grad_y": 2, "grad_out": 3, "mean": 4, "invstd": 5}

    def debug_train_tensor(self, name, which):
        """flat host tensor: one tensor of the training arenas after the last train_forward / train_backward (include/yfv2.h
        yfv2_debug_train_tensor).  name: a conv's state_dict prefix, or "backbone.maxpool", "backbone.stageS.I", "fpn.p2";
        which: "y", "out", "grad_y", "grad_out", "mean", "invstd" (or the number)"""
        L = _lib.lib()
        w = self.TRAIN_TENSOR[which] if isinstance(which, str) else int(which)
        n = L.yfv2_debug_train_tensor(self._h, name.encode(), w, None, 0)
        if n < 0:
            check(-1, self._h)
        host = torch.empty(n, dtype=torch.float32)
        if L.yfv2_debug_train_tensor(self._h, name.encode(), w, C.c_void_p(host.data_ptr()), n) != n:
            check(-1, self._h)
        return host

    def sgd_step(self, param, grad, buf, lr, momentum, weight_decay, first):
        check(_lib.lib().yfv2_sgd_step(self._h, _ptr(param), _ptr(grad), _ptr(buf), param.numel(), float(lr), float(momentum), float(weight_decay),
                                       1 if first else 0, _stream(self.device)), self._h)

    def sgd_step_multi(self, items, lr, momentum, weight_decay):
        """items: a prepared (SgdItem * n) table (see utils/optim.py) - one entry per parameter tensor, a few launches in all."""
        check(_lib.lib().yfv2_sgd_step_multi(self._h, items, len(items), float(lr), float(momentum), float(weight_decay), _stream(self.device)), self._h)

    def stats_overflowed(self):
        """Waits for the stream; True if any batch_statistics(sync=False) call since the last query met an image with
        more than 1024 targets (its flags are then invalid).  Clears the flag."""
        over = C.c_int32(0)
        check(_lib.lib().yfv2_batch_statistics_overflow(self._h, C.byref(over), _stream(self.device)), self._h)
        return bool(over.value)

    def nonfinite(self):
        """Waits for the stream; True if any forward / detect on this handle since the last query tripped the range guard of the
        fp16x3 plan (an activation beyond +-4094, an fp32 input beyond +-255.9, or a non-finite value: include/yfv2.h
        yfv2_nonfinite).  Clears the word."""
        flag = C.c_int32(0)
        check(_lib.lib().yfv2_nonfinite(self._h, C.byref(flag), _stream(self.device)), self._h)
        return bool(flag.value)

    def peek_nonfinite(self):
        """True if a kernel that has ALREADY COMPLETED on this handle tripped the range guard; waits for nothing, clears nothing."""
        flag = C.c_int32(0)
        check(_lib.lib().yfv2_nonfinite_peek(self._h, C.byref(flag)), self._h)
        return bool(flag.value)

    def clock_probe_begin(self, workgroups=256, milliseconds=50.0, busy=True):
        """Enqueue the shader-clock probe on the CURRENT stream (include/yfv2.h yfv2_clock_probe_begin)."""
        check(_lib.lib().yfv2_clock_probe_begin(self._h, int(workgroups), float(milliseconds), 1 if busy else 0, _stream(self.device)), self._h)

    def clock_probe_end(self):
        """Waits for the current stream; dict with the effective shader clock (MHz) min / mean / max over the probe's workgroups."""
        out = (C.c_double * 6)()
        check(_lib.lib().yfv2_clock_probe_end(self._h, out, _stream(self.device)), self._h)
        return {"sclk_mhz_min": round(out[0], 1), "sclk_mhz_mean": round(out[1], 1), "sclk_mhz_max": round(out[2], 1),
                "ref_clock_mhz": round(out[3], 3), "interval_ms": round(out[4], 3), "xcds_seen": int(out[5])}

    def check_finite(self, what="forward"):
        """Raise if the range guard tripped (call where the host waits for the device anyway)."""
        if self.nonfinite():
            raise _lib.Yfv2Error(_lib.ERR_RANGE, "%s: an activation left the range of the default (fp16x3) plan - |activation| >= 4094 or a non-finite "
                                     "input; the result is invalid.  Create the handle on the fp32-matrix plan - Engine(..., plan={'fp32_matrix': 1}), "
                                     "yfv2_plan.fp32_matrix = 1, or YFV2_BF6=0 in the environment of the Python layer (every conv on the fp32 matrix "
                                     "instructions, no such bound) - for this model / input" % what)

    # ---- introspection --------------------------------------------------------------------
    def stages(self):
        L = _lib.lib()
        n = L.yfv2_num_stages(self._h)
        out = []
        buf = C.create_string_buffer(256)
        for i in range(n):
            fl, by, ex = C.c_double(), C.c_double(), C.c_double()
            check(L.yfv2_stage_info(self._h, i, buf, 256, C.byref(fl), C.byref(by), C.byref(ex)), self._h)
            st = {"name": buf.value.decode(), "flops_per_image": fl.value, "bytes_per_image": by.value, "external_bytes_per_image": ex.value}
            check(L.yfv2_stage_kernel(self._h, i, buf, 256), self._h)
            st["kernel"] = buf.value.decode()
            out.append(st)
        return out

    def profile_forward(self, x, iters=5):
        """Per-launch mean milliseconds (hipEvent pairs on the current stream)."""
        x = self._check_x(x)
        B = x.shape[0]
        self.ensure_batch(B)
        out = [torch.empty(s, device=self.device, dtype=torch.float32) for s in self.logit_shapes(B)]
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in out])
        n = _lib.lib().yfv2_num_stages(self._h)
        ms = (C.c_float * n)()
        check(_lib.lib().yfv2_profile_forward(self._h, _ptr(x), B, ptrs, int(iters), ms, _stream(self.device)), self._h)
        return list(ms)

    def debug_activation(self, which, B):
        """NHWC activation of the last forward: 0 stem+pool, 1 stage2, 2 C2, 3 C3, 4 S2, 5 S3.
        (0: the default plan runs the stem and stage2.0 as ONE launch that never writes the stem's output - the hook then re-runs the
        stem's own launch on the LAST forward's input, which the caller must still hold.)"""
        L = _lib.lib()
        n = L.yfv2_debug_activation(self._h, which, B, None, 0)
        if n < 0:
            check(int(n), self._h)
        host = torch.empty(n, dtype=torch.float32)
        got = L.yfv2_debug_activation(self._h, which, B, C.c_void_p(host.data_ptr()), n)
        if got < 0:
            check(int(got), self._h)
        return host


def unpack_detections(dets, idx, cnt):
    """(B,300,6),(B,300),(B) device tensors -> (list of (n_i,6) CPU tensors, list of (n_i,) CPU index tensors).
    One D2H copy per tensor (not per image)."""
    cnt_h = cnt.cpu()
    dets_h, idx_h = dets.cpu(), idx.cpu()
    rows, ids = [], []
    for b in range(cnt_h.shape[0]):
        n = int(cnt_h[b])
        rows.append(dets_h[b, :n].clone())
        ids.append(idx_h[b, :n].to(torch.int64))
    return rows, ids


_engines = {}


def get_engine(device, height, width, classes=80, anchor_num=3):
    """Process-wide engine cache: one handle per (device, H, W, classes)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), int(height), int(width), int(classes), int(anchor_num))
    eng = _engines.get(key)
    if eng is None:
        eng = Engine(device, height, width, classes, anchor_num)
        _engines[key] = eng
    return eng
