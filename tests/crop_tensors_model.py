"""The numpy statement of the crop-tensor rule (include/yfv2.h "second-stage crops as network input"; the library's functions of it
are yfv2_crop_letterbox_inner and yfv2_crop_tensor_f32 / _f16, yfv2_internal.h).  Selection, numbering and rectangles are
crops_model's; this file is the geometry (Python integers: exact), the byte image (the oracle's resize on a canvas of fill) and
the value (np.float32 operations, each rounded on its own; .astype(np.float16) rounds to nearest even)."""
import numpy as np

from oracle import yfv2_oracle as oracle


def letterbox(cw, ch, out_h, out_w, letterbox):
    """-> (ox0, oy0, iw, ih): where a cw x ch rectangle lands in the (out_h, out_w) output"""
    cw, ch, H, W = int(cw), int(ch), int(out_h), int(out_w)
    if not letterbox:
        return 0, 0, W, H
    if W * ch <= H * cw:
        iw, ih = W, max(1, (2 * ch * W + cw) // (2 * cw))
    else:
        iw, ih = max(1, (2 * cw * H + ch) // (2 * ch)), H
    return (W - iw) >> 1, (H - ih) >> 1, iw, ih


def value(a, mean, std):
    """bytes a (any shape), fp32 mean and std (broadcastable) -> the fp32 values: x = a / 255; v = (x - mean) / std"""
    with np.errstate(over="ignore"):
        x = np.asarray(a).astype(np.float32) / np.float32(255.0)
        return ((x - np.float32(mean)).astype(np.float32) / np.float32(std)).astype(np.float32)


def to_dtype(v, half):
    with np.errstate(over="ignore"):
        return v.astype(np.float16) if half else v


def byte_image(view, out_h, out_w, lb, fill):
    """view (ch, cw, 3) uint8 -> the (out_h, out_w, 3) byte image that defines the bits"""
    ox0, oy0, iw, ih = letterbox(view.shape[1], view.shape[0], out_h, out_w, lb)
    img = np.empty((out_h, out_w, 3), np.uint8)
    img[:] = np.asarray(fill, np.uint8)
    img[oy0:oy0 + ih, ox0:ox0 + iw] = oracle.resize_linear_u8(np.ascontiguousarray(view), iw, ih)
    return img


def from_bytes(img, mean, std, rgb, half):
    """(..., H, W, 3) byte images -> (..., 3, H, W): plane c is byte channel 2 - c when rgb, with mean[c], std[c]"""
    img = np.asarray(img)
    planes = np.moveaxis(img[..., ::-1] if rgb else img, -1, -3)
    m = np.asarray(mean, np.float32).reshape(3, 1, 1)
    s = np.asarray(std, np.float32).reshape(3, 1, 1)
    return to_dtype(value(planes, m, s), half)


def tensors(host_frames, plan, out_size, mean=(0, 0, 0), std=(1, 1, 1), rgb=False, lb=False, fill=(0, 0, 0), half=False):
    """host_frames: the B, G, R frames; plan: crops_model.plan's dict -> (live, 3, H, W) fp32 or fp16"""
    H, W = out_size
    out = np.empty((len(plan["frame"]), 3, H, W), np.float16 if half else np.float32)
    for k, (b, (x0, y0, w, h)) in enumerate(zip(plan["frame"].tolist(), plan["rect"].tolist())):
        out[k] = from_bytes(byte_image(host_frames[b][y0:y0 + h, x0:x0 + w], H, W, lb, fill), mean, std, rgb, half)
    return out


def bits(a):
    """the raw bits of an fp32 / fp16 array, for exact comparison (NaN-safe, -0 != +0)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)
