"""The rule of yfv2_deploy_post (include/yfv2.h) restated in numpy: the ncnn sample's predHandle + nmsHandle
(sample/ncnn/src/yolo-fastestv2.cpp:58-183) over two export maps.  Written from the statement of the rule, with every rounding
explicit (np.float32 / np.float64 / np.trunc) and a STABLE sort: equal scores rank by candidate order (scale 0 then 1; h, w,
anchor), the one point the sample's std::sort leaves open.  tests/golden/golden_deploy.npz holds what the compiled sample itself
returns on tie-free inputs; test_deploy_host.py checks this model against it, test_gpu_deploy.py the kernel against both.
"""
import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32


def candidates(m, scale_index, anchors, in_h, thresh, scale_w, scale_h):
    """one map (fh, fw, 15 + classes) fp32 -> (boxes (n, 4) int32, cate (n,) int32, score (n,) fp32, dropped) in row order"""
    fh, fw, C = m.shape
    stride = int(in_h) // fh                                           # :146 integer division
    v = np.ascontiguousarray(m, F32).reshape(fh * fw, C)
    obj = v[:, 12:15]                                                  # objScore = values[4 * numAnchor + b]
    with np.errstate(all="ignore"):
        prod = (v[:, None, 15:] * obj[:, :, None]).astype(F32)         # clsScore *= objScore, fp32: (cells, 3, classes)
    above = prod > F32(0)                                              # strict > from tmp = 0; a NaN product never enters
    masked = np.where(above, prod, F32(-np.inf))
    cate = np.where(above.any(-1), masked.argmax(-1), -1).astype(I32)  # argmax: the FIRST maximum
    score = np.where(above.any(-1), masked.max(-1), F32(-1)).astype(F32)
    cand = (cate >= 0) & (score > F32(thresh))                         # (cells, 3)
    hh, ww = np.divmod(np.arange(fh * fw), fw)
    anc = np.asarray(anchors, F64).astype(F32).reshape(2, 3, 2)[scale_index]   # the sample holds float anchors
    reg = v[:, :12].reshape(-1, 3, 4).astype(F64)
    with np.errstate(all="ignore"):
        bcx = (((reg[..., 0] * 2.0 - 0.5) + ww[:, None].astype(F64)) * F64(stride)).astype(F32)
        bcy = (((reg[..., 1] * 2.0 - 0.5) + hh[:, None].astype(F64)) * F64(stride)).astype(F32)
        tw, th = reg[..., 2] * 2.0, reg[..., 3] * 2.0
        bw = ((tw * tw) * anc[None, :, 0].astype(F64)).astype(F32)     # pow(x, 2) = x * x, exact for a float x
        bh = ((th * th) * anc[None, :, 1].astype(F64)).astype(F32)
        sw, sh = F64(F32(scale_w)), F64(F32(scale_h))
        d = np.stack([(bcx.astype(F64) - 0.5 * bw.astype(F64)) * sw, (bcy.astype(F64) - 0.5 * bh.astype(F64)) * sh,
                      (bcx.astype(F64) + 0.5 * bw.astype(F64)) * sw, (bcy.astype(F64) + 0.5 * bh.astype(F64)) * sh], -1)
        ok = ((d > -2147483649.0) & (d < 2147483648.0)).all(-1)        # (int) of anything else is undefined in C++: dropped
    keep = cand & ok
    box = np.trunc(np.where(ok[..., None], d, 0.0)).astype(np.int64).astype(I32)
    return box[keep], cate[keep], score[keep], int((cand & ~ok).sum())  # boolean indexing walks (cell, anchor) in row order


def iou_f32(bi, bp):
    """:58-70, :91-92 in fp32: candidate box bi (4,) against the picked boxes bp (k, 4), int32"""
    bi = bi.astype(I32)
    disjoint = (bi[0] > bp[:, 2]) | (bi[2] < bp[:, 0]) | (bi[1] > bp[:, 3]) | (bi[3] < bp[:, 1])
    with np.errstate(all="ignore"):
        iw = (np.minimum(bi[2], bp[:, 2]) - np.maximum(bi[0], bp[:, 0])).astype(I32).astype(F32)
        ih = (np.minimum(bi[3], bp[:, 3]) - np.maximum(bi[1], bp[:, 1])).astype(I32).astype(F32)
        inter = np.where(disjoint, F32(0), (iw * ih).astype(F32)).astype(F32)
        area_i = F32(I32(bi[2] - bi[0])) * F32(I32(bi[3] - bi[1]))
        area_p = ((bp[:, 2] - bp[:, 0]).astype(F32) * (bp[:, 3] - bp[:, 1]).astype(F32)).astype(F32)
        union = ((F32(area_i) + area_p).astype(F32) - inter).astype(F32)
        return (inter / union).astype(F32)                             # 0 / 0 = NaN: never above a threshold


def deploy_image(map0, map1, anchors, in_h, thresh, nms_thresh, scale_w=1.0, scale_h=1.0):
    """-> (records (n, 6) int32: x1, y1, x2, y2, cate, score bits - the survivors in picked order, dropped)"""
    parts = [candidates(m, s, anchors, in_h, thresh, scale_w, scale_h) for s, m in enumerate((map0, map1))]
    box = np.concatenate([p[0] for p in parts]).reshape(-1, 4)
    cate = np.concatenate([p[1] for p in parts])
    score = np.concatenate([p[2] for p in parts])
    dropped = parts[0][3] + parts[1][3]
    order = np.argsort(-score, kind="stable")                          # ties by candidate order
    box, cate, score = box[order], cate[order], score[order]
    picked = []
    pb = np.zeros((len(order), 4), I32)
    pc = np.zeros(len(order), I32)
    thr = F32(nms_thresh)
    for i in range(len(order)):
        k = len(picked)
        if k and ((iou_f32(box[i], pb[:k]) > thr) & (pc[:k] == cate[i])).any():
            continue
        pb[k], pc[k] = box[i], cate[i]
        picked.append(i)
    rec = np.zeros((len(picked), 6), I32)
    rec[:, :4], rec[:, 4], rec[:, 5] = box[picked], cate[picked], score[picked].view(I32)
    return rec, dropped


def deploy_batch(map0, map1, anchors, in_h, thresh, nms_thresh, scale=None, max_out=None):
    """maps (B, fh, fw, C) -> (boxes (B, max_out, 6) int32, count (B,) int32, dropped) as yfv2_deploy_post writes them"""
    B = map0.shape[0]
    rows = 3 * (map0.shape[1] * map0.shape[2] + map1.shape[1] * map1.shape[2])
    max_out = rows if max_out is None else max_out
    boxes, count, dropped = np.zeros((B, max_out, 6), I32), np.zeros(B, I32), 0
    for b in range(B):
        sw, sh = (1.0, 1.0) if scale is None else scale[b]
        rec, d = deploy_image(map0[b], map1[b], anchors, in_h, thresh, nms_thresh, sw, sh)
        count[b] = len(rec)
        boxes[b, :min(len(rec), max_out)] = rec[:max_out]
        dropped += d
    return boxes, count, dropped
