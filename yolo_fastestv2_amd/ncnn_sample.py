"""The reference's ncnn sample (sample/ncnn/src/yolo-fastestv2.cpp) as a Python entry point: what `yoloFastestv2::detection`
returns - integer boxes in the source frame, class, score - computed on the MI355X by Engine.detect_deploy_frames
(include/yfv2.h yfv2_detect_deploy_frames_u8).  The Python path of the reference (test.py: handel_preds +
non_max_suppression) is a DIFFERENT algorithm and stays where it was: Engine.detect_frames.
"""
NMS_THRESH = 0.25    # yolo-fastestv2.cpp:18


def unpack(boxes, count):
    """(boxes (B, max_out, 6) int32, count (B)) device tensors -> per-frame lists of (x1, y1, x2, y2, cate, score).  One copy per tensor."""
    import torch
    b, c = boxes.cpu(), count.cpu()
    score = b[..., 5].contiguous().view(torch.float32)
    out = []
    for i in range(b.shape[0]):
        n = min(int(c[i]), b.shape[1])
        out.append([tuple(int(v) for v in b[i, k, :5]) + (float(score[i, k]),) for k in range(n)])
    return out


def detection(engine, frames, thresh=0.3, nms_thresh=NMS_THRESH):
    """frames: list of uint8 (h, w, 3) tensors on the engine's device (BGR, as cv::Mat holds them).  Returns one list per frame of
    (x1, y1, x2, y2, cate, score) in the sample's order (score descending; equal scores by row order).  Waits for the device."""
    boxes, count = engine.detect_deploy_frames(frames, thresh, nms_thresh)
    out = unpack(boxes, count)
    engine.check_finite("ncnn_sample.detection")
    return out
