/* yfv2.h - C ABI of libyfv2.so: the MI355X-native (gfx950) Yolo-FastestV2 forward
 * detection path.  This header is the drop-in boundary: plain C, raw device
 * pointers and sizes, no torch / C++ types.  The reference (dog-qiuqiu/
 * Yolo-FastestV2) is pure Python and has no FFI of its own; each entry point
 * below replaces the named reference Python symbol (file:line under the
 * reference tree), and yolo_fastestv2_amd/ binds them with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every function returns 0 on success or a negative yfv2_status; nothing
 *     throws across the ABI; yfv2_last_error() gives the message for a handle
 *     (or for the calling thread when the handle is NULL / creation failed).
 *   - the caller owns every buffer it passes; the library owns only its weight
 *     blob and workspace (allocated in yfv2_create for `max_batch` images).
 *   - all work is enqueued on the caller's HIP stream (`stream` is a
 *     hipStream_t passed as void*; NULL = the default stream).  No hidden
 *     device synchronisation, except in yfv2_profile_forward and
 *     yfv2_debug_activation, which are measurement/debug helpers and say so.
 *   - all pointers named x / out6 / boxes / dets / idx / count are DEVICE
 *     pointers; weights passed to yfv2_load_weights are HOST pointers.
 *     (yfv2_plan.lanes = N at yfv2_create_ex: a forward / detect of a large batch is cut into N slices that run on
 *     N streams owned by the handle - forked from and joined back into the caller's stream with events inside the call, same
 *     ordering contract, bit-identical results; DESIGN.md section 5.  Memory: the parent handle keeps its full workspace
 *     for max_batch images - it serves batches below the slicing threshold, yfv2_profile_forward and the training entry
 *     points - and every lane adds a workspace for max_batch / N images plus its own copy of the 1 MB weight blob:
 *     about twice the activation memory of a handle without lanes, ~3 GB at max_batch 256.)
 *   - one handle per device, not thread-safe, and ONE STREAM AT A TIME: the handle's workspace (activations, logits
 *     and candidate rows of yfv2_detect, the class-filter scratch of yfv2_nms) is shared by all calls on it, so calls
 *     issued on different streams must be ordered by the caller (events); use one handle per concurrent stream.
 *   - there is no CPU fallback: if no gfx950 device is usable, yfv2_create
 *     fails with YFV2_ERR_DEVICE.
 */
#ifndef YFV2_H
#define YFV2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YFV2_ABI_VERSION 7 /* 2: yfv2_stage_info reports external bytes as well; 3: yfv2_train_*, yfv2_sgd_step; 4: yfv2_nonfinite, lanes; 5: yfv2_nonfinite_peek, yfv2_clock_probe_*; 6: yfv2_plan / yfv2_create_ex (the library reads no environment variable); 7: yfv2_debug_post; still 7 with the additive yfv2_frame, yfv2_resize_frames_u8, yfv2_detect_frames_u8 and the additive yfv2_anchor_kmeans, yfv2_kmeans_info, yfv2_debug_kmeans_group; still 7 with the additive yfv2_tile, yfv2_tile_plan, yfv2_merge_tiles, yfv2_detect_tiled_u8 and the additive yfv2_target_box, yfv2_export_maps, yfv2_deploy_post, yfv2_deploy_dropped, yfv2_detect_deploy_frames_u8 (old callers are unaffected) */
#define YFV2_API __attribute__((visibility("default")))
#define YFV2_MAX_DET 300 /* utils/utils.py:243 max_det */

typedef enum yfv2_status {
  YFV2_OK = 0,
  YFV2_ERR_ARG = -1,     /* NULL / out-of-range argument */
  YFV2_ERR_CONFIG = -2,  /* unsupported model configuration */
  YFV2_ERR_DEVICE = -3,  /* no usable gfx950 device / HIP runtime error */
  YFV2_ERR_WEIGHTS = -4, /* missing / mis-shaped tensor in yfv2_load_weights */
  YFV2_ERR_STATE = -5,   /* call order (e.g. forward before load_weights) */
  YFV2_ERR_BATCH = -6,   /* B < 1 or B > max_batch */
  YFV2_ERR_RANGE = -7    /* reported by the HOST classes (include/yfv2.hpp detection(), the Python Engine): the range guard of the
                            default plan tripped (yfv2_nonfinite) - the results of that call are invalid */
} yfv2_status;

typedef struct yfv2_ctx* yfv2_handle;

/* Mirrors the cfg dict the reference reads from its ".data" file
 * (utils/utils.py:13-65: classes, anchor_num, width, height, anchors) plus
 * the workspace size. */
typedef struct yfv2_config {
  int32_t classes;     /* 80; 1..255 */
  int32_t anchor_num;  /* 3 (the reference hard-codes 3: utils/utils.py:300,326) */
  int32_t height;      /* 352; multiple of 32 */
  int32_t width;       /* 352; multiple of 32; at most 4096 decode rows = 3 (H/16 W/16 + H/32 W/32), i.e. up to 512x512 */
  double anchors[12];  /* data/coco.data:17, float64 like utils/utils.py:305 */
  int32_t max_batch;   /* workspace is sized for this many images */
  int32_t device;      /* HIP device ordinal */
} yfv2_config;

/* One named fp32 tensor of a reference state_dict (host memory). */
typedef struct yfv2_tensor_desc {
  const char* name;  /* reference key, e.g. "backbone.stage2.0.branch_main.0.weight" */
  const float* data; /* host pointer, contiguous fp32 */
  int64_t numel;
} yfv2_tensor_desc;

/* Plan switches of a handle: WHICH kernels compute the path, never WHAT it computes (every plan is held to the same parity
 * tests, tests/test_gpu_parity.py::test_fallback_plans_match_oracle).  All zero = the default plan.  The library reads no
 * environment variable: this struct, passed to yfv2_create_ex, is the only way a plan is chosen (the Python layer and the
 * tools map YFV2_BF6=0 / YFV2_FUSED=0 / YFV2_POSTFUSE=0 / YFV2_FRONT=0 / YFV2_TPAIR=0 / YFV2_LANES=N / YFV2_TRACE=1 of THEIR
 * environment onto it, yolo_fastestv2_amd/_lib.py plan_from_env). */
typedef struct yfv2_plan {
  int32_t struct_size;        /* sizeof(yfv2_plan) of the caller's header (the struct may grow at its end) */
  int32_t fp32_matrix;        /* 1: every channel contraction on the fp32 matrix instructions (the reference's own arithmetic: no
                                 range limit, about half the speed) instead of fp16x3 on the f16 matrix cores */
  int32_t layer_by_layer;     /* 1: one launch per reference layer (77 launches), NHWC throughout: the general plan every fused
                                 kernel was first validated against */
  int32_t post_two_launches;  /* 1: yfv2_detect's decode and NMS as two launches (the only form beyond 96 classes / 2048 rows) */
  int32_t front_two_launches; /* 1: the stem and stage2.0 as two launches */
  int32_t towers_unpaired;    /* 1: the tower halves of the 22x22-class level as four launches instead of two */
  int32_t lanes;              /* N > 1: one call on a large batch is cut into N slices on N streams the handle owns; 0 / 1: off */
  int32_t trace;              /* 1: debug - per-wave cycle stamps of the stamped kernels (yfv2_debug_activation(100)) ... */
  int32_t trace_step;         /* ... of launch `trace_step` of the plan only (-1: of every stamped launch) */
} yfv2_plan;

/* ---- lifetime -------------------------------------------------------------- */

/* replaces: model/detector.py:8-19 Detector.__init__ (+ .to(device)).  yfv2_create(out, cfg) = yfv2_create_ex(out, cfg, NULL):
 * the default plan. */
YFV2_API int yfv2_create(yfv2_handle* out, const yfv2_config* cfg);
YFV2_API int yfv2_create_ex(yfv2_handle* out, const yfv2_config* cfg, const yfv2_plan* plan);
YFV2_API void yfv2_destroy(yfv2_handle h);
YFV2_API const char* yfv2_last_error(yfv2_handle h);
YFV2_API int yfv2_abi_version(void);

/* replaces: nn.Module.load_state_dict (test.py:28, evaluation.py:53).  Takes the
 * reference key set (BN running stats included, num_batches_tracked ignored),
 * folds BN to per-channel scale/shift (eval mode, eps 1e-5), re-lays-out the
 * filters for the kernels and uploads them.  Synchronous. */
YFV2_API int yfv2_load_weights(yfv2_handle h, const yfv2_tensor_desc* tensors, int32_t n);

/* Replace the 6 anchor pairs used by yfv2_decode / yfv2_detect (the reference passes
 * cfg["anchors"] to handel_preds on every call, utils/utils.py:305-306). Host-side only. */
YFV2_API int yfv2_set_anchors(yfv2_handle h, const double anchors[12]);

/* ---- the hot path ---------------------------------------------------------- */

/* replaces: model/detector.py:21-47 Detector.forward (export_onnx=False).
 * x: (B,3,H,W) fp32 NCHW in [0,1], 16-byte aligned (YFV2_ERR_ARG otherwise; the uint8 entry points: 4-byte aligned) (test.py:38; any |x| < 255.9 is computed to fp32 accuracy, beyond that the default
 * plan's stem - two-term fp16 operands on the matrix cores, yfv2_stem16.hip - leaves fp16's range: DETECTED, see
 * yfv2_nonfinite below; a handle created with yfv2_plan.fp32_matrix = 1 and the uint8 entry point yfv2_forward_u8 have no such bound).  out6: six NCHW fp32 logit tensors in the
 * reference's return order (reg_2, obj_2, cls_2, reg_3, obj_3, cls_3) with
 * shapes (B,4A,H/16,W/16) (B,A,..) (B,classes,..) and the same at H/32. */
YFV2_API int yfv2_forward(yfv2_handle h, const float* x, int32_t B, float* const out6[6], void* stream);

/* Range guard of the default plan.  Its channel contractions run as "fp16x3" (every fp32 operand split into two fp16 terms
 * after an exact power-of-two scale: fp32-accurate) and are valid while |activation| < 4094 and, for
 * yfv2_forward's fp32 input, |x| < 255.9 - two orders of magnitude above anything the COCO checkpoint or a He-initialised
 * network produces.  Beyond that an operand becomes (+Inf, -Inf), its products NaN, and the ReLU behind the conv would turn
 * the NaN into a silent 0; the reference's fp32 conv has no such cliff.  So every kernel of that plan tests its matrix-core
 * accumulators BEFORE the ReLU and sets a sticky word in the handle when one is not a number (also true for non-finite
 * values in x itself).  yfv2_nonfinite waits for `stream`, writes 1 to *flag if any forward / detect since the last query
 * tripped the guard (0 otherwise) and clears the word.  A handle created with yfv2_plan.fp32_matrix = 1 computes every
 * conv on the fp32 matrix instructions, has no such bound and never sets it.  The Python surface queries the word wherever it
 * synchronises anyway (handel_preds, non_max_suppression's callers, evaluation) and raises. */
YFV2_API int yfv2_nonfinite(yfv2_handle h, int32_t* flag, void* stream);
/* The same word WITHOUT waiting for anything and without clearing it: 1 if a kernel that has already completed tripped the
 * guard.  The word lives in host-mapped memory, so this is a host memory read - free.  For callers that never synchronise
 * with the host between calls (a detect loop that hands device tensors on, include/yfv2.hpp, Engine.detect): they look before
 * every call and learn of a tripped guard one call late instead of never; yfv2_nonfinite (after the results were waited
 * for) stays the exact query and the one that clears. */
YFV2_API int yfv2_nonfinite_peek(yfv2_handle h, int32_t* flag);

/* Same forward from the image layout the reference's callers hold BEFORE their pre-process step
 * (test.py:34-38, utils/datasets.py:106-111): uint8 (B, height, width, 3) - HWC, channel order as decoded
 * (BGR for cv2), values 0..255 - already resized to the configured size.  Replaces
 * `img.reshape(1,H,W,3); torch.from_numpy(img.transpose(0,3,1,2)); img.to(device).float()/255.0` + Detector.forward:
 * the transpose/cast is done by the stem kernel's loads, the 1/255 is folded into its filter (logits agree with
 * the fp32 path to rounding, same 1e-4 bound).  SURVEY.md section 8(f) row 1. */
YFV2_API int yfv2_forward_u8(yfv2_handle h, const uint8_t* x, int32_t B, float* const out6[6], void* stream);

/* replaces: utils/utils.py:303-358 handel_preds (+ make_grid :298-300).
 * boxes: (B, rows, 5+classes) fp32, rows = A*(H/16*W/16 + H/32*W/32) = 1815,
 * row order (y, x, anchor) per scale, scale 0 then 1; columns cx,cy,w,h,obj,cls. */
YFV2_API int yfv2_decode(yfv2_handle h, const float* const out6[6], int32_t B, float* boxes, void* stream);

/* replaces: utils/utils.py:232-296 non_max_suppression incl. xywh2xyxy :67-74
 * and torchvision.ops.nms (called at :286), without the 1 s wall-clock abort.
 * conf_thres is compared in fp32 (as the reference's tensor>python-float does),
 * iou_thres in double (as torchvision's kernel does).  classes may be NULL.
 * dets: (B,300,6) fp32 rows x1,y1,x2,y2,conf,cls, descending conf, first
 * count[b] rows valid; idx: (B,300) int32 = row index of each survivor in the
 * decode order; count: (B) int32. */
YFV2_API int yfv2_nms(yfv2_handle h, const float* boxes, int32_t B, float conf_thres, double iou_thres,
             const int32_t* classes, int32_t n_classes, float* dets, int32_t* idx, int32_t* count,
             void* stream);

/* forward -> decode -> NMS in one call (test.py:42,48,49 / utils/utils.py:379-383).
 * Intermediate logits and compact candidate rows live in the handle's workspace; the
 * (B,rows,5+classes) tensor is not materialised on this path (same arithmetic, same result). */
YFV2_API int yfv2_detect(yfv2_handle h, const float* x, int32_t B, float conf_thres, double iou_thres,
                float* dets, int32_t* idx, int32_t* count, void* stream);

/* yfv2_detect from uint8 (B, height, width, 3) images (see yfv2_forward_u8). */
YFV2_API int yfv2_detect_u8(yfv2_handle h, const uint8_t* x, int32_t B, float conf_thres, double iou_thres,
                            float* dets, int32_t* idx, int32_t* count, void* stream);

/* replaces: cv2.resize(img, (cfg.width, cfg.height), interpolation=cv2.INTER_LINEAR) of test.py:35 and
 * utils/datasets.py:107 for B equally sized uint8 HWC frames: src (B, src_h, src_w, 3) -> dst (B, cfg.height,
 * cfg.width, 3), both on the device, dst 4-byte aligned; dst is what yfv2_forward_u8 / yfv2_detect_u8 take.  The
 * arithmetic is OpenCV's 8-bit fixed-point bilinear path (11-bit coefficients, see yfv2_pre.hip); src size == dst
 * size is an exact copy.  Source rows up to ~27 000 pixels wide.  SURVEY.md section 8(f) row 1. */
YFV2_API int yfv2_resize_u8(yfv2_handle h, const uint8_t* src, int32_t B, int32_t src_h, int32_t src_w, uint8_t* dst, void* stream);

/* One uint8 HWC frame of a batch of frames of DIFFERENT sizes.  data: DEVICE pointer to its first byte (any alignment);
 * row r starts at data + r * row_pitch (row_pitch >= 3 * width: a crop of a larger frame needs no copy). */
typedef struct yfv2_frame {
  const uint8_t* data;
  int32_t height, width;
  int64_t row_pitch;
} yfv2_frame;

/* yfv2_resize_u8 for B frames of any sizes at once: frames is a HOST array of B descriptors; dst (B, cfg.height, cfg.width, 3)
 * on the device, 4-byte aligned.  Frame b's output is bit-identical to yfv2_resize_u8 of that frame alone.  Checked before
 * anything is enqueued (YFV2_ERR_ARG with a message): NULL pointers, B < 1, height or width < 1, row_pitch < 3 * width, a
 * frame wider than (160 KiB - 3 cfg.width) / 6 - 2 pixels (27 128 at width 352), dst not 4-byte aligned.  B > max_batch is
 * YFV2_ERR_BATCH: the descriptors go to a table of max_batch entries the handle owns, in one copy on `stream`.
 * Replaces test.py:35 over a list of decoded frames. */
YFV2_API int yfv2_resize_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, uint8_t* dst, void* stream);

/* test.py:34-68 for a batch of frames of any sizes: yfv2_resize_frames_u8 into a (max_batch, height, width, 3) buffer the
 * handle owns (allocated by the first call, which waits for the device once, like yfv2_loss's workspace), yfv2_detect_u8 on it
 * (on the handle's lanes where the plan has them), then columns 0-3 of the first count[b] rows of frame b are multiplied by
 * width_b / cfg.width (x) and height_b / cfg.height (y): fp32(double(x) * (double(w) / double(W))), test.py:58,65-66, no
 * clipping.  conf, class, idx, count and the rows beyond count[b] are exactly what yfv2_detect_u8 writes.  Same checks as
 * yfv2_resize_frames_u8 plus those of yfv2_detect_u8 (B <= max_batch, weights loaded). */
YFV2_API int yfv2_detect_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, float conf_thres, double iou_thres,
                                   float* dets, int32_t* idx, int32_t* count, void* stream);

/* ---- tiled detection of large frames: plan tiles, detect on every tile, merge on the device ----
 * The network sees cfg.width x cfg.height pixels; a 1920x1080 frame resized to that loses its small objects.  The usual remedy is
 * to cut the frame into overlapping tiles, detect on each, move the boxes back into the frame and suppress the duplicates the
 * overlaps produce.  A tile is a crop, which yfv2_frame reads in place; what these entry points add is the plan and the last step. */
typedef struct yfv2_tile { int32_t frame; int32_t x0, y0, width, height; } yfv2_tile; /* a rectangle inside frames[frame] */

/* Host only, no handle, no device.  Per axis of length L, tile t and overlap o (0 <= o < t): L <= t is the one interval [0, L);
 * otherwise s = t - o, n = ceil((L - t) / s) + 1 tiles of length t starting at min(i * s, L - t) - the last one ends on the edge.
 * Tiles are written row-major, y outer, .frame = 0; with include_full != 0 and more than one grid tile, one more tile covering
 * the whole frame comes last.  Returns the tile count (>= 1); tiles may be NULL to ask for it.  YFV2_ERR_ARG (negative): a size
 * < 1, an overlap outside [0, tile), cap smaller than the count. */
YFV2_API int yfv2_tile_plan(int32_t frame_h, int32_t frame_w, int32_t tile_h, int32_t tile_w, int32_t overlap_h, int32_t overlap_w,
                            int32_t include_full, yfv2_tile* tiles, int32_t cap);

/* The merge alone, on tile detections the caller already has: tile_dets (T, 300, 6) / tile_count (T) on the device in the layout
 * of yfv2_detect_frames_u8's output (every tile's rows conf-descending, finite coordinates, in TILE coordinates); tiles: HOST, T
 * entries, of which .frame, .x0 and .y0 are read here.  THE RULE, bit for bit (tests/tiles_ref.py merge_model restates it):
 *   candidates of frame f   its tiles in ascending k, rows r = 0 .. tile_count[k] - 1 of each; x1, x2 become fp32(x + fp32(x0)),
 *                           y1, y2 become fp32(y + fp32(y0)); conf and class are untouched
 *   order                   conf descending, stable over (k, r)
 *   greedy walk             a candidate is dropped if an already KEPT candidate has the same class (the floats compare equal) and a
 *                           match with it for which double(match) > merge_thres.  match, in fp32 as torchvision's kernel computes
 *                           IoU: w = max(0, min(x2) - max(x1)), h likewise, inter = w * h, areas (x2 - x1) * (y2 - y1);
 *                           merge_metric 0: inter / (a_i + a_j - inter); 1: inter / min(a_i, a_j) - intersection over the smaller
 *                           box, which merges an object cut by a tile edge with its whole view next door.  A NaN match (0 / 0)
 *                           suppresses nothing.  Classes are compared, not offset by cls * 4096 as non_max_suppression does: that
 *                           trick rounds away box bits at frame scale and breaks beyond 4096 pixels.
 *   stop                    after max_out kept rows
 * dets (F, max_out, 6): the kept rows of frame f in walk order, frame coordinates; src (F, max_out) or NULL: k * 300 + r, the
 * origin of each; count (F).  Rows beyond count[f] are not written; a frame without tiles has count 0.  Checked before anything
 * is enqueued (YFV2_ERR_ARG with a message): NULL pointers, T or F outside 1..65536, tiles[k].frame outside [0, F) or decreasing
 * in k (a frame's tiles are one contiguous range), merge_metric not 0 or 1, max_out outside 1..4096, merge_thres not finite.
 * Enqueue only.  The ordered candidate lists (32 bytes per tile row) live in a workspace of the handle, allocated by the first call
 * (one device wait) and grown - another wait - only by a call with more tiles or frames than any before.  No output bit
 * depends on the launch geometry or the run: positions come from binary searches, nothing is accumulated in floating point. */
YFV2_API int yfv2_merge_tiles(yfv2_handle h, const float* tile_dets /* (T,300,6) */, const int32_t* tile_count /* (T) */,
                              const yfv2_tile* tiles /* HOST, T entries */, int32_t T, int32_t F,
                              double merge_thres, int32_t merge_metric, int32_t max_out,
                              float* dets /* (F,max_out,6) */, int32_t* src /* (F,max_out) or NULL */, int32_t* count /* (F) */,
                              void* stream);

/* crop -> resize -> detect -> tile-to-frame -> merge, enqueue only.  frames: HOST array of F descriptors; tile k is the crop
 * {frames[f].data + y0 * row_pitch + 3 * x0, height, width, row_pitch}; the T crops go through yfv2_detect_frames_u8 unchanged
 * (same kernels, resize buffer and lanes), their results into a (max_batch, 300, 6) / idx / count workspace of the handle
 * (allocated by the first call, one device wait), then the merge above runs on them.  Checked before anything is enqueued:
 * everything yfv2_detect_frames_u8 checks, per crop; everything yfv2_merge_tiles checks; each frame's height, width >= 1, data,
 * row_pitch >= 3 * width; each rectangle inside its frame with width and height >= 1; T > max_batch is YFV2_ERR_BATCH. */
YFV2_API int yfv2_detect_tiled_u8(yfv2_handle h, const yfv2_frame* frames, int32_t F, const yfv2_tile* tiles, int32_t T,
                                  float conf_thres, double iou_thres, double merge_thres, int32_t merge_metric, int32_t max_out,
                                  float* dets, int32_t* src, int32_t* count, void* stream);

/* ---- decoder-format frames: YUV planes read in place (the samplings other than 4:2:0: 4.24) ----
 * Video decoders write a luma plane and half-resolution chroma - one interleaved plane (NV12 / NV21) or two planes
 * (I420; YV12 = I420 with u and v swapped by the caller) - each with a row pitch of its own.  A JPEG decoder keeps the sampling of
 * its file - 4:4:4, 4:4:0, 4:2:2 (planar, or one packed plane), grey, or 4:2:0 - and capture devices deliver packed 4:2:2: the six
 * further 8-bit formats below.  The entry points below take those planes as they are.  THE RULE: the result for a YUV frame is bit-identical to converting the frame to packed B, G, R with the
 * integer formula below and passing that to the _u8 entry point of the same name.
 *   pixel (r, c)   R = y0 + r, C = x0 + c; luma y[R * pitch_y + C]; chroma at (R >> 1, C >> 1), replicated, no interpolation (as
 *                  cv2 and the decoders' own sample converters do): NV12 u[(R>>1) * pitch_c + 2 * (C>>1)] is U and the byte after
 *                  it V; NV21 the same two bytes swapped; I420 u[(R>>1) * pitch_c + (C>>1)] is U and v[...] is V
 *   colour         int32 throughout, SHIFT = 20, coefficients rint(k * 2^20) (limited range: luma * 255/219, chroma * 255/224):
 *                                        off  CY       CVR      CVG      CUG      CUB
 *                    YFV2_BT601_LIMITED  16   1220542  1673527  -852492  -409993  2116026   (OpenCV's COLOR_YUV2BGR_NV12 / _I420 literals)
 *                    YFV2_BT709_LIMITED  16   1220945  1879825  -558796  -223607  2215014
 *                    YFV2_BT601_FULL     0    1048576  1470104  -748826  -360853  1858077   (JPEG)
 *                    YFV2_BT709_FULL     0    1048576  1651297  -490864  -196424  1945738
 *                  yy = max(Y - off, 0) * CY; u = U - 128; v = V - 128
 *                  R = clamp((yy + (1 << 19) + CVR * v) >> 20, 0, 255)              (arithmetic shift: floor for negatives)
 *                  G = clamp((yy + (1 << 19) + CVG * v + CUG * u) >> 20, 0, 255)
 *                  B = clamp((yy + (1 << 19) + CUB * u) >> 20, 0, 255)              stored B, G, R: the network's channel order
 * OpenCV is not in this image: the tests compare with a numpy statement of this published arithmetic (tests/yuv_model.py) - parity
 * with cv2 proper is unpinned, exactly as for the resize.
 *
 * 10-bit frames: what HEVC Main10, AV1 and VP9 profile 2 streams decode to.  Two formats of two-byte samples,
 * little-endian 16-bit words; yfv2_frame_yuv is unchanged (uint8_t* plane pointers, pitches in BYTES):
 *   YFV2_YUV_P010  semi-planar like NV12, U first in the interleaved plane; the value is in the HIGH 10 bits, v = word >> 6, and
 *                  the low 6 bits are ignored, whatever they hold (the hardware decoders' format)
 *   YFV2_YUV_I010  planar like I420 (yuv420p10le); the value is in the LOW 10 bits, v = word & 1023, and the high bits are ignored
 *   pixel (r, c)   the 8-bit rule with every sample index doubled to a byte offset: luma word at y + R * pitch_y + 2 * C; chroma at
 *                  (R >> 1, C >> 1), replicated: P010 u + (R>>1) * pitch_c + 4 * (C>>1) is U and the word after it V; I010
 *                  u + (R>>1) * pitch_c + 2 * (C>>1) is U and v + ... is V
 *   colour         the same expression on 10-bit codes; the 8-bit B, G, R is rounded ONCE from 10-bit precision, not truncated to
 *                  8 bits first.  Every literal is rint(k * 2^20) of the real coefficient per 10-bit code - limited range: luma
 *                  255 / (219 * 4), chroma 255 / (224 * 4) times 2(1-Kr), -2Kr(1-Kr)/Kg, -2Kb(1-Kb)/Kg, 2(1-Kb); full range:
 *                  255 / 1023 in place of both; Kr / Kb = 0.299 / 0.114 (BT.601), 0.2126 / 0.0722 (BT.709).  These are NOT OpenCV
 *                  literals: cv2 has no P010 conversion to agree with (tests/yuv_model.py re-derives them in float64).
 *                                        off  CY      CVR     CVG      CUG      CUB
 *                    YFV2_BT601_LIMITED  64   305236  418389  -213115  -102698  528805
 *                    YFV2_BT709_LIMITED  64   305236  469956  -139699  -55902   553753
 *                    YFV2_BT601_FULL     0    261375  366448  -186658  -89949   463157
 *                    YFV2_BT709_FULL     0    261375  411614  -122356  -48962   485008
 *                  yy = max(Y - off, 0) * CY; u = U - 512; v = V - 512; R, G, B as above (int32, + (1 << 19), >> 20, clamp to 0..255)
 * THE RULE is the one above: every *_yuv entry point on a 10-bit frame is bit-identical to converting the frame with this formula
 * and calling the _u8 entry point of the same name.  For limited-range frames whose samples are 4 times 8-bit samples the result is within 1 of the
 * 8-bit rule on those.  Checked in addition, before anything is enqueued (YFV2_ERR_ARG, the message names the frame and the
 * field): y, u (and v) 2-byte aligned; pitch_y and pitch_c even; pitch_y >= 2 * (x0 + width); pitch_c at least the last chroma byte
 * of a row; a frame wider than the two-byte width limit - the widest whose two luma rows, chroma rows and output row fit 160 KiB of
 * LDS, 20 343 at cfg.width 352 (half of the 8-bit limit: the staged rows take twice the bytes); and all frames of one call must
 * have ONE sample width - a call that mixes 8-bit and 10-bit frames is refused, the message naming the first frame that differs
 * from frame 0 (one launch is one kernel instantiation; split the batch).
 *
 * The other 8-bit samplings: six formats of one-byte samples; yfv2_frame_yuv is unchanged.  Pixel (r, c) of the
 * frame is (R, C) = (y0 + r, x0 + c) of the planes and reads
 *   YFV2_YUV_I422  planes y, u, v   luma y[R * pitch_y + C]; U u[R * pitch_c + (C >> 1)]; V likewise in v           (4:2:2, planar)
 *   YFV2_YUV_I440  planes y, u, v   luma as above; chroma at ((R >> 1), C)                                            (4:4:0)
 *   YFV2_YUV_I444  planes y, u, v   luma as above; chroma at (R, C)                                                   (4:4:4)
 *   YFV2_YUV_YUYV  plane y only     luma y[R * pitch_y + 2 C]; U y[R * pitch_y + 4 (C >> 1) + 1]; V that + 2          (YUY2: Y0 U Y1 V)
 *   YFV2_YUV_UYVY  plane y only     luma y[R * pitch_y + 2 C + 1]; U y[R * pitch_y + 4 (C >> 1)]; V that + 2          (U Y0 V Y1)
 *   YFV2_YUV_GREY  plane y only     luma y[R * pitch_y + C]; U = V = 128                                              (4:0:0)
 * Chroma is replicated, never interpolated, exactly as for 4:2:0 (a JPEG decoder's "fancy" up-sampling is not this rule).  The
 * colour formula is the 8-bit one above with the same four tables; for YFV2_YUV_GREY it runs with u = v = 0, so a full-range grey
 * frame gives B = G = R = Y.  THE RULE is the one above: every *_yuv entry point on such a frame is bit-identical to converting the
 * frame with that formula and calling the _u8 entry point of the same name.  Origin and size may have any parity: a tile or a crop
 * of a packed frame at odd x0 starts in the middle of a macropixel.
 * Checked before anything is enqueued (YFV2_ERR_ARG, the message names the frame and the field): u and v may be NULL and pitch_c is
 * ignored for YUYV, UYVY and GREY; u and v must not be NULL for the three planar formats; pitch_y >= x0 + width for the planar formats
 * and grey, pitch_y >= 4 * (((x0 + width - 1) >> 1) + 1) for the packed ones (an odd last pixel still reads its whole macropixel, and
 * nothing beyond it); pitch_c at least the last chroma byte of a row, with the format's horizontal shift; the range checks on the
 * pitches with the format's vertical shift.
 * ONE CALL MAY MIX 8-BIT FORMATS.  A call whose frames are all NV12, NV21 or I420 is the launch it always was.  A call with at least
 * one frame of these six formats runs the GENERAL 8-bit launch, which reads every 8-bit format, the three 4:2:0 ones included - a
 * 4:2:0 frame in such a call gives the same bits as in a 4:2:0-only call.  The general launch stages up to three full-width rows per
 * blended source row (a 4:4:4 frame has them), so its width limit is lower - 27 125 pixels at cfg.width 352 where a 4:2:0-only call
 * admits 40 689 (26 429 against 39 641 for training batches) - and it applies to EVERY frame of a mixed call, the NV12 ones too: the
 * message names the limit and says why.  Mixing 8-bit and 10-bit frames stays refused, as above. */
enum { YFV2_YUV_NV12 = 0, YFV2_YUV_NV21 = 1, YFV2_YUV_I420 = 2,
       YFV2_YUV_I422 = 3, YFV2_YUV_I440 = 4, YFV2_YUV_I444 = 5, YFV2_YUV_YUYV = 6, YFV2_YUV_UYVY = 7, YFV2_YUV_GREY = 8,   /*  */
       YFV2_YUV_P010 = 16, YFV2_YUV_I010 = 17 };   /* bit 4: two-byte samples (the 10-bit formats, above) */
enum { YFV2_BT601_LIMITED = 0, YFV2_BT709_LIMITED = 1, YFV2_BT601_FULL = 2, YFV2_BT709_FULL = 3 };
typedef struct yfv2_frame_yuv {
  const uint8_t* y;        /* DEVICE: luma plane, any alignment (P010/I010: 2-byte aligned, like u and v); YUYV/UYVY: the one packed plane */
  const uint8_t* u;        /* NV12/NV21/P010: the interleaved chroma plane; I420/I422/I440/I444/I010: the U plane; ignored for YUYV/UYVY/GREY */
  const uint8_t* v;        /* I420/I422/I440/I444/I010: the V plane; ignored for every other format */
  int64_t pitch_y, pitch_c;/* bytes per row of the luma / chroma plane(s); pitch_c is ignored for YUYV/UYVY/GREY */
  int32_t x0, y0;          /* top-left pixel of the frame inside the planes (any parity): a crop needs no copy */
  int32_t width, height;   /* pixels, >= 1, any parity */
  int32_t format, colour;  /* YFV2_YUV_*, YFV2_BT* */
} yfv2_frame_yuv;

/* yfv2_resize_frames_u8 for B YUV 4:2:0 frames of any sizes: dst is bit-identical to yfv2_resize_frames_u8 of the frames converted
 * by the rule above; the conversion happens at the four taps of each output pixel, from planes staged in LDS, so the planes are
 * read once and no B, G, R frame exists in memory.  Only bytes of the frame's own rectangle of each plane are read (and the chroma
 * samples it shares with its neighbours).  Checked before anything is enqueued (YFV2_ERR_ARG with a message naming the frame and
 * the field): NULL frames, y or u; NULL v with I420; width or height < 1; x0 or y0 < 0; pitch_y < x0 + width; pitch_c smaller
 * than the last chroma byte a row of the frame reads; unknown format or colour; a frame wider than the widest whose two luma rows,
 * chroma rows and output row fit 160 KiB of LDS (40 689 at cfg.width 352); pitches out of range; dst not 4-byte aligned.
 * B > max_batch is YFV2_ERR_BATCH: the descriptors go to a table of max_batch entries the handle owns, in one copy on `stream`. */
YFV2_API int yfv2_resize_frames_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B, uint8_t* dst, void* stream);

/* yfv2_detect_frames_u8 with the resize launch exchanged for yfv2_resize_frames_yuv's: the same handle-owned resize buffer, the
 * same yfv2_detect_u8 and the same frame-coordinate scaling by width_b / cfg.width, height_b / cfg.height.  Bit-identical to
 * yfv2_detect_frames_u8 on the converted frames.  Same checks as yfv2_resize_frames_yuv plus those of yfv2_detect_u8. */
YFV2_API int yfv2_detect_frames_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B, float conf_thres, double iou_thres,
                                    float* dets, int32_t* idx, int32_t* count, void* stream);

/* yfv2_detect_tiled_u8 on YUV frames: tile k is frames[tiles[k].frame]'s descriptor with x0 += tile.x0, y0 += tile.y0 and the
 * tile's size (which is why x0 and y0 may be odd); the T descriptors go through yfv2_detect_frames_yuv, then the same merge.
 * Bit-identical to yfv2_detect_tiled_u8 on the converted frames.  Checked before anything is enqueued: everything
 * yfv2_detect_frames_yuv checks, per frame and per tile; everything yfv2_merge_tiles checks; each rectangle inside its frame. */
YFV2_API int yfv2_detect_tiled_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t F, const yfv2_tile* tiles, int32_t T,
                                   float conf_thres, double iou_thres, double merge_thres, int32_t merge_metric, int32_t max_out,
                                   float* dets, int32_t* src, int32_t* count, void* stream);

/* ---- training batches from decoded frames: resize, contrast / brightness, NCHW fp32 in one launch ----
 * replaces: utils/datasets.py:107-111 (cv2.resize, img_aug, transpose(2,0,1)) with :10-16 contrast_and_brightness - the only
 * augmentation img_aug runs - and train.py:101 imgs.to(device).float() / 255.0, for B decoded frames of any sizes: dst is the
 * (B, 3, cfg.height, cfg.width) fp32 tensor yfv2_train_forward takes.  No uint8 batch exists in memory.
 * THE RULE, for both entry points: dst is bit-identical to yfv2_resize_frames_u8 / yfv2_resize_frames_yuv of the same frames,
 * followed per byte a of frame b by
 *     t = fl32(fl32(float(a) * alpha[b]) + beta[b])       two fp32 roundings, no fused multiply-add
 *     q = rint_half_even(min(max(t, 0.f), 255.f))
 *     x = fl32(float(q) / 255.f)                           IEEE-correct fp32 division = torch's .float() / 255.0
 * and permute(0, 3, 1, 2): dst[b][c][y][x] is that of byte (b, y, x, c), c = 0, 1, 2 = B, G, R (tests/train_batch_model.py states
 * it in numpy).  alpha = 1, beta = 0 is the identity (imgaug=False, the validation loader); alpha == beta == NULL means that for
 * every frame.  The three lines are OpenCV's scalar saturate_cast<uchar>(a * alpha + 0 * (1 - alpha) + beta) for 8-bit
 * addWeighted with the zero image of datasets.py:13.  OpenCV's own vector body fuses the multiply-add and its tail does not, so
 * cv2 itself is not one function of the byte, and OpenCV is not in this image: parity with cv2 proper is unpinned, exactly as for
 * the resize and the YUV conversion.  The draws of alpha and beta (random.uniform(0.25, 1.75) twice per image) stay the caller's.
 * alpha, beta: HOST, B floats each; they travel with the frame descriptors in their one copy on `stream`.  dst: DEVICE, 16-byte
 * aligned.  Checked before anything is enqueued (YFV2_ERR_ARG with a message): everything yfv2_resize_frames_u8 / _yuv checks of
 * the frames, under a lower width limit - the row is staged in LDS as fp32: (160 KiB - 1024 - 12 cfg.width) / 6 - 6 pixels for
 * B, G, R frames (26 426 at width 352), 39 641 for YUV frames at width 352 (19 819 for P010 / I010 frames); exactly one of alpha / beta NULL; an alpha or beta that is
 * not finite (the message names the frame); dst NULL or not 16-byte aligned.  B > max_batch is YFV2_ERR_BATCH.  Enqueue only: no
 * workspace, no device wait. */
YFV2_API int yfv2_train_batch_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B,
                                        const float* alpha, const float* beta /* HOST, B each, or both NULL */,
                                        float* dst /* DEVICE (B,3,H,W), 16-byte aligned */, void* stream);
YFV2_API int yfv2_train_batch_frames_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B,
                                         const float* alpha, const float* beta, float* dst, void* stream);

/* ---- second-stage crops: detections to resized crops, on the device ----
 * A detector this small usually runs first in a cascade: every box is cut out of its frame, resized to a fixed size and handed to
 * a second network.  These entry points do that without the host learning the boxes or their number: a plan launch turns the
 * detection rows into the resize kernels' own frame descriptors, and the resize launch covers the output's capacity.
 * THE RULE, bit for bit (tests/crops_model.py restates it; the library's one function of it is yfv2_crop_row_rect, yfv2_internal.h).
 * Row r of frame b is fp32 x1, y1, x2, y2, conf, cls in frame coordinates (yfv2_detect_frames_* / yfv2_detect_tiled_* output), the
 * frame is h x w pixels, px = double(pad_x), py = double(pad_y).  All arithmetic is IEEE double, every operation rounded on its
 * own (no fused multiply-add).
 *   candidate    r < min(max(count[b], 0), R), and cls is finite, equals an integer in 0..254 and that integer is one of
 *                `classes` (NULL: every class)
 *   skipped      a candidate with a coordinate that is not finite, or bw = x2 - x1 or bh = y2 - y1 not > 0; or, with
 *                ax1 = x1 - px * bw, ax2 = x2 + px * bw, cx1 = max(ax1, 0), cx2 = min(ax2, w), one for which cx2 > cx1 fails; the
 *                same in y with py, bh and h.  Counted per frame in crop_skipped, before and after the cut below; takes no slot.
 *   rectangle    X0 = floor(cx1), X1 = ceil(cx2), Y0, Y1 likewise: rect = (X0, Y0, X1 - X0, Y1 - Y0).  The rule gives
 *                0 <= X0 < X1 <= w, so nothing is clamped after the conversion to int and every rectangle has a pixel.
 *   selection    frame b's crops are its first max_per_frame candidates that are not skipped, in row order (rows are conf-descending:
 *                the top max_per_frame); n_b of them.  crop_offset = the exclusive prefix sum of n_b, crop_offset[B] the total.
 *   numbering    crop k = crop_offset[b] + j is the j-th selected row of frame b; only crops k < min(crop_offset[B], cap) are written
 *   pixels       crop k is the bilinear resize to (out_h, out_w) of the view {data + Y0 * row_pitch + 3 * X0, height, width,
 *                row_pitch} of its frame: bit-identical to what yfv2_resize_frames_u8 writes for that view on a handle whose network
 *                size is (out_h, out_w).  The two scales 1 / (out_w / width), 1 / (out_h / height) are the same two correctly
 *                rounded double divisions, computed on the device. */
typedef struct yfv2_crop_rule {
  int32_t out_h, out_w;      /* the size of every crop; out_w a multiple of 4 */
  float pad_x, pad_y;        /* each side of the box grows by pad * its extent on that axis; in [0, 16] */
  int32_t max_per_frame;     /* >= 1 */
  const int32_t* classes;    /* HOST: n_classes ints in 0..254, or NULL for every class */
  int32_t n_classes;
} yfv2_crop_rule;

/* The rectangle of one box: host only, no handle, no device, like yfv2_tile_plan.  box: x1, y1, x2, y2.  Returns 1 and writes
 * rect = X0, Y0, width, height; 0 when the rule skips the box (rect untouched); YFV2_ERR_ARG (negative) for a NULL pointer, a frame
 * size < 1 or a pad that is not finite or outside [0, 16].  It calls the function the plan kernel calls. */
YFV2_API int yfv2_crop_rect(const float box[4], int32_t frame_h, int32_t frame_w, float pad_x, float pad_y, int32_t rect[4]);

/* frames: HOST array of B descriptors (the frames the rows were detected on); dets (B, R, 6) and count (B) on the device - R = 300
 * for yfv2_detect_frames_* output, max_out for yfv2_detect_tiled_* output.  Outputs, all on the device: crops (cap, out_h, out_w,
 * 3) uint8, 4-byte aligned; crop_src (cap) = b * R + r of each crop; crop_rect (cap, 4); crop_offset (B + 1); crop_skipped (B) or
 * NULL.  Nothing is written beyond slot min(total, cap) of crops, crop_src and crop_rect; crop_offset[B] is the untruncated
 * total, which is how a caller sees that cap was too small.  Enqueue only: two small plan launches and the resize launch (grid cap *
 * out_h; a workgroup beyond the live crops returns at once), no host wait - except that the first call, or a call with a larger cap
 * than any before, allocates the handle's crop descriptor table and waits for the device once.  No output depends on the launch
 * geometry: slots come from ballots and integer prefix sums.  Checked before anything is enqueued (YFV2_ERR_ARG with a message):
 * NULL pointers; B < 1; R outside 1..4096; cap < 1 or cap * out_h > 2^31 - 1; out_h < 1; out_w < 4 or not a multiple of 4; crops
 * not 4-byte aligned; a pad that is not finite or outside [0, 16]; max_per_frame < 1; a class outside 0..254; everything
 * yfv2_resize_frames_u8 checks per frame, with the width limit taken at out_w: (160 KiB - 3 out_w) / 6 - 2 pixels.  B > max_batch
 * is YFV2_ERR_BATCH. */
YFV2_API int yfv2_crop_detections_u8(yfv2_handle h, const yfv2_frame* frames /* HOST, B */, int32_t B,
                                     const float* dets /* (B,R,6) */, const int32_t* count /* (B) */, int32_t R, const yfv2_crop_rule* rule,
                                     uint8_t* crops /* (cap,out_h,out_w,3) */, int32_t* crop_src /* (cap) */, int32_t* crop_rect /* (cap,4) */,
                                     int32_t* crop_offset /* (B+1) */, int32_t* crop_skipped /* (B) or NULL */, int32_t cap, void* stream);

/* The same for YUV 4:2:0 frames: rectangles are relative to the frame's own rectangle (x0, y0, width, height of yfv2_frame_yuv),
 * and the result is bit-identical to converting each frame with the integer colour formula above and calling
 * yfv2_crop_detections_u8.  A crop's descriptor is its frame's with the origin moved by (X0, Y0) - any parity.  Checks: as above
 * with everything yfv2_resize_frames_yuv checks per frame, its width limit taken at out_w. */
YFV2_API int yfv2_crop_detections_yuv(yfv2_handle h, const yfv2_frame_yuv* frames /* HOST, B */, int32_t B,
                                      const float* dets, const int32_t* count, int32_t R, const yfv2_crop_rule* rule,
                                      uint8_t* crops, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset, int32_t* crop_skipped,
                                      int32_t cap, void* stream);

/* ---- second-stage crops as network input: fp32 / fp16 NCHW, normalised, letterboxed, in the same launch ----
 * replaces, behind yfv2_crop_detections_*: permute(0, 3, 1, 2).float().div(255).sub(mean).div(std), the channel flip and the cast
 * to half that every classifier or re-identification network in a cascade asks for, and adds the aspect-preserving form.  The
 * entry points below do everything yfv2_crop_detections_u8 / _yuv do - same frames, dets, count, R and yfv2_crop_rule, the same
 * crop_src, crop_rect, crop_offset and crop_skipped from the same plan launches, the same counted launch over cap - and write, in
 * place of the uint8 crops, out (cap, 3, out_h, out_w).  No uint8 crop exists in memory.
 * THE RULE, bit for bit (tests/crop_tensors_model.py restates it in numpy; the library's functions of it are
 * yfv2_crop_letterbox_inner and yfv2_crop_tensor_f32 / _f16, yfv2_internal.h, which the kernels and the two host functions below call).
 *   1 selection  candidates, skipped rows, rectangles, selection and numbering are yfv2_crop_detections_*'s, above.
 *   2 geometry   integers, int64 intermediates, / = floor division.  A rectangle of cw x ch pixels, output (H, W) = (out_h, out_w):
 *                  letterbox = 0                   iw = W, ih = H, ox0 = oy0 = 0                       (the stretch of the uint8 crops)
 *                  letterbox = 1, W * ch <= H * cw iw = W, ih = max(1, (2 * ch * W + cw) / (2 * cw))   (the box is the wider)
 *                  letterbox = 1, otherwise        ih = H, iw = max(1, (2 * cw * H + ch) / (2 * ch))
 *                and with letterbox ox0 = (W - iw) >> 1, oy0 = (H - ih) >> 1: the aspect-preserving size rounded half up, never
 *                larger than the output, centred with the odd pixel of a margin on the right / below.
 *   3 bytes      the byte image, which is never written: a (H, W, 3) canvas of `fill` (B, G, R); its rows oy0 .. oy0 + ih, columns
 *                ox0 .. ox0 + iw hold the bilinear resize of the rectangle's view to (ih, iw) - yfv2_resize_frames_u8's arithmetic
 *                with the scales 1 / (iw / cw), 1 / (ih / ch).  With letterbox = 0 it is yfv2_crop_detections_*'s crop, byte for byte.
 *   4 value      out[k][c][y][x] comes from byte a = image[y][x][rgb ? 2 - c : c]:
 *                    x = fl32(float(a) / 255.f)
 *                    v = fl32(fl32(x - mean[c]) / std[c])
 *                every operation rounded to fp32 on its own - no fused multiply-add, IEEE-correct divisions - which is torchvision's
 *                ToTensor followed by Normalize on the host; mean = 0, std = 1 is plain / 255.  For YFV2_F16 v is rounded once more,
 *                to binary16, to nearest even (overflow gives an infinity).  Fill pixels go through the same lines. */
#define YFV2_F32 0
#define YFV2_F16 1
typedef struct yfv2_crop_tensor {
  int32_t dtype;             /* YFV2_F32 or YFV2_F16 */
  int32_t rgb;               /* 0: planes B, G, R (the frame's order); 1: planes R, G, B */
  float mean[3], std[3];     /* by OUTPUT plane; finite, std > 0 */
  int32_t letterbox;         /* 0: stretch; 1: keep the rectangle's aspect ratio, centre, fill the rest */
  uint8_t fill[3];           /* B, G, R: the frame's order, whatever rgb is */
} yfv2_crop_tensor;

/* Step 2 for one rectangle: host only, no handle, no device.  inner = ox0, oy0, iw, ih; 1 <= iw <= out_w, 1 <= ih <= out_h.
 * YFV2_ERR_ARG for a NULL pointer, a size < 1 or letterbox outside 0..1.  It calls the function the plan kernel calls. */
YFV2_API int yfv2_crop_letterbox(int32_t cw, int32_t ch, int32_t out_h, int32_t out_w, int32_t letterbox, int32_t inner[4]);

/* Step 4 for one byte: host only.  Writes the fp32 value and the bits of its binary16 form (either pointer may be NULL).
 * YFV2_ERR_ARG for a outside 0..255, a mean that is not finite or a std that is not finite and > 0. */
YFV2_API int yfv2_crop_tensor_value(int32_t a, float mean, float std, float* f32, uint16_t* f16_bits);

/* out: DEVICE (cap, 3, out_h, out_w) fp32 or fp16, 16-byte aligned; everything else as yfv2_crop_detections_u8.  Nothing is written
 * beyond slot min(total, cap).  out_w is a multiple of 4 as for the uint8 crops; an fp16 row is stored 16 bytes at a time when
 * out_w is a multiple of 8 and 8 bytes at a time otherwise.  Enqueue only, like yfv2_crop_detections_u8: two plan launches, one
 * resize launch; the descriptor table is the same handle-owned workspace.  Checked before anything is enqueued (YFV2_ERR_ARG with
 * a message): everything yfv2_crop_detections_u8 checks (out in place of crops: NULL, or not 16-byte aligned); tensor NULL; dtype,
 * rgb or letterbox out of range; a mean that is not finite; a std that is not finite or not > 0; the width limit of the frames,
 * which is lower than the crops': the row is staged as three fp32 or fp16 planes - (160 KiB - 12 out_w) / 6 - 6 pixels for fp32,
 * (160 KiB - 6 out_w) / 6 - 6 for fp16. */
YFV2_API int yfv2_crop_tensors_u8(yfv2_handle h, const yfv2_frame* frames /* HOST, B */, int32_t B,
                                  const float* dets /* (B,R,6) */, const int32_t* count /* (B) */, int32_t R, const yfv2_crop_rule* rule,
                                  const yfv2_crop_tensor* tensor, void* out /* (cap,3,out_h,out_w) */, int32_t* crop_src /* (cap) */,
                                  int32_t* crop_rect /* (cap,4) */, int32_t* crop_offset /* (B+1) */, int32_t* crop_skipped /* (B) or NULL */,
                                  int32_t cap, void* stream);

/* The same for YUV 4:2:0 frames: bit-identical to yfv2_crop_tensors_u8 on the frames converted with the integer colour formula.
 * Checks: as above with everything yfv2_resize_frames_yuv checks per frame; the width limit is the widest frame whose two luma rows,
 * chroma rows (each rounded to 16 bytes) and three planes fit 160 KiB of LDS, never above yfv2_crop_detections_yuv's. */
YFV2_API int yfv2_crop_tensors_yuv(yfv2_handle h, const yfv2_frame_yuv* frames /* HOST, B */, int32_t B,
                                   const float* dets, const int32_t* count, int32_t R, const yfv2_crop_rule* rule,
                                   const yfv2_crop_tensor* tensor, void* out, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset,
                                   int32_t* crop_skipped, int32_t cap, void* stream);

/* ---- identity across frames: a per-stream IoU tracker on the device ----
 * The inputs of the entry points above are video: many streams, one frame of each per batch.  A tracker gives every detection an
 * identity that lasts across frames, so that a second stage runs once per object: its state lives on the device, one launch updates
 * it from a batch of detection rows, and the launch can emit - compacted, in the (dets, count) layout yfv2_crop_detections_* takes -
 * exactly the rows whose track was confirmed in this frame.  This form has no motion model: an unmatched track keeps its last box
 * (yfv2_track_update_motion, below, is the form with one).
 * THE RULE, bit for bit (tests/track_model.py restates it; the one function of the IoU is behind yfv2_track_iou).
 * A tracker has S streams, each a table of M = max_tracks slots.
 *   state        one caller-owned device buffer of S * (8 + 10 * M) int32 words; all zero = empty.  Per stream 8 header words - ids
 *                issued, live tracks, frames seen, births, deaths, dropped births, 0, 0 - then M slots of 10 words: the fp32 bits of
 *                x1, y1, x2, y2, conf, cls, then int32 id, hits, misses, age.  id == 0: the slot is free and all ten words are zero.
 *   a call       B frames; frame b belongs to stream stream_of[b], the streams of one call are distinct; its rows are dets[b, 0..n),
 *                n = min(max(count[b], 0), R), fp32 x1, y1, x2, y2, conf, cls (yfv2_detect_frames_* / yfv2_detect_tiled_* output).
 * For each frame, in this order:
 *   1 valid      a row is valid when all six floats are finite and x2 > x1, y2 > y1.  Invalid rows never match, never start a track.
 *   2 edges      valid row r - live slot s when (class_aware: the two class floats compare equal) and, with v = the IoU in fp32 as
 *                yfv2_merge_tiles computes it - xx1 = max(x1, x1'), xx2 = min(x2, x2'), w = max(0, xx2 - xx1), h likewise, inter =
 *                w * h, v = inter / ((area + area') - inter), area = (x2 - x1) * (y2 - y1); every operation a separate fp32 one -
 *                double(v) > match_thres.  A NaN v gives no edge.
 *   3 matching   greedy: the edges in the order v descending, then r ascending, then s ascending; an edge is taken if its row and
 *                its slot are both still free.
 *   4 matched    the slot's box, conf and cls become the row's; hits += 1, misses = 0, age += 1; track_id[b, r] = id,
 *                track_hits[b, r] = hits.
 *   5 unmatched  live slot: misses += 1, age += 1; if misses > max_misses the slot is zeroed and deaths += 1.
 *   6 births     the valid unmatched rows with conf >= init_conf (fp32), in row order, after the deaths of step 5: the k-th takes
 *                the k-th lowest free slot (slots freed in step 5 included) with id = issued + 1, issued += 1, hits = 1, misses = 0,
 *                age = 1, births += 1; track_id / track_hits of the row are the new id and 1.  No free slot: dropped += 1, id 0.
 *   7 header     frames += 1; live = the number of live slots.  track_id and track_hits are written for every r in [0, R): 0 where
 *                no track is assigned, 0 beyond n.
 *   8 fresh      (optional outputs) a row is fresh when track_hits[b, r] == confirm_hits - hits only grows, so each track is fresh
 *                once.  The fresh rows in row order: fresh_dets[b, j] = the row's six floats untouched, fresh_src[b, j] = r,
 *                fresh_count[b] their number; rows beyond fresh_count[b] are not written.
 * No output bit depends on the launch geometry, on the other frames of the call or on the run: slots and compaction come from
 * ballots and integer prefix sums, and nothing is accumulated in floating point. */
typedef struct yfv2_track_rule {
  int32_t max_tracks;        /* M: slots per stream, 1..1024 */
  double  match_thres;       /* an edge needs double(IoU) > match_thres; finite, >= 0 */
  int32_t class_aware;       /* != 0: a row matches only a track of an equal class float */
  float   init_conf;         /* a birth needs conf >= init_conf; not NaN */
  int32_t max_misses;        /* a track dies at its (max_misses + 1)-th consecutive miss; >= 0 */
  int32_t confirm_hits;      /* a row is fresh when its track's hits equal this; >= 1 */
} yfv2_track_rule;

/* int32 words of ONE stream's state: 8 + 10 * max_tracks; YFV2_ERR_ARG (negative) for max_tracks outside 1..1024.  Host only. */
YFV2_API int64_t yfv2_track_state_words(int32_t max_tracks);

/* The IoU of step 2 for two boxes x1, y1, x2, y2: host only, no handle, like yfv2_crop_rect; it calls the function the kernel
 * calls.  Returns YFV2_OK and writes *v (which may be NaN), YFV2_ERR_ARG for a NULL pointer. */
YFV2_API int yfv2_track_iou(const float a[4], const float b[4], float* v);

/* One update of the streams stream_of[0..B) from dets (B, R, 6) / count (B), all device pointers but stream_of.  state: S *
 * yfv2_track_state_words(M) int32; track_id (B, R); track_hits (B, R) or NULL; fresh_dets (B, R, 6), fresh_src (B, R), fresh_count
 * (B): all three or none.  Enqueue only: one workgroup per frame, one launch (per 768 frames - stream_of travels in the launch's own
 * arguments), no host wait, no handle workspace.  Checked before anything is enqueued (YFV2_ERR_ARG with a message, the state
 * untouched): NULL pointers; B < 1; S < 1; R outside 1..4096; max_tracks outside 1..1024; a stream outside [0, S) or named twice;
 * match_thres not finite or negative; init_conf NaN; max_misses < 0; confirm_hits < 1; the three fresh outputs not all given or
 * all NULL. */
YFV2_API int yfv2_track_update(yfv2_handle h, const float* dets /* (B,R,6) */, const int32_t* count /* (B) */, int32_t R, int32_t B,
                               const int32_t* stream_of /* HOST, B */, int32_t* state, int32_t S, const yfv2_track_rule* rule,
                               int32_t* track_id /* (B,R) */, int32_t* track_hits /* (B,R) or NULL */, float* fresh_dets /* (B,R,6) or NULL */,
                               int32_t* fresh_src, int32_t* fresh_count, void* stream);

/* ---- identity across frames with a motion model: a constant-velocity Kalman filter per track ----
 * The rule above matches a row against a track's LAST box, so an object hidden for a few frames comes back under a new id (and is
 * fresh a second time).  The motion form is opt-in and changes nothing above: the same kernel, the same walk, a state of its own
 * layout.  Each track carries four independent one-dimensional constant-velocity Kalman filters, one per coordinate cx, cy, w, h -
 * exact, not an approximation: with diagonal process and measurement noise and the transition ByteTrack and BoT-SORT use, the 8 x 8
 * covariance stays block-diagonal in (position, velocity) pairs - so a coordinate is five fp32 numbers x, v, p00, p01, p11.
 * THE RULE, bit for bit (tests/track_motion_model.py restates it; the one function of the filter is behind yfv2_track_filter_step
 * and yfv2_track_birth).  Every fp32 operation is one separately rounded operation in the order written; divisions round to
 * nearest.  sp, sv, sm = std_pos, std_vel, std_meas.  The scale l is the track's w for cx and w, its h for cy and h: predict uses
 * the posterior w.x / h.x from before the predict, update the predicted w.x / h.x.
 *   predict      tp = sp * l; tv = sv * l; x' = x + v; p00' = (((p00 + p01) + p01) + p11) + tp * tp; p01' = p01 + p11;
 *                p11' = p11 + tv * tv; v is unchanged.
 *   update (z)   tm = sm * l'; s = p00' + tm * tm; k0 = p00' / s; k1 = p01' / s; y = z - x'; x = x' + k0 * y; v = v + k1 * y;
 *                p00 = p00' - k0 * p00'; p01 = p01' - k0 * p01'; p11 = p11' - k1 * p01'.
 *   birth        x = z, v = 0, p01 = 0, p00 = t * t with t = (2.0f * sp) * l, p11 = t * t with t = (10.0f * sv) * l; l from the row's
 *                own w / h.
 *   measurement  of a row: cx = (x1 + x2) * 0.5f, w = x2 - x1, and likewise for y.
 *   corners      of a filter state: x1 = cx - w * 0.5f, x2 = cx + w * 0.5f, and likewise for y.
 *   NaN          which NaN an invalid operation makes depends on the processor; every NaN among the five results of a predict or an
 *                update, or among four corners, is replaced by the quiet NaN 0x7fc00000 before it is stored, used or written out.
 *   state        S * (8 + 32 * M) int32 words; the header as above; a slot is 32 words: 0..9 as above, 10..29 the four filters in the
 *                order cx, cy, w, h, each x, v, p00, p01, p11 (fp32 bits), 30..31 zero.  All zero = empty.  One update is one time
 *                step; a stream absent from a call is not advanced.
 * Per frame the order above changes in these places only:
 *   0 predict    (new) every live slot is predicted and its 20 filter words are replaced by the predicted ones.  A slot is BLIND for
 *                this frame if any of its 20 words is not finite or its predicted w or h is not > 0: it has no edges, so it misses.
 *   1 valid      a row is also invalid if any of its four measurement values is not finite.
 *   2 edges      v is the IoU between the row and the slot's PREDICTED CORNERS, not its last box.
 *   4 matched    the filter is updated with the row's measurement; words 0..5 become the row; track_box[b, r] = the posterior corners.
 *   5 unmatched  the filter words stay as predicted (the track coasts), words 0..5 keep the last matched row; a dead slot zeroes all
 *                its words.
 *   6 births     as above, plus the filter initialised from the row; track_box[b, r] = the corners of the born state.
 *   7 header     track_box (optional) is zero where no track is assigned and zero beyond n.
 * Defaults (documented, not applied by the C ABI): std_pos = 1/20, std_vel = 1/160, std_meas = 1/20. */
typedef struct yfv2_track_motion {
  float std_pos, std_vel, std_meas;   /* all three finite and > 0 */
} yfv2_track_motion;

/* int32 words of ONE stream's state in the motion form: 8 + 32 * max_tracks; errors as yfv2_track_state_words.  Host only. */
YFV2_API int64_t yfv2_track_motion_state_words(int32_t max_tracks);

/* One filter, host only, no handle, like yfv2_track_iou: it calls the function the kernel calls.  out = in predicted one step with
 * scale_predict and then, if z is not NULL, updated with *z and scale_update.  YFV2_ERR_ARG for a NULL in / out / motion or a
 * motion value that is not finite and > 0. */
YFV2_API int yfv2_track_filter_step(const float in[5], const float* z /* NULL: predict only */, float scale_predict, float scale_update,
                                    const yfv2_track_motion* motion, float out[5]);

/* The 20 filter words of a track born from a row's box x1, y1, x2, y2.  Host only; errors likewise. */
YFV2_API int yfv2_track_birth(const float row_box[4], const yfv2_track_motion* motion, float out[20]);

/* yfv2_track_update in the motion form: state is S * yfv2_track_motion_state_words(M) int32; track_box (B, R, 4) fp32 or NULL.
 * Every check of yfv2_track_update, plus motion not NULL and its three values finite and > 0.  Enqueue only: one workgroup per
 * frame, one launch per 768 frames, no host wait, no handle workspace. */
YFV2_API int yfv2_track_update_motion(yfv2_handle h, const float* dets /* (B,R,6) */, const int32_t* count /* (B) */, int32_t R, int32_t B,
                                      const int32_t* stream_of /* HOST, B */, int32_t* state, int32_t S, const yfv2_track_rule* rule,
                                      const yfv2_track_motion* motion, int32_t* track_id /* (B,R) */, int32_t* track_hits /* (B,R) or NULL */,
                                      float* track_box /* (B,R,4) or NULL */, float* fresh_dets /* (B,R,6) or NULL */, int32_t* fresh_src,
                                      int32_t* fresh_count, void* stream);

/* ---- identity across frames, two association passes: low-score rows keep tracks alive and start none ----
 * With one detection threshold a caller chooses between losing an object whose score dips for a few frames (occlusion, blur: the
 * track dies, the object returns under a new id and is fresh a second time) and starting a track from every spurious row.  The
 * two-pass form (ByteTrack's second association) is opt-in and changes nothing above: the same kernel, the same walk, either state
 * layout as it is - a state can be handed between the one-pass and the two-pass entry point of its layout from call to call.
 * Detect at a low threshold; confident rows are matched first; the low-score rows are offered only to the tracks still unmatched;
 * no track ever starts from a low-score row.
 * THE RULE, bit for bit (tests/track_two_pass_model.py restates it).  Per frame the order of the rule above changes in these places
 * only; in the motion form the same changes apply on top of the motion rule (step 0 stays, v is taken against the predicted corners):
 *   1 valid      as before.  A valid row is additionally HIGH when conf >= high_conf, LOW when low_conf <= conf < high_conf, OUT
 *                otherwise (fp32 compares).  Invalid rows and OUT rows are treated alike: they never match, never start a track,
 *                track_id 0.
 *   2/3 first    the edges and the greedy walk exactly as above, over the HIGH rows only, with match_thres.
 *   3b second    (new) edges between the LOW rows and the live slots the first pass left unmatched - with tracked_only, only
 *                those whose misses word was 0 when the frame began: double(v) > match_thres_low, class_aware as in the first
 *                pass; the same greedy order, v descending, then r ascending, then s ascending.  The first pass is complete
 *                before the second begins: a LOW row never takes a slot from a HIGH row, whatever its IoU.
 *   4 matched    identical for both passes (in the motion form: the filter update with the row's measurement, track_box).
 *   5 unmatched  as before; a slot barred from the second pass by tracked_only is simply unmatched.
 *   6 births     only HIGH rows that are unmatched and have conf >= init_conf.  A LOW row never starts a track.
 *   7 header     header word 6 - 0 in the other forms, which do not touch it - counts second-pass matches: += their number in
 *                this frame.  track_pass (optional) is 1 for a row matched in the first pass or born, 2 for a row matched in the
 *                second pass, 0 otherwise and beyond n.
 *   8 fresh      unchanged: a LOW row whose match brings hits to confirm_hits is fresh.
 * Consequence: with high_conf = -inf every valid row is HIGH, and the form is the one-pass form of its layout bit for bit - state,
 * header and every output - with track_pass == 1 wherever track_id != 0.
 * Defaults (documented, not applied by the C ABI): high_conf = 0.5, low_conf = 0.1, match_thres_low = 0.5, tracked_only = 1 -
 * ByteTrack's track_thresh, its 0.1 floor, its second-pass threshold and its "lost tracks are not offered low rows". */
typedef struct yfv2_track_second {
  float   high_conf;        /* a valid row is HIGH when conf >= high_conf (fp32 compare); not NaN */
  float   low_conf;         /* ... LOW when low_conf <= conf < high_conf; a valid row below low_conf takes no part; not NaN, <= high_conf */
  double  match_thres_low;  /* a second-pass edge needs double(IoU) > match_thres_low; finite, >= 0 */
  int32_t tracked_only;     /* != 0: the second pass offers only slots whose misses were 0 when the frame began */
} yfv2_track_second;

/* One update in the two-pass form, of either layout: motion NULL - state is S * yfv2_track_state_words(M) int32, the plain 10-word
 * slots; else S * yfv2_track_motion_state_words(M), the 32-word motion slots.  track_pass (B, R) int32 or NULL; track_box (B, R, 4)
 * or NULL, and only with motion; the other arguments as above.  Every check of yfv2_track_update (and, with motion, of
 * yfv2_track_update_motion); also YFV2_ERR_ARG with a message, nothing enqueued and the state untouched, for: second NULL;
 * high_conf or low_conf NaN; low_conf > high_conf; match_thres_low not finite or negative; track_box given without motion.
 * Enqueue only: one workgroup per frame, one launch per 768 frames, no host wait, no handle workspace.  An addition within ABI 7:
 * yfv2_abi_version() is unchanged, as for the two tracker forms above. */
YFV2_API int yfv2_track_update_two_pass(yfv2_handle h, const float* dets /* (B,R,6) */, const int32_t* count /* (B) */, int32_t R, int32_t B,
                                        const int32_t* stream_of /* HOST, B */, int32_t* state, int32_t S, const yfv2_track_rule* rule,
                                        const yfv2_track_motion* motion /* NULL: the plain 10-word slots; else the 32-word motion slots */,
                                        const yfv2_track_second* second, int32_t* track_id /* (B,R) */, int32_t* track_hits /* (B,R) or NULL */,
                                        int32_t* track_pass /* (B,R) or NULL */, float* track_box /* (B,R,4) or NULL; needs motion */,
                                        float* fresh_dets /* (B,R,6) or NULL */, int32_t* fresh_src, int32_t* fresh_count, void* stream);

/* ---- identity across frames, appearance association: the IoU fused with the cosine of second-stage embeddings ----
 * yfv2_crop_tensors_* produces what a re-identification network takes; this form takes what it returns.  Every row comes with an
 * embedding, every track keeps a unit-norm feature - a moving average of the embeddings it absorbed - and a first-pass edge between
 * a row and a track whose boxes are close may be valued by the cosine of the two instead of the IoU (BoT-SORT's fusion: the larger
 * similarity wins).  The form is opt-in and changes nothing above: the same kernel, the same walk, either state layout as it is, one
 * pass or two.  The features live in a buffer of their own, so a state can be handed between this entry point and the others.
 * THE RULE, bit for bit (tests/track_appearance_model.py restates it; its functions are behind yfv2_track_cosine and
 * yfv2_track_feature_step).  Every fp32 operation is one separately rounded operation in the order written; divisions and the
 * square root round to nearest.
 *   emb          (B, R, D) fp32 on the device, 16-byte aligned: emb[b, r, :] is the embedding e of row r of frame b - the caller's
 *                network output for the crop of that row; it need not be normalised.  Rows beyond n are not read.
 *   feat         one caller-owned device buffer of S * M * (4 + D) int32 words; all zero = empty.  A slot of the table has the 4 + D
 *                words feat[(stream * M + slot) * (4 + D) ..]: word 0 the int32 n_feat, the number of embeddings absorbed (0: the
 *                track has no feature), words 1..3 zero, then D fp32 bits: the unit-norm feature f.
 *   dot16(a, b)  the only reduction.  Sixteen partial sums P[j] = 0.0f; for i = 0 .. D/16 - 1 ascending: P[j] = P[j] + a[16 i + j] *
 *                b[16 i + j]; then for stride = 8, 4, 2, 1: P[j] = P[j] + P[j + stride] for j < stride; the result is P[0].
 *   appearance   of a row: n_r = sqrt(dot16(e, e)); the row HAS APPEARANCE when n_r is finite and > 0 (a NaN, an infinity, an
 *                overflowing square or an all-zero e fails on its own: no element is tested).  Otherwise it takes part by IoU alone.
 *   cosine       c(r, s) = dot16(e_r, f_s) / n_r, every NaN replaced by the quiet NaN 0x7fc00000; used only when finite.
 * Per frame, on top of the rule of the layout and the pass form in use:
 *   2 edges      (first pass only) v is the IoU as before (motion: against the predicted corners).  If the row has appearance, the
 *                slot has n_feat > 0, double(v) > prox_thres, c is finite and double(c) > app_thres, then s = c > v ? c : v; else
 *                s = v.  There is an edge when double(s) > match_thres; class_aware as before.  The walk orders by s descending, then
 *                row, then slot.  Boxes that do not overlap never pair (prox_thres >= 0, the compare is strict).  The second pass
 *                (3b) uses the IoU alone with match_thres_low.
 *   4 matched    (either pass) track_cos[b, r] = c of the pair against the feature from BEFORE this frame's update; 0 if the row
 *                has no appearance or the slot no feature.  Header word 7 - 0 in every other form, which do not touch it - += the
 *                number of first-pass matches whose edge value was c (the conditions above held and c > v).  Then, if the row has
 *                appearance: with n_feat == 0, f[d] = e[d] / n_r and n_feat = 1; otherwise g[d] = alpha * f[d] + beta * (e[d] /
 *                n_r) with beta = 1.0f - alpha, m = sqrt(dot16(g, g)), and if m is finite and > 0, f[d] = g[d] / m and n_feat += 1 -
 *                if not, the feature is unchanged.  A row without appearance leaves the feature unchanged.
 *   5 unmatched  the feature is unchanged; a dead slot zeroes all its 4 + D words.
 *   6 births     f = e / n_r, n_feat = 1; for a row without appearance all 4 + D words are zero.
 *   7 header     track_cos (optional) is 0 where no track is assigned, for born rows and beyond n.
 * Consequence: with app_thres = +inf no pair passes, and state, header (word 7 stays 0) and every shared output are those of the
 * entry point of the same layout and pass form, bit for bit, while feat is still maintained.
 * Defaults (documented, not applied by the C ABI): dim = 128, prox_thres = 0.5, app_thres = 0.75, alpha = 0.9 - BoT-SORT's
 * proximity_thresh, 1 - appearance_thresh and the momentum of its feature average.
 * LDS: one workgroup holds 28 R + 52 M bytes (the other forms: 24 R + 48 M; here also a row's n_r and a slot's n_feat), which must
 * not exceed 163328 - a CU's 160 KiB less 512 bytes the kernel keeps: R = 4096 admits M <= 935, M = 1024 admits R <= 3931. */
typedef struct yfv2_track_appearance {
  int32_t dim;              /* D: floats of an embedding; a multiple of 16 in 16..2048 (pad another width with zeros: they add exactly) */
  double  prox_thres;       /* the cosine counts only when double(IoU) > prox_thres; finite, >= 0 */
  double  app_thres;        /* ... and when double(cosine) > app_thres; not NaN, +inf: never */
  float   alpha;            /* weight of the old feature in the moving average; finite, in [0, 1] */
} yfv2_track_appearance;

/* int32 words of ONE stream's features: max_tracks * (4 + D); YFV2_ERR_ARG (negative) for max_tracks outside 1..1024 or a D that
 * yfv2_track_appearance does not admit.  Host only. */
YFV2_API int64_t yfv2_track_feature_words(int32_t max_tracks, int32_t D);

/* The norm and the cosine of the rule for one embedding e and one feature f of D floats: *norm = sqrt(dot16(e, e)), *cos =
 * dot16(e, f) / *norm, NaNs as 0x7fc00000 - computed whether or not the norm gives e an appearance.  Host only, no handle, like
 * yfv2_track_iou: the functions the kernel calls.  YFV2_ERR_ARG for a NULL pointer or a D outside the rule's. */
YFV2_API int yfv2_track_cosine(const float* e, const float* f, int32_t D, float* norm, float* cos);

/* Step 4's feature update for one track: f_in / n_feat_in (>= 0) and the matched row's embedding e -> f_out / *n_feat_out
 * (f_out may be f_in).  Host only; YFV2_ERR_ARG likewise, and for an alpha that is not finite or outside [0, 1]. */
YFV2_API int yfv2_track_feature_step(const float* f_in, int32_t n_feat_in, const float* e, int32_t D, float alpha, float* f_out,
                                     int32_t* n_feat_out);

/* One update in the appearance form: motion NULL or not chooses the state's layout, second NULL or not one pass or two, exactly as
 * for yfv2_track_update_two_pass; emb, feat and appearance as above; track_cos (B, R) fp32 or NULL; track_pass only with second,
 * track_box only with motion.  Every check of the form it extends; also YFV2_ERR_ARG with a message, nothing enqueued, state and
 * feat untouched, for: emb, feat or appearance NULL; emb not 16-byte aligned; dim not a multiple of 16 or outside 16..2048;
 * prox_thres not finite or negative; app_thres NaN; alpha not finite or outside [0, 1]; 28 R + 52 max_tracks above 163328.
 * Enqueue only: one workgroup per frame, one launch per 768 frames, no host wait, no handle workspace.  An addition within ABI 7:
 * yfv2_abi_version() is unchanged. */
YFV2_API int yfv2_track_update_appearance(yfv2_handle h, const float* dets /* (B,R,6) */, const int32_t* count /* (B) */, int32_t R, int32_t B,
                                          const int32_t* stream_of /* HOST, B */, int32_t* state, int32_t S, const yfv2_track_rule* rule,
                                          const yfv2_track_motion* motion /* NULL: the plain slots */, const yfv2_track_second* second /* NULL: one pass */,
                                          const yfv2_track_appearance* appearance, const float* emb /* (B,R,D) */, int32_t* feat,
                                          int32_t* track_id /* (B,R) */, int32_t* track_hits /* (B,R) or NULL */,
                                          int32_t* track_pass /* (B,R) or NULL; needs second */, float* track_box /* (B,R,4) or NULL; needs motion */,
                                          float* track_cos /* (B,R) or NULL */, float* fresh_dets /* (B,R,6) or NULL */, int32_t* fresh_src,
                                          int32_t* fresh_count, void* stream);

/* ---- the ncnn sample's deployment path (sample/ncnn/src/yolo-fastestv2.cpp) ----
 * The reference's only native component post-processes differently from its Python path in every step that decides which boxes
 * come out: no objectness pre-filter (score = cls * obj > thresh only), boxes scaled to the source frame and TRUNCATED TO int
 * before the NMS, the overlap of intersection_area (touching boxes intersect, with area 0), classes compared explicitly, no
 * limit of 300, default thresholds 0.3 / 0.25.  The entry points below compute exactly that; yfv2_decode / yfv2_nms /
 * yfv2_detect* stay the Python path's arithmetic. */
typedef struct yfv2_target_box { int32_t x1, y1, x2, y2, cate; float score; } yfv2_target_box;   /* yolo-fastestv2.h:9-25 TargetBox */

/* replaces: model/detector.py:33-44, the export layout of Detector(export_onnx=True), on the six NCHW logit maps of yfv2_forward:
 * map0 (B, H/16, W/16, 5A + classes), map1 (B, H/32, W/32, 5A + classes), NHWC fp32 on the device, 4-byte aligned; channels
 * sigmoid(4A reg) | sigmoid(A obj) | softmax(classes).  The obj and class channels of pixel (y, x) are bit-identical to columns 4
 * and 5.. of yfv2_decode's rows (y, x, a) (the same device functions); the reg channels are that sigmoid of the logits.  One
 * launch, every logit read once.  Needs no weights. */
YFV2_API int yfv2_export_maps(yfv2_handle h, const float* const out6[6], int32_t B, float* map0, float* map1, void* stream);

/* replaces: yolo-fastestv2.cpp:113-183 getCategory + predHandle and :58-110 intersection_area + nmsHandle, for B images at once,
 * on two maps in yfv2_export_maps' layout (from any producer).  One workgroup per image; enqueue only.  THE RULE, bit for bit
 * (tests/deploy_model.py restates it in numpy; tests/golden/golden_deploy.npz holds the compiled sample's own results):
 *   rows         scale 0 then 1; h, w, anchor b - the sample's loop order.  v = the pixel's 5A + classes floats
 *   score, cate  objScore = v[4A + b]; over the classes i in ascending order fl32(v[5A + i] * objScore), running maximum with
 *                strict > from 0: the FIRST maximum wins; nothing above 0 (or only NaN): score -1, cate -1, never a candidate
 *   candidate    score > thresh in fp32
 *   box          bcx = fl32(((v[4b] * 2. - 0.5) + w) * stride) in double, stride = cfg.height / map height (integer); bcy likewise;
 *                bw = fl32((v[4b + 2] * 2.)^2 * anchor) in double with the handle's anchor (yfv2_set_anchors) ROUNDED TO float, as
 *                the sample's std::vector<float> holds it; x1 = (int)((bcx - 0.5 * bw) * scaleW) in double, truncated toward zero
 *   order        score descending; TIES BY CANDIDATE ORDER (the row order above).  The sample calls std::sort, which leaves the
 *                order of equal scores unspecified: this is the ONLY place where the result may differ from a build of the sample
 *   greedy walk  a candidate is dropped if an already kept one has the same cate and IoU > nms_thresh with it, in fp32:
 *                inter = 0 if a.x1 > b.x2 || a.x2 < b.x1 || a.y1 > b.y2 || a.y2 < b.y1, else float(min x2 - max x1) *
 *                float(min y2 - max y1) (int differences); area = float(x2 - x1) * float(y2 - y1); IoU = inter / ((area_a +
 *                area_b) - inter), IEEE division - 0 / 0 = NaN keeps the box
 *   scale        device (B, 2) fp32 scaleW, scaleH per image, or NULL = 1, 1
 *   boxes        device (B, max_out) records: the kept candidates of image b in walk order; count[b] is the FULL number of
 *                survivors (there is no cap of 300: the sample has none), only the first max_out are stored and the records from
 *                min(count[b], max_out) on are zero.  max_out in 1..yfv2_num_rows
 * DELIBERATE DIFFERENCE: the sample's (int) of a value that is NaN or outside int32 is undefined behaviour (a candidate whose reg
 * values are not finite).  Such a candidate is dropped here and counted: yfv2_deploy_dropped waits for `stream` and returns the
 * number of candidates the LAST yfv2_deploy_post / yfv2_detect_deploy_frames_u8 on this handle dropped (0 for sane maps).
 * thresh < 0 or NaN is YFV2_ERR_ARG (a score is never negative; the order keys rely on it), as are NULL pointers and max_out out
 * of range - before anything is enqueued; B outside 1..max_batch is YFV2_ERR_BATCH.  Needs no weights.  The first post call on a
 * handle allocates a few bytes (one device wait). */
YFV2_API int yfv2_deploy_post(yfv2_handle h, const float* map0, const float* map1, int32_t B,
                              const float* scale /* device (B,2) fp32 scaleW,scaleH; NULL = 1,1 */, float thresh, float nms_thresh,
                              yfv2_target_box* boxes /* (B,max_out) */, int32_t* count /* (B) */, int32_t max_out, void* stream);
YFV2_API int yfv2_deploy_dropped(yfv2_handle h, int32_t* dropped /* host */, void* stream);

/* replaces: yolo-fastestv2.cpp:185-221 yoloFastestv2::detection for a batch of frames of any sizes: yfv2_resize_frames_u8 ->
 * yfv2_forward_u8 (on the handle's lanes where the plan has them) -> yfv2_export_maps into a workspace of the handle ->
 * yfv2_deploy_post with scaleW = (float)width_b / (float)cfg.width, scaleH = (float)height_b / (float)cfg.height (:189-190).  Bit-identical
 * to those four calls one after the other.  The resize is the library's cv2-arithmetic bilinear (yfv2_resize_u8), NOT ncnn's
 * from_pixels_resize (:193): pixel values, and with them scores, differ slightly from an ncnn run on the same frame; the
 * post-process on given maps does not.  Same checks as yfv2_detect_frames_u8 and yfv2_deploy_post.  Enqueue only (the first call
 * allocates the resize buffer and the maps for max_batch images and waits for the device once). */
YFV2_API int yfv2_detect_deploy_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, float thresh, float nms_thresh,
                                          yfv2_target_box* boxes, int32_t* count, int32_t max_out, void* stream);

/* replaces: utils/utils.py:194-230 get_batch_statistics (with bbox_iou :76-108), the per-detection loop of
 * evaluation() (:361-395).  dets/count: the padded output of yfv2_nms / yfv2_detect; targets: (T,6) fp32 device rows
 * [image index, label, x1, y1, x2, y2] in pixels, i.e. what evaluation() holds after utils.py:372-376; tp: (B,300)
 * int32, 1 where the reference's true_positives is 1.  Same walk as the reference: detections in their (score-
 * descending) order, best-IoU target over all of the image's targets (first on ties), IoU with the "+1 pixel"
 * convention in fp32, threshold compared in fp32, a target is matched once, stop when all targets are matched.
 * At most 1024 targets per image (YFV2_ERR_ARG otherwise; COCO's maximum is below 100).  B is not bound by max_batch
 * (no workspace is involved).  Unlike the other entry points this one waits for the stream before it returns (it reads
 * the overflow flag back); evaluation loops use the two-call form below instead.  SURVEY.md section 8(f) row 2. */
YFV2_API int yfv2_batch_statistics(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets,
                                   int32_t T, float iou_threshold, int32_t* tp, void* stream);
/* The same launch, enqueue only (no host synchronisation): an image with more than 1024 targets sets a sticky flag
 * inside the handle (its own device word, not shared with any other entry point).  yfv2_batch_statistics_overflow
 * waits for `stream`, returns that flag through *overflowed (1: at least one call since the last query produced an
 * invalid tp row) and clears it - call it once after the last batch (utils.evaluation does). */
YFV2_API int yfv2_batch_statistics_async(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets,
                                         int32_t T, float iou_threshold, int32_t* tp, void* stream);
YFV2_API int yfv2_batch_statistics_overflow(yfv2_handle h, int32_t* overflowed, void* stream);
/* The same matching at K IoU thresholds in ONE launch (for AP at several thresholds, e.g. 0.50:0.05:0.95; the definition stays
 * the reference's get_batch_statistics at each of them - nothing of pycocotools is modelled).
 *   thresholds  HOST array of K floats, copied before the call returns; any values, in any order, repeats allowed
 *   K           1..32
 *   tpmask      device (B, 300) uint32: bit k of tpmask[b][i] is EXACTLY what yfv2_batch_statistics_async writes to tp[b][i] at
 *               iou_threshold = thresholds[k] (compared in fp32; a NaN threshold gives a zero bit); bits at and above K are 0
 * The target with the largest IoU for a detection does not depend on the threshold: it is found once per detection, and only
 * the walk "above the threshold and still free" runs per threshold (one lane each).  Note that bit k is NOT monotone in the
 * threshold: a detection can miss at 0.5 because a higher-ranked one took its target, and hit at 0.75 where that one failed.
 * The 1024-targets-per-image rule and its sticky flag are those of yfv2_batch_statistics_async (the same word, read by
 * yfv2_batch_statistics_overflow); the blocking form reads it back and fails like yfv2_batch_statistics.  K outside 1..32 or a
 * NULL thresholds / tpmask is YFV2_ERR_ARG before anything is enqueued. */
YFV2_API int yfv2_batch_statistics_multi_async(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets,
                                               int32_t T, const float* thresholds /* host */, int32_t K, uint32_t* tpmask, void* stream);
YFV2_API int yfv2_batch_statistics_multi(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets,
                                         int32_t T, const float* thresholds /* host */, int32_t K, uint32_t* tpmask, void* stream);

/* replaces: utils/loss.py:130-208 compute_loss (with build_target :53-124 and bbox_iou(CIoU) :8-51) and, when grad6 is
 * not NULL, what autograd derives from it: the gradient of the TOTAL loss w.r.t. each of the six logit maps (same
 * shapes as out6; device pointers; overwritten).  SURVEY.md section 8(f) row 3, first slice - the loss end of the
 * training path (train.py:105-108); train-mode forward and the convolutions' backward are not implemented.
 *   out6     the six NCHW logit maps of yfv2_forward (B images)
 *   targets  (T, 6) fp32 device rows [image index in the batch, class, cx, cy, w, h], box normalised to [0, 1]: the tensor
 *            the reference's collate_fn builds (utils/datasets.py:12-22); T may be 0
 *            PRECONDITION: 0 <= image index < B and 0 <= class < classes; a row that violates it is skipped (the
 *            reference's CrossEntropyLoss raises on such a class), it is never used as an index
 *   losses   device float[4]: lbox (x3.2), lobj (x64), lcls (x32) and their sum, the 4-tuple compute_loss returns
 * Uses the handle's anchors (yfv2_set_anchors) as float64 like the reference.  Work is enqueued on `stream`; the
 * handle's loss workspace grows (one device synchronisation) when T exceeds what earlier calls needed. */
YFV2_API int yfv2_loss(yfv2_handle h, const float* const out6[6], int32_t B, const float* targets, int32_t T, float* losses,
                       float* const grad6[6], void* stream);

/* ---- anchors from a label set: the first step a user of the reference takes on their own data (genanchors.py) ---- */

typedef struct yfv2_kmeans_info {
  int32_t struct_size;    /* in: sizeof(yfv2_kmeans_info) of the caller's header (the struct may grow at its end; 0 = this header's) */
  int32_t iterations;     /* passes run, the terminating one included (the reference's `iter`) */
  int32_t converged;      /* 1: assignments repeated; 0: stopped at max_iter, on an empty cluster or on bad input */
  int32_t empty_cluster;  /* -1, or the first cluster index that received no point (the reference divides 0/0 there) */
  int32_t bad_input;      /* 1: some w or h is not a finite number > 0 */
} yfv2_kmeans_info;

/* replaces: genanchors.py:67-102 kmeans (+ IOU :17-32, avg_IOU :34-40).  IoU k-means over N label sizes, float64 throughout:
 * every pass assigns each point to the centroid of smallest 1 - IoU (the reference's four cases, each with its own formula;
 * first minimum on ties) and, unless the pass ends the loop, replaces every centroid by the mean of its points.
 *   wh         device (N, 2) float64: w, h of every label (the reference's annotation_dims), 8-byte aligned
 *   centroids  device (k, 2) float64, 8-byte aligned: in = the initial centroids, out = the final ones in the reference's
 *              order (unsorted); 1 <= k <= 32
 *   assign     device (N) int32 or NULL: the cluster of every point under the RETURNED centroids
 *   avg_iou    device, 1 double: sum over the points of their largest IoU with a returned centroid / N (avg_IOU)
 *   info       HOST; set info->struct_size before the call
 * Termination is the reference's (:87-92): the loop ends in the first pass whose assignments equal the previous pass's; that
 * pass does not move the centroids, and `iterations` counts it.  The loop also ends - still YFV2_OK, info says why - after
 * pass number max_iter (>= 1), on a cluster that received no point and, in the first pass, on a w or h that is not a finite
 * number > 0.  DELIBERATE DIFFERENCE: the reference divides 0 / 0 on an empty cluster and carries NaN centroids on; here the
 * pass that ends the loop, for whatever reason, never moves the centroids: they hold the last completed update, and assign
 * and avg_iou are those of exactly these centroids (on bad input avg_iou may itself be not a number).
 * Every output bit is a function of (wh, initial centroids, k) alone - not of the device, the launch geometry or the run:
 * sums are taken over fixed chunks of 1024 points in a fixed tree, no floating-point atomics.
 * Work is enqueued on `stream` in groups of passes; like yfv2_batch_statistics, and unlike the hot path, this call WAITS for
 * the stream after every group and before it returns (it reads the verdict of the passes back).  Argument errors (a NULL
 * wh / centroids / avg_iou / info, N < 1, k outside 1..32, max_iter < 1, wh or centroids not 8-byte aligned) are
 * YFV2_ERR_ARG with a message, before anything is enqueued.  Works on any handle, whatever its configuration; needs no
 * weights; touches nothing of the forward / detect workspace (its own buffer grows - one device synchronisation - when
 * ceil(N / 1024) * k, or N where assign is NULL, exceeds what earlier calls needed). */
YFV2_API int yfv2_anchor_kmeans(yfv2_handle h, const double* wh /* device (N,2) */, int64_t N,
                                double* centroids /* device (k,2): in = initial, out = final, reference order (unsorted) */,
                                int32_t k, int32_t max_iter, int32_t* assign /* device (N) or NULL */,
                                double* avg_iou /* device, 1 double */, yfv2_kmeans_info* info /* host */, void* stream);
/* Test hook: how many passes yfv2_anchor_kmeans enqueues between two looks at the verdict (1..64, default 8).  No output bit
 * depends on it (tests/test_gpu_anchors.py shows that); it only trades host waits against launches that return at once. */
YFV2_API int yfv2_debug_kmeans_group(yfv2_handle h, int32_t group);

/* ---- average precision over a whole validation set: the last line of evaluation() (utils/utils.py:397) ---- */

typedef struct yfv2_ap_result {
  int32_t struct_size;          /* in: sizeof(yfv2_ap_result) of the caller's header (the struct may grow at its end; 0 = this header's) */
  int32_t classes_present;      /* distinct target classes */
  int32_t bad_input;            /* 1: a target class that is not an integer in 0..254, or a conf that is not finite; the rest is then undefined */
  int64_t n_gt[256], n_pred[256];    /* per class: targets, predictions (0 where the class has no target) */
  double p[256], r[256], ap[256];    /* per class: final precision, final recall, average precision; 0 where the class is absent */
  double mean_p, mean_r, mean_ap, mean_f1;   /* over the present classes in ascending order, added one after the other on the host; NaN if there is none */
} yfv2_ap_result;

/* replaces: utils/utils.py:136-192 ap_per_class with :110-134 compute_ap, the host tail of evaluation() (:397).
 *   tp          device (N) int32: 1 = true positive, what yfv2_batch_statistics writes (any non-zero value counts as 1)
 *   conf        device (N) fp32 confidences, pred_cls device (N) fp32 class labels of the same detections
 *   target_cls  device (T) fp32: the class of every ground-truth object; each must be an integer in 0..254
 *   out         HOST; set out->struct_size before the call
 * TIE RULE.  Detections are ranked by conf descending and, where conf is equal (+0 and -0 are equal), by ascending input index:
 * np.argsort(-conf, kind="stable").  The reference calls np.argsort(-conf), an unstable sort whose order among equal confidences
 * is an accident of numpy's implementation; this is the ONLY place where the result may differ from the reference's by more
 * than the order of a summation.  Per class c of target_cls: n_gt / n_pred = its count in target_cls / pred_cls; over its
 * detections in rank order prec_i = tpc_i / (i + 1), rec_i = tpc_i / (n_gt + 1e-16) with tpc the running count of tp; p and r
 * are the last prec and rec; ap = sum over the true positives of (rec_i - rec_{i-1}) * max(prec_j, j >= i) - compute_ap's
 * envelope sum (its closing term to recall 1 is +-0).  A pred_cls that equals no target class is ignored, as the reference's
 * `pred_cls == c` ignores it; a class without predictions scores 0 on all three.
 * Every output bit is a function of the four arrays alone: the ap sum is one fixed tree over chunks of 1024 ranked positions
 * (DESIGN.md 4.12), no floating-point atomics.  A target class outside 0..254 or not an integer, or a NaN / infinite conf,
 * sets bad_input (still YFV2_OK; such a value is never used as an index).  N = 0 gives all zeros; T = 0 gives
 * classes_present = 0 and NaN means (np.mean of an empty list).  N and T are limited to 2^31 - 1 (YFV2_ERR_ARG beyond, as for
 * NULL arrays, negative sizes or arrays that are not 4-byte aligned - before anything is enqueued).
 * Work is enqueued on `stream`; like yfv2_anchor_kmeans this call WAITS for the stream before it returns.  Works on any handle;
 * touches nothing of the forward / detect workspace (its own buffer: a call needs about 17 bytes per detection; when N exceeds
 * what earlier calls needed it is re-allocated - one device synchronisation - at 1.5 times the need, about 25 bytes per detection). */
YFV2_API int yfv2_ap_per_class(yfv2_handle h, const int32_t* tp, const float* conf, const float* pred_cls, int64_t N,
                               const float* target_cls, int64_t T, yfv2_ap_result* out, void* stream);
/* yfv2_ap_per_class at K thresholds in one pass (mAP@[.5:.95] is the mean of out[k].mean_ap over the ten thresholds; the
 * definition is the reference's ap_per_class + compute_ap at each threshold - no 101-point interpolation, no crowd flags, no
 * area ranges).
 *   tpmask  device (N) uint32: bit k = tp at threshold k, what yfv2_batch_statistics_multi writes; bits at and above K are ignored
 *   K       1..32
 *   out     HOST, K records one after the other; set out[k].struct_size before the call (out[0]'s is the distance between records)
 * out[k] equals, bit for bit and in every field, what yfv2_ap_per_class returns for tp[i] = (tpmask[i] >> k) & 1: the targets'
 * histogram, the keys and the five sort passes run once (the rank does not look at tp), one launch brings the masks into rank
 * order, and the per-class walk - the same device code, reading bit k where the single form reads its tp bit - runs on a
 * (class, threshold) grid.  The tie rule, bad_input (reported in every record), the limits on N and T, the alignment and NULL
 * checks and "waits for the stream" are yfv2_ap_per_class's; K outside 1..32 is YFV2_ERR_ARG.  Workspace: about 21 bytes per
 * detection (the single form's 17 and the 4 of the permuted mask) plus K result blocks of 10 KB and K sets of chunk sums (8 bytes
 * per 1024 detections each); re-allocated at 1.5 times the need, about 32 bytes per detection, when N or K exceed what earlier
 * calls needed. */
YFV2_API int yfv2_ap_per_class_multi(yfv2_handle h, const uint32_t* tpmask, const float* conf, const float* pred_cls, int64_t N,
                                     const float* target_cls, int64_t T, int32_t K, yfv2_ap_result* out, void* stream);

/* ---- the rest of the training path: one iteration of train.py:96-123 on the device.
 * Parameters, their gradients and the BatchNorm buffers are the CALLER's device tensors in the reference's own layouts and
 * under the reference's state_dict names; nothing is copied.  Correctness-first kernels (plain NCHW fp32, float64
 * reductions), not the throughput path.
 *
 * yfv2_train_bind      tensors: every floating-point entry of the state_dict (weights, biases, running_mean / running_var) as
 *                      DEVICE pointers; grads: one device buffer per trainable parameter (same names).  Pointers must stay
 *                      valid until the next bind.
 * yfv2_train_forward   replaces model/detector.py:21-47 Detector.forward in train() mode (train.py:105): every BatchNorm on
 *                      batch statistics (biased variance), running statistics moved by momentum 0.1 with the unbiased
 *                      variance (num_batches_tracked is the caller's integer); writes the six NCHW logit maps and records
 *                      what the backward needs in a workspace that grows with B.
 * yfv2_train_backward  replaces total_loss.backward() (train.py:110) from the logits down: grad6 = gradient of the loss
 *                      w.r.t. the six logit maps (yfv2_loss); ADDS the gradient of every parameter to its bound buffer (zero
 *                      them first; accumulating over `subdivisions` batches as train.py:122 does is then free).
 * yfv2_sgd_step        replaces optimizer.step() (torch.optim.SGD as train.py:81-85 builds it: momentum, weight_decay,
 *                      dampening 0, no Nesterov) for ONE parameter tensor of n elements: d = g + wd p; buf = first_step ? d :
 *                      momentum buf + d; p -= lr buf.  The warm-up of train.py:113-117 only changes `lr`. */
YFV2_API int yfv2_train_bind(yfv2_handle h, const yfv2_tensor_desc* tensors, int32_t n, const yfv2_tensor_desc* grads, int32_t ng);
YFV2_API int yfv2_train_forward(yfv2_handle h, const float* x, int32_t B, float* const out6[6], void* stream);
YFV2_API int yfv2_train_backward(yfv2_handle h, const float* const grad6[6], void* stream);
YFV2_API int yfv2_sgd_step(yfv2_handle h, float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                           float weight_decay, int32_t first_step, void* stream);
/* The same update for MANY parameter tensors in a few launches (the network has 225: one launch each is 225 kernels of two
 * microseconds and as many gaps).  items: HOST array, one entry per tensor (device pointers inside); the entries travel in the
 * kernel-argument segment, 96 per launch. */
typedef struct yfv2_sgd_item {
  float* param; const float* grad; float* momentum_buf; /* device pointers */
  int64_t n;                                            /* elements */
  int32_t first_step; int32_t reserved;                 /* first_step: momentum_buf is uninitialised (buf = d) */
} yfv2_sgd_item;
YFV2_API int yfv2_sgd_step_multi(yfv2_handle h, const yfv2_sgd_item* items, int32_t n_items, float lr, float momentum, float weight_decay,
                                 void* stream);

/* ---- introspection / measurement (bench.py, tests) ------------------------- */

YFV2_API int32_t yfv2_num_rows(yfv2_handle h);   /* 1815 for 352x352, A=3 */
YFV2_API int32_t yfv2_num_stages(yfv2_handle h); /* launches in one forward */

/* Static description of launch `i` of the forward plan: kernel name, which
 * reference layers it covers, and its ALGORITHMIC work per image: flops =
 * 2*MACs; bytes_per_image = per-LAYER accounting (every reference layer the
 * launch covers reads its input and writes its output once, fp32: BASELINE.md
 * section 4); external_bytes_per_image = SURVEY.md section 8(d)'s figure for a
 * fused launch - only what the launch itself must read from and write to HBM
 * (the chain of seven stride-1 blocks: one read + one write of the activation).
 * bench.py's roofline uses the external figure. */
YFV2_API int yfv2_stage_info(yfv2_handle h, int32_t i, char* name, int32_t name_cap, double* flops_per_image,
                    double* bytes_per_image, double* external_bytes_per_image);
/* The kernel (family) launch `i` runs, as a prefix of the symbol name a rocprofv3 kernel trace shows for it
 * (e.g. "block_s1chain_kernel", "tower2_kernel<6, 512, 4, 4>"): lets bench.py group its per-launch times the way
 * the kernel-stats tables under profiles/ do. */
YFV2_API int yfv2_stage_kernel(yfv2_handle h, int32_t i, char* name, int32_t name_cap);

/* Measurement helper (synchronises once, at the end): one untimed pass, then
 * `iters` passes of the forward queued back to back on `stream`, every launch
 * recording its own begin and end into a hipEvent pair (hipExtLaunchKernel start /
 * stop events: the dispatch's timestamps, as a rocprofv3 trace reports them; a step
 * of several launches: first begin to last end); the mean duration of each step in
 * milliseconds goes to ms[0..num_stages).  Between two passes the decode + NMS launch of
 * yfv2_detect runs untimed (thresholds 0.3 / 0.4, results discarded) where the
 * configuration has the fused form, so that a pass's first launch follows what it
 * follows in a detect loop. */
YFV2_API int yfv2_profile_forward(yfv2_handle h, const float* x, int32_t B, float* const out6[6], int32_t iters,
                         float* ms, void* stream);

/* Measurement helper: the EFFECTIVE shader clock of the device, measured by the shader itself.  `workgroups` one-wave
 * workgroups stay on the device for `milliseconds` and stamp s_memtime (shader cycles) against s_memrealtime (the constant
 * reference clock, hipDeviceAttributeWallClockRate); the quotient is the clock the wave's engine ran at over the interval -
 * DVFS, power cap and performance level included.  busy = 1: dependent FMAs between the stamps (launch >= one workgroup per
 * CU: the clock under an all-CU vector load); busy = 0: the waves sleep between looks at the reference clock and take no issue
 * slots worth naming - launched with a handful of workgroups on a SIDE stream while forwards run on the main stream, they
 * report the clock those forwards' kernels actually ran at.  yfv2_clock_probe_begin only enqueues on `stream`;
 * yfv2_clock_probe_end waits for `stream` and writes out[0..2] = min / mean / max MHz over the workgroups, out[3] = reference
 * clock in MHz, out[4] = mean measured interval in ms, out[5] = number of distinct XCDs the workgroups ran on.  bench.py puts
 * these figures next to every timing it reports (boxes of one pool differ). */
YFV2_API int yfv2_clock_probe_begin(yfv2_handle h, int32_t workgroups, float milliseconds, int32_t busy, void* stream);
YFV2_API int yfv2_clock_probe_end(yfv2_handle h, double out[6], void* stream);

/* Measurement helper: one whole forward, then launch `step` of the plan (0 .. yfv2_num_stages) `iters` times back to back on
 * `stream`; enqueue only.  A launch repeated for a few hundred milliseconds is long enough for the device's power sensor:
 * tools/power_probe.py reads it meanwhile and prices every launch in joules (the pipelined headline is power-limited). */
YFV2_API int yfv2_debug_repeat_step(yfv2_handle h, const float* x, int32_t B, float* const out6[6], int32_t step, int32_t iters, void* stream);

/* Test hook: what yfv2_detect runs after its forward, on the caller's logits out6 (the six maps of yfv2_forward, device pointers):
 * the fused decode + NMS launch where the plan and the shape allow it, otherwise decode into compact candidate rows + NMS over
 * them.  Output as yfv2_detect; enqueue only.  Lets a test feed chosen logits (ties, saturated or non-finite values) to the
 * launches yfv2_detect uses, which yfv2_decode + yfv2_nms do not reach. */
YFV2_API int yfv2_debug_post(yfv2_handle h, const float* const out6[6], int32_t B, float conf_thres, double iou_thres,
                             float* dets, int32_t* idx, int32_t* count, void* stream);

/* Debug/parity helper: copy one internal NHWC activation of the LAST forward
 * to host as (B,H,W,C).  which: 0 stem+pool, 1 stage2, 2 stage3 (C2), 3 stage4
 * (C3), 4 S2 (fpn 22x22), 5 S3 (fpn 11x11).  Returns the element count.
 * which = 0 on the default plan: the stem's output never exists in memory (it is fused into stage2.0's launch), so the hook RE-RUNS
 * the stem's own launch on the input pointer of the last forward / detect - the caller must still hold that buffer, unchanged
 * (YFV2_ERR_STATE if no forward of at least B images has run on the handle since it was created). */
YFV2_API int64_t yfv2_debug_activation(yfv2_handle h, int32_t which, int32_t B, float* host_dst, int64_t cap);

/* Debug/parity helper for the training path: the output of one ReLU'd conv+BatchNorm of the LAST yfv2_train_forward, dense
 * (B,C,H,W), copied to host.  conv_name is the state_dict prefix of its conv ("backbone.stage2.0.branch_main.0",
 * "fpn.cls_head_2.block.5", ...).  Its sign pattern is the set of ReLU decisions that execution took - the gradient parity
 * test replays the float64 oracle on exactly those decisions (tests/test_train_gpu.py).  Returns the element count (with
 * host_dst NULL or capacity too small: the count needed, nothing copied), -1 on error.  Synchronises the device. */
YFV2_API int64_t yfv2_debug_train_relu_output(yfv2_handle h, const char* conv_name, float* host_dst, int64_t capacity);
/* ... and every tensor a training kernel reads or writes, after a yfv2_train_forward and after the yfv2_train_backward that follows it
 * (the arenas are bump-allocated and the gradient arena is zeroed only at the start of a backward: all of them are intact when either
 * call has returned).  name = a conv's state_dict prefix: which = 0 the conv's output y (before BatchNorm), 1 the op's output window
 * (after BatchNorm [+ ReLU]), 2 / 3 the gradients of those two, 4 / 5 the saved batch mean / 1 / sqrt(biased variance + eps), C floats.
 * name = "backbone.maxpool", "backbone.stageS.I" (a shuffle block's concatenated output) or "fpn.p2" (the upsample + concat tensor):
 * which = 1 the value, 3 its gradient.  Dense (B,C,H,W); the contract of yfv2_debug_train_relu_output (size query with NULL, -1 and a
 * message on misuse, synchronises the device).  Gradients read before the first backward are whatever the arena holds.  An addition
 * within ABI 7. */
YFV2_API int64_t yfv2_debug_train_tensor(yfv2_handle h, const char* name, int32_t which, float* host_dst, int64_t capacity);

/* Host-only test hook: validates cfg, builds the launch plan and packs the weights exactly as yfv2_create +
 * yfv2_load_weights do, WITHOUT a device (the workspace gets made-up addresses used only for pointer arithmetic);
 * reports the number of launches and the packed blob size.  Lets the CPU test suite exercise the host logic for every
 * (classes, height, width) the configuration check admits.  Never launches or computes anything. */
YFV2_API int yfv2_debug_plan_dryrun(const yfv2_config* cfg, const yfv2_tensor_desc* tensors, int32_t n, int32_t* n_steps, int64_t* blob_floats);
/* the same for a plan other than the default (NULL = the default plan) */
YFV2_API int yfv2_debug_plan_dryrun_ex(const yfv2_config* cfg, const yfv2_plan* plan, const yfv2_tensor_desc* tensors, int32_t n, int32_t* n_steps,
                                       int64_t* blob_floats);
/* Host-only test hook: the packed LDS image of launch `step` of that plan (up to `cap` floats from the image's start) and
 * the launch's name; returns the number of floats copied or a negative error code.
 * INDEX SPACE: images are packed per reference block, so this hook numbers the steps of the IMAGE VIEW: where the default plan runs
 * the stem and stage2.0 as one launch (front2_kernel) the view still has two steps - 0 = the stem's image, 1 = stage2.0's, launch k of
 * the plan (yfv2_num_stages / yfv2_stage_info / yfv2_profile_forward / yfv2_debug_repeat_step index the LAUNCHES) = view step k + 1.
 * step = -1 returns the number of view steps (dst may be NULL).  step + 1000 (j + 1) = job j of a launch that runs several tower halves. */
YFV2_API int64_t yfv2_debug_plan_image(const yfv2_config* cfg, const yfv2_tensor_desc* tensors, int32_t n, int32_t step, char* name,
                                       int32_t name_cap, float* dst, int64_t cap);
YFV2_API int64_t yfv2_debug_plan_image_ex(const yfv2_config* cfg, const yfv2_plan* plan, const yfv2_tensor_desc* tensors, int32_t n, int32_t step,
                                          char* name, int32_t name_cap, float* dst, int64_t cap);   /* ... of a plan other than the default */
/* Host-only test hook: the channel order in which that plan stores stage 3's output C2 (label[k] = logical channel at
 * NHWC position k, 96 entries); returns 1 if the plan permutes (chain kernel), 0 for plain NHWC, negative on error. */
YFV2_API int yfv2_debug_plan_c2_label(const yfv2_config* cfg, const yfv2_tensor_desc* tensors, int32_t n, int32_t* label);
/* Host-only test hook: what the frame entry points' one launch takes and admits.  row_kind: 0 the uint8 batch of yfv2_resize_frames_* /
 * yfv2_detect_frames_*, 1 the uint8 crops of yfv2_crop_detections_*, 2 the fp32 batch of yfv2_train_batch_frames_*, 3 / 4 the fp32 /
 * fp16 tensor of yfv2_crop_tensors_*; yuv: 0 yfv2_frame, 1 yfv2_frame_yuv; w: a frame's width, 1 .. 2^26; W: the output row's width
 * (the network's, or out_w), 1 .. 2^20.  *lds_bytes = the LDS of one workgroup of that launch for a frame w wide, *max_width = the
 * widest frame the entry point admits at W (either may be NULL).  Opens no device. */
YFV2_API int yfv2_debug_rows(int32_t row_kind, int32_t yuv, int32_t w, int32_t W, int64_t* lds_bytes, int32_t* max_width);
/* ... and for yfv2_frame_yuv frames of two-byte samples (YFV2_YUV_P010 / _I010): the same arguments, checks and results.  (yuv = 1
 * above is the one-byte formats and yuv = 2 stays an argument error.)  An addition within ABI 7. */
YFV2_API int yfv2_debug_rows16(int32_t row_kind, int32_t w, int32_t W, int64_t* lds_bytes, int32_t* max_width);
/* ... and for the GENERAL one-byte launch, the one of a call with at least one frame that is not 4:2:0 (YFV2_YUV_I422 .. _GREY): the
 * same arguments, checks and results.  An addition within ABI 7. */
YFV2_API int yfv2_debug_rows_any(int32_t row_kind, int32_t w, int32_t W, int64_t* lds_bytes, int32_t* max_width);

#ifdef __cplusplus
}
#endif
#endif /* YFV2_H */
