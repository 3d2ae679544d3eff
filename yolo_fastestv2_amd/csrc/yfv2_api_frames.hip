// yfv2_api_frames.hip - host side of libyfv2.so, the entry points that take caller frames: the resize, detection on ragged
// batches of frames, and tiled detection (tile plan, merge, both in one call).  The handle and the shared plumbing: yfv2_ctx.h.
// Frames come in two kinds, yfv2_frame (packed B, G, R) and yfv2_frame_yuv (YUV planes: 4:2:0 at 8 or 10 bits, or any 8-bit sampling).  Each kind is described once
// (BgrFrames, YuvFrames: what differs); what a batch becomes is a row kind (Yfv2RowKind, yfv2_internal.h: uint8 batch, counted
// uint8 crops, training batch, fp32 / fp16 tensor), a VALUE: check_frames<Kind> turns a caller's batch into a FrameBatch under the
// row kind's width limit (yfv2_rows_max_width), enqueue_rows uploads its table and launches the rows of the resize or the training
// batch (yfv2_launch_rows), and resize_frames / train_batch_frames / detect_frames / crop_detections (yfv2_crop_tensors_* too: the
// same template with a yfv2_crop_tensor) / detect_tiled are one template each.  The extern "C" functions pass their names.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "yfv2_ctx.h"

// The host doubles of a w x h frame resized to W x H, written once: every entry point, yfv2_resize_u8 included, takes them from
// here, so a frame of a batch is resized bit for bit like that frame alone.  (This unit is built with the plain flags.)
struct FrameScales { double scale_x, scale_y, box_x, box_y; };
static FrameScales frame_scales(int w, int h, int W, int H) {
  FrameScales s;
  s.scale_x = yfv2_resize_scale(W, w);            // cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale
  s.scale_y = yfv2_resize_scale(H, h);
  s.box_x = (double)w / (double)W;                // test.py:58  scale_w = w / cfg["width"]
  s.box_y = (double)h / (double)H;
  return s;
}

// what every entry point checks of a caller's frame; `at` = "<entry point>: frame <i>: "
static int check_frame(yfv2_handle h, const std::string& at, const yfv2_frame& f) {
  if (f.height < 1 || f.width < 1) return fail(h, YFV2_ERR_ARG, at + "height and width must be >= 1");
  if (!f.data) return fail(h, YFV2_ERR_ARG, at + "null data");
  if (f.row_pitch < 3ll * f.width) return fail(h, YFV2_ERR_ARG, at + "row_pitch " + std::to_string(f.row_pitch) + " < 3 * width");
  return YFV2_OK;
}

// what every YUV entry point checks of one caller's frame - a whole frame of yfv2_detect_tiled_yuv or a frame of a batch; `at` as in
// check_frame.  The width limit is not here: it binds what is resized, which for a tiled frame are its tiles.
static int check_frame_yuv(yfv2_handle h, const std::string& at, const yfv2_frame_yuv& f) {
  if (!(f.format >= YFV2_YUV_NV12 && f.format <= YFV2_YUV_GREY) && f.format != YFV2_YUV_P010 && f.format != YFV2_YUV_I010)
    return fail(h, YFV2_ERR_ARG, at + "unknown format " + std::to_string(f.format));
  static const char* const names8[] = {"NV12", "NV21", "I420", "I422", "I440", "I444", "YUYV", "UYVY", "GREY"};
  const int sb = yfv2_yuv_sample_bytes(f.format);           // 2: every sample index below is doubled to a byte offset
  if (f.colour < YFV2_BT601_LIMITED || f.colour > YFV2_BT709_FULL) return fail(h, YFV2_ERR_ARG, at + "unknown colour " + std::to_string(f.colour));
  if (f.height < 1 || f.width < 1) return fail(h, YFV2_ERR_ARG, at + "height and width must be >= 1");
  if (f.x0 < 0 || f.y0 < 0) return fail(h, YFV2_ERR_ARG, at + "x0 and y0 must be >= 0");
  if (!f.y) return fail(h, YFV2_ERR_ARG, at + "null y");
  const bool planar = yfv2_yuv_planar(f.format), packed = yfv2_yuv_packed(f.format);
  const bool chroma = !packed && !yfv2_yuv_grey(f.format);  // the format has chroma planes: u (and v), pitch_c
  if (chroma && !f.u) return fail(h, YFV2_ERR_ARG, at + "null u");
  if (planar && !f.v) {
    std::string msg = at + "null v (" + (sb == 1 ? names8[f.format] : "I010") + ")";
    // The values 3, 4 and 5 were refused as unknown before the planar 4:2:2 / 4:4:0 / 4:4:4 formats took them, and a caller's table
    // written for two planes has no v: say what the value means now and what it got before, whichever of the two the caller meant.
    if (f.format >= YFV2_YUV_I422 && f.format <= YFV2_YUV_I444)
      msg += ": format " + std::to_string(f.format) + " takes the planes y, u and v (a library older than these formats answers \"unknown format " + std::to_string(f.format) + "\")";
    return fail(h, YFV2_ERR_ARG, msg);
  }
  if (sb == 2) {
    if (reinterpret_cast<uintptr_t>(f.y) & 1) return fail(h, YFV2_ERR_ARG, at + "y must be 2-byte aligned (two-byte samples)");
    if (reinterpret_cast<uintptr_t>(f.u) & 1) return fail(h, YFV2_ERR_ARG, at + "u must be 2-byte aligned (two-byte samples)");
    if (planar && (reinterpret_cast<uintptr_t>(f.v) & 1)) return fail(h, YFV2_ERR_ARG, at + "v must be 2-byte aligned (two-byte samples)");
    if (f.pitch_y & 1) return fail(h, YFV2_ERR_ARG, at + "pitch_y " + std::to_string(f.pitch_y) + " must be even (two-byte samples)");
    if (f.pitch_c & 1) return fail(h, YFV2_ERR_ARG, at + "pitch_c " + std::to_string(f.pitch_c) + " must be even (two-byte samples)");
  }
  const long long xe = (long long)f.x0 + f.width, ye = (long long)f.y0 + f.height;     // one past the frame's last column / row in the planes
  if (xe > 0x7fffffffll || ye > 0x7fffffffll) return fail(h, YFV2_ERR_ARG, at + "x0 + width and y0 + height must be below 2^31");
  if (packed) {                                             // up to the last macropixel's last byte: an odd last pixel reads all of it
    const long long prow = 4 * (((xe - 1) >> 1) + 1);
    if (f.pitch_y < prow)
      return fail(h, YFV2_ERR_ARG, at + "pitch_y " + std::to_string(f.pitch_y) + " < " + std::to_string(prow) + " = 4 * (((x0 + width - 1) >> 1) + 1), the last macropixel of a row (" + names8[f.format] + ")");
  } else if (f.pitch_y < sb * xe)
    return fail(h, YFV2_ERR_ARG, at + "pitch_y " + std::to_string(f.pitch_y) + (sb == 1 ? " < x0 + width" : " < 2 * (x0 + width)"));
  const int sx = yfv2_yuv_shift_x(f.format), sy = yfv2_yuv_shift_y(f.format);
  const long long crow = (((xe - 1) >> sx) + 1) * (planar ? 1 : 2) * sb;                 // chroma bytes of a row up to the frame's last sample
  if (chroma && f.pitch_c < crow) return fail(h, YFV2_ERR_ARG, at + "pitch_c " + std::to_string(f.pitch_c) + " < " + std::to_string(crow) + ", the last chroma byte of a row");
  if (f.pitch_y > (1ll << 40) || (ye - 1) * f.pitch_y > (1ll << 52)) return fail(h, YFV2_ERR_ARG, at + "pitch_y out of range");
  if (chroma && (f.pitch_c > (1ll << 40) || ((ye - 1) >> sy) * f.pitch_c > (1ll << 52))) return fail(h, YFV2_ERR_ARG, at + "pitch_c out of range");
  return YFV2_OK;
}

// A checked and expanded batch: t for every kind (frame_boxes_kernel reads box_x / box_y from it; for B, G, R frames it is the
// resize kernel's table too), yuv for YUV frames only (the resize kernel's table then); max_w sizes the resize launch's LDS.
struct FrameBatch {
  std::vector<ResizeFrame> t;
  std::vector<ResizeFrameYuv> yuv;
  int max_w = 1;
  int sample_bytes = 1;       // of a YUV batch: one launch is one instantiation, so all its frames have one sample width
  bool general = false;       // of a 1-byte YUV batch: a frame of it is not 4:2:0, so the launch is the general kind's (a property of the whole batch)
  Yfv2FrameKind kind() const { return yuv.empty() ? YFV2_FRAMES_BGR : sample_bytes == 2 ? YFV2_FRAMES_YUV16 : general ? YFV2_FRAMES_YUV8_ANY : YFV2_FRAMES_YUV8; }
};

// ---- the two kinds: only what differs.  check = one caller frame (a whole frame of a tiled call too); expand = frame b of the
// batch into its device descriptor(s), after its own last check; crop = the frame that a tile of `fr` is (the rectangle was checked).
struct BgrFrames {
  using Frame = yfv2_frame;
  static Yfv2FrameKind kind(const Frame&) { return YFV2_FRAMES_BGR; }
  static bool general(const Frame*, int32_t) { return false; }
  static int check(yfv2_handle h, const std::string& at, const Frame& f) { return check_frame(h, at, f); }
  static int expand(yfv2_handle h, const std::string& at, const Frame& f, FrameBatch& fb, size_t b) {
    if (f.row_pitch > (1ll << 40) || (long long)(f.height - 1) * f.row_pitch > (1ll << 52))
      return fail(h, YFV2_ERR_ARG, at + "row_pitch out of range");
    fb.t[b].data = f.data; fb.t[b].pitch = f.row_pitch;
    return YFV2_OK;
  }
  static Frame crop(const Frame& fr, const yfv2_tile& t) { return Frame{fr.data + (int64_t)t.y0 * fr.row_pitch + 3ll * t.x0, t.height, t.width, fr.row_pitch}; }
};

// (kernel: resize_frames_yuv_kernel, yfv2_pre.hip)  The descriptor has the origin folded into the plane pointers.
struct YuvFrames {
  using Frame = yfv2_frame_yuv;
  static Yfv2FrameKind kind(const Frame& f) { return yfv2_yuv_sample_bytes(f.format) == 2 ? YFV2_FRAMES_YUV16 : YFV2_FRAMES_YUV8; }   // (of a checked frame) by sample width
  // whether a batch of 1-byte frames needs the general launch: one of its formats is an 8-bit one that is not 4:2:0 (YFV2_YUV_I422 .. _GREY)
  static bool general(const Frame* frames, int32_t B) {
    for (int32_t b = 0; b < B; ++b)
      if (frames[b].format >= YFV2_YUV_I422 && frames[b].format <= YFV2_YUV_GREY) return true;
    return false;
  }
  static int check(yfv2_handle h, const std::string& at, const Frame& f) { return check_frame_yuv(h, at, f); }
  static int expand(yfv2_handle, const std::string&, const Frame& f, FrameBatch& fb, size_t b) {
    if (fb.yuv.empty()) fb.yuv.assign(fb.t.size(), ResizeFrameYuv{});
    ResizeFrameYuv& r = fb.yuv[b];
    fb.sample_bytes = yfv2_yuv_sample_bytes(f.format);
    r.y = f.y; r.ca = f.u; r.cb = yfv2_yuv_planar(f.format) ? f.v : nullptr;      // the planes at their own origin ...
    r.pitch_y = f.pitch_y; r.pitch_c = f.pitch_c; r.h = f.height; r.w = f.width;
    if (yfv2_yuv_packed(f.format)) {              // the one plane is both: y the luma byte of pixel (0, 0), ca the U byte of its macropixel
      r.y = f.y + (f.format == YFV2_YUV_UYVY ? 1 : 0); r.ca = f.y + (f.format == YFV2_YUV_YUYV ? 1 : 0); r.pitch_c = f.pitch_y;
    } else if (yfv2_yuv_grey(f.format)) { r.ca = nullptr; r.pitch_c = 0; }
    r.px = 0; r.py = 0; r.format = f.format; r.coef = yfv2_yuv_coef(f.colour, fb.sample_bytes);
    yfv2_yuv_move(r, f.x0, f.y0);                                                 // ... moved to the frame's (the fold, yfv2_internal.h)
    r.scale_x = fb.t[b].scale_x; r.scale_y = fb.t[b].scale_y;
    return YFV2_OK;
  }
  static Frame crop(const Frame& fr, const yfv2_tile& t) {
    Frame c = fr;
    c.x0 = fr.x0 + t.x0; c.y0 = fr.y0 + t.y0;     // (inside the frame, whose far corner is below 2^31)
    c.width = t.width; c.height = t.height;
    return c;
  }
};

// Ragged batches: every frame is checked here, before anything is enqueued, and expanded by its scales into fb.  The tables are
// B entries of the handle's max_batch, so B is bound by max_batch on every entry point.
// rows: what the frames become, which decides how wide one may be (a row kind's LDS holds the output row in its own format).
// (H, W): what the frames are resized to - the network's size on every entry point but the crops', whose caller names it.
template <class Kind>
static int check_frames(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t B, FrameBatch& fb, Yfv2RowKind rows, int H, int W) {
  const std::string w_ = what;
  if (!frames) return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  if (B < 1) return fail(h, YFV2_ERR_ARG, w_ + ": B < 1");
  if (B > h->cfg.max_batch)
    return fail(h, YFV2_ERR_BATCH, w_ + ": batch " + std::to_string(B) + " above max_batch=" + std::to_string(h->cfg.max_batch));
  Yfv2FrameKind kind = YFV2_FRAMES_BGR;      // the sample width's, of frame 0, once it is checked
  // The launch's kind is a property of the WHOLE batch, decided here, before any width is checked: one frame that is not 4:2:0 makes
  // a 1-byte batch the general kind's, whose width limit then binds every frame of the call (a frame of an unknown format is refused
  // by its own check below).
  const bool general = Kind::general(frames, B);
  int limit = 0, limit420 = 0;
  fb.t.assign((size_t)B, ResizeFrame{});
  for (int32_t b = 0; b < B; ++b) {
    const typename Kind::Frame& f = frames[b];
    const std::string at = w_ + ": frame " + std::to_string(b) + ": ";
    if (int rc = Kind::check(h, at, f)) return rc;
    if (b == 0) {
      kind = Kind::kind(f);
      fb.general = general && kind == YFV2_FRAMES_YUV8;
      limit = yfv2_rows_max_width(rows, fb.general ? YFV2_FRAMES_YUV8_ANY : kind, W);
      if (fb.general) limit420 = yfv2_rows_max_width(rows, YFV2_FRAMES_YUV8, W);
    }
    if (Kind::kind(f) != kind)
      return fail(h, YFV2_ERR_ARG, at + "format has " + (kind == YFV2_FRAMES_YUV16 ? "one-byte samples, frame 0 two-byte" : "two-byte samples, frame 0 one-byte") +
                                       " samples: the frames of one call must have one sample width");
    if (f.width > limit)
      return fail(h, YFV2_ERR_ARG, at + "frames wider than " + std::to_string(limit) + " pixels are not supported" +
                                       (fb.general ? " in a call with a frame that is not 4:2:0: its one launch holds three full-width rows per source row in LDS (a call of NV12, NV21 and I420 frames alone admits " +
                                                         std::to_string(limit420) + ")"
                                                   : std::string()));
    const FrameScales s = frame_scales(f.width, f.height, W, H);
    ResizeFrame& r = fb.t[(size_t)b];
    r.h = f.height; r.w = f.width; r.scale_x = s.scale_x; r.scale_y = s.scale_y; r.box_x = s.box_x; r.box_y = s.box_y;
    if (int rc = Kind::expand(h, at, f, fb, (size_t)b)) return rc;
    fb.max_w = std::max(fb.max_w, (int)f.width);
  }
  if ((long long)B * H > 0x7fffffffll) return fail(h, YFV2_ERR_ARG, w_ + ": batch too large");
  return YFV2_OK;
}
template <class Kind>
static int check_frames(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t B, FrameBatch& fb, Yfv2RowKind rows = YFV2_ROWS_U8) {
  return check_frames<Kind>(h, what, frames, B, fb, rows, h->cfg.height, h->cfg.width);
}

// The submit of every frame batch: ONE copy of the descriptor table into the handle's table of its kind, ONE launch reading it.
template <class D, class Launch>
static int submit_frames(yfv2_handle h, const std::vector<D>& table, void* d_table, int32_t B, hipStream_t s, Launch launch) {
  HIP_TRY(h, hipMemcpyAsync(d_table, table.data(), sizeof(D) * (size_t)B, hipMemcpyHostToDevice, s));
  launch(static_cast<const D*>(d_table));
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

// A descriptor table with each frame's (alpha, beta) behind its descriptor (NULL, NULL: the identity): the training rows' table - the
// pair travels in the one descriptor copy.
template <class D>
static auto with_augment(const std::vector<D>& src, const float* alpha, const float* beta) {
  std::vector<std::conditional_t<std::is_same_v<D, ResizeFrame>, TrainFrame, TrainFrameYuv>> t(src.size());
  for (size_t b = 0; b < src.size(); ++b) {
    static_cast<D&>(t[b]) = src[b];
    t[b].alpha = alpha ? alpha[b] : 1.0f;
    t[b].beta = beta ? beta[b] : 0.0f;
  }
  return t;
}

// Uploads the table the row kernel of the batch's kind reads and enqueues that ONE launch into dst; everything was checked.
// rows: YFV2_ROWS_U8, the resized batch, or YFV2_ROWS_TRAIN, the training batch of (alpha, beta).
static int enqueue_rows(yfv2_handle h, const FrameBatch& fb, int32_t B, Yfv2RowKind rows, void* dst, hipStream_t s, const float* alpha = nullptr,
                        const float* beta = nullptr) {
  const bool yuv = !fb.yuv.empty();
  auto submit = [&](const auto& table, void* d_table) {     // the batch's table, the handle's device table of its kind
    auto launch = [&](const void* d) { yfv2_launch_rows(rows, fb.kind(), d, B, fb.max_w, dst, h->cfg.height, h->cfg.width, s); };
    if (rows == YFV2_ROWS_TRAIN) return submit_frames(h, with_augment(table, alpha, beta), d_table, B, s, launch);
    return submit_frames(h, table, d_table, B, s, launch);
  };
  return yuv ? submit(fb.yuv, h->d_frames_yuv) : submit(fb.t, h->d_frames);
}

template <class Kind>
static int resize_frames(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t B, uint8_t* dst, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!dst) return fail(h, YFV2_ERR_ARG, std::string(what) + ": null pointer");
  if ((reinterpret_cast<uintptr_t>(dst) & 3) != 0) return fail(h, YFV2_ERR_ARG, std::string(what) + ": dst must be 4-byte aligned");
  FrameBatch fb;
  if (int rc = check_frames<Kind>(h, what, frames, B, fb)) return rc;
  DeviceGuard guard(h->device);
  return enqueue_rows(h, fb, B, YFV2_ROWS_U8, dst, static_cast<hipStream_t>(stream));
}

// yfv2_train_batch_frames_u8 / _yuv: its own arguments first, then check_frames, then each frame's pair; then the one submit.
template <class Kind>
static int train_batch_frames(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t B, const float* alpha, const float* beta,
                              float* dst, void* stream) {
  const std::string w_ = what;
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!dst) return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  if ((reinterpret_cast<uintptr_t>(dst) & 15) != 0) return fail(h, YFV2_ERR_ARG, w_ + ": dst must be 16-byte aligned");
  if (!alpha != !beta) return fail(h, YFV2_ERR_ARG, w_ + ": alpha and beta must both be given or both be NULL");
  FrameBatch fb;
  if (int rc = check_frames<Kind>(h, what, frames, B, fb, YFV2_ROWS_TRAIN)) return rc;
  for (int32_t b = 0; alpha && b < B; ++b)
    if (!std::isfinite(alpha[b]) || !std::isfinite(beta[b]))
      return fail(h, YFV2_ERR_ARG, w_ + ": frame " + std::to_string(b) + ": alpha and beta must be finite numbers");
  DeviceGuard guard(h->device);
  return enqueue_rows(h, fb, B, YFV2_ROWS_TRAIN, dst, static_cast<hipStream_t>(stream), alpha, beta);
}

// What every detection on frames does once they are checked and expanded: the handle's resized batch, the resize, then
// yfv2_detect_u8 and the frame-coordinate epilogue.  frame_boxes_kernel reads box_x / box_y from d_frames: the B, G, R resize
// has uploaded that table as its own, the YUV resize reads another, so a YUV batch uploads it here.
static int detect_frames_tail(yfv2_handle h, const FrameBatch& fb, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx,
                              int32_t* count, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(h->device);
  if (int rc = h->frames_u8.reserve(h, (size_t)h->cfg.height * h->cfg.width * 3 * (size_t)h->cfg.max_batch, true)) return rc;   // the resized batch
  if (!fb.yuv.empty()) HIP_TRY(h, hipMemcpyAsync(h->d_frames, fb.t.data(), sizeof(ResizeFrame) * (size_t)B, hipMemcpyHostToDevice, s));
  if (int rc = enqueue_rows(h, fb, B, YFV2_ROWS_U8, h->frames_u8.as<uint8_t>(), s)) return rc;
  if (int rc = yfv2_detect_u8(h, h->frames_u8.as<uint8_t>(), B, conf_thres, iou_thres, dets, idx, count, stream)) return rc;
  yfv2_launch_frame_boxes(dets, count, h->d_frames, B, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

template <class Kind>
static int detect_frames(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t B, float conf_thres, double iou_thres,
                         float* dets, int32_t* idx, int32_t* count, void* stream) {
  if (int rc = check_call(h, B, true)) return rc;
  if (!dets || !idx || !count) return fail(h, YFV2_ERR_ARG, std::string(what) + ": null pointer");
  FrameBatch fb;
  if (int rc = check_frames<Kind>(h, what, frames, B, fb)) return rc;
  return detect_frames_tail(h, fb, B, conf_thres, iou_thres, dets, idx, count, stream);
}

// ---- second-stage crops (kernels: yfv2_crops.hip and the counted instantiations of yfv2_pre.hip) -----------------
// yfv2_crop_detections_u8 / _yuv.  Every check first - the call's own arguments, then the frames under the width limit of the
// CROPS' width - then the workspace (the first call, or a larger cap: one device wait), the frame table's one copy, the two plan
// launches and the resize launch over the table's capacity.  The host never reads a count.
constexpr int CROP_MAX_R = 4096;
constexpr double CROP_MAX_PAD = 16.0;

// yfv2_crop_tensors_u8 / _yuv are the same template with `tensor` given (its dtype checked): `crops` is then the
// fp32 / fp16 tensor, 16-byte aligned, the frames are held to the tensor rows' width limit and the plan and the row launch are the
// tensor kinds'.  tensor == nullptr is yfv2_crop_detections_*, check for check and launch for launch what it was.
template <class Kind>
static int crop_detections(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t B, const float* dets, const int32_t* count, int32_t R,
                           const yfv2_crop_rule* rule, void* crops, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset, int32_t* crop_skipped,
                           int32_t cap, void* stream, const yfv2_crop_tensor* tensor = nullptr) {
  const std::string w_ = what;
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!frames || !dets || !count || !rule || !crops || !crop_src || !crop_rect || !crop_offset) return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  if (B < 1) return fail(h, YFV2_ERR_ARG, w_ + ": B < 1");
  if (R < 1 || R > CROP_MAX_R) return fail(h, YFV2_ERR_ARG, w_ + ": R must be in 1.." + std::to_string(CROP_MAX_R));
  const yfv2_crop_rule& q = *rule;
  if (q.out_h < 1) return fail(h, YFV2_ERR_ARG, w_ + ": out_h must be >= 1");
  if (q.out_w < 4 || q.out_w % 4 != 0) return fail(h, YFV2_ERR_ARG, w_ + ": out_w must be a multiple of 4, at least 4");
  if (cap < 1 || (long long)cap * q.out_h > 0x7fffffffll) return fail(h, YFV2_ERR_ARG, w_ + ": cap must be >= 1 and cap * out_h at most 2^31 - 1");
  if (!tensor && (reinterpret_cast<uintptr_t>(crops) & 3) != 0) return fail(h, YFV2_ERR_ARG, w_ + ": crops must be 4-byte aligned");
  if (tensor) {
    const yfv2_crop_tensor& t = *tensor;
    if ((reinterpret_cast<uintptr_t>(crops) & 15) != 0) return fail(h, YFV2_ERR_ARG, w_ + ": out must be 16-byte aligned");
    if (t.rgb < 0 || t.rgb > 1 || t.letterbox < 0 || t.letterbox > 1) return fail(h, YFV2_ERR_ARG, w_ + ": rgb and letterbox must be 0 or 1");
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(t.mean[c]) || !std::isfinite(t.std[c]) || !(t.std[c] > 0.f))
        return fail(h, YFV2_ERR_ARG, w_ + ": plane " + std::to_string(c) + ": mean must be finite and std finite and > 0");
  }
  if (!std::isfinite(q.pad_x) || !std::isfinite(q.pad_y) || q.pad_x < 0.f || q.pad_y < 0.f || q.pad_x > CROP_MAX_PAD || q.pad_y > CROP_MAX_PAD)
    return fail(h, YFV2_ERR_ARG, w_ + ": pad_x and pad_y must be finite numbers in [0, 16]");
  if (q.max_per_frame < 1) return fail(h, YFV2_ERR_ARG, w_ + ": max_per_frame must be >= 1");
  if (q.n_classes < 0 || (q.n_classes > 0 && !q.classes)) return fail(h, YFV2_ERR_ARG, w_ + ": n_classes < 0, or classes NULL with n_classes > 0");
  CropTensorPlanArgs a{};
  if (!q.classes) {
    for (int i = 0; i < 8; ++i) a.classes[i] = i < 7 ? 0xffffffffu : 0x7fffffffu;     // classes 0..254
  } else {
    for (int32_t i = 0; i < q.n_classes; ++i) {
      const int32_t c = q.classes[i];
      if (c < 0 || c > 254) return fail(h, YFV2_ERR_ARG, w_ + ": class " + std::to_string(c) + " outside 0..254");
      a.classes[c >> 5] |= 1u << (c & 31);
    }
  }
  const Yfv2RowKind rows = !tensor ? YFV2_ROWS_COUNTED_U8 : tensor->dtype == YFV2_F16 ? YFV2_ROWS_TENSOR_F16 : YFV2_ROWS_TENSOR_F32;
  FrameBatch fb;
  if (int rc = check_frames<Kind>(h, what, frames, B, fb, rows, q.out_h, q.out_w)) return rc;
  if ((long long)B * R > 0x7fffffffll) return fail(h, YFV2_ERR_ARG, w_ + ": B * R above 2^31 - 1");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the workspace: n_sel (max_batch int32, rounded to 16 bytes), the table's head - the tensor launches' constants and the live
  // count, the count last - and the table: cap entries of the widest kind
  const size_t n_bytes = ((sizeof(int32_t) * (size_t)h->cfg.max_batch + 15) & ~(size_t)15) + sizeof(CropTensorHead) - sizeof(CountedHead);
  const int ws_cap = std::max(cap, h->crop_cap);
  if (int rc = h->crop_ws.reserve(h, n_bytes + sizeof(CountedHead) + sizeof(TensorFrameYuv) * (size_t)ws_cap, true)) return rc;
  h->crop_cap = ws_cap;
  char* base = h->crop_ws.as<char>();
  a.dets = dets; a.count = count; a.B = B; a.R = R; a.out_h = q.out_h; a.out_w = q.out_w; a.pad_x = q.pad_x; a.pad_y = q.pad_y;
  a.max_per_frame = q.max_per_frame; a.n_sel = reinterpret_cast<int32_t*>(base); a.src = crop_src; a.rect = crop_rect; a.offset = crop_offset;
  a.skipped = crop_skipped; a.cap = cap; a.head = reinterpret_cast<CountedHead*>(base + n_bytes);
  void* table = base + n_bytes + sizeof(CountedHead);
  if (tensor) {
    for (int c = 0; c < 3; ++c) { a.p.mean[c] = tensor->mean[c]; a.p.std[c] = tensor->std[c]; }
    a.p.fill = (uint32_t)tensor->fill[0] | (uint32_t)tensor->fill[1] << 8 | (uint32_t)tensor->fill[2] << 16;
    a.p.rgb = tensor->rgb; a.letterbox = tensor->letterbox;
  }
  const bool yuv = !fb.yuv.empty();
  auto launch = [&](const void* d) {       // the plan's two launches, then the rows of the table they wrote
    yfv2_launch_crop_plan(a, tensor != nullptr, yuv, d, table, s);
    yfv2_launch_rows(rows, fb.kind(), table, cap, fb.max_w, crops, q.out_h, q.out_w, s);
  };
  return yuv ? submit_frames(h, fb.yuv, h->d_frames_yuv, B, s, launch) : submit_frames(h, fb.t, h->d_frames, B, s, launch);
}

// the tensor entry points: the handle, the struct and its dtype, which picks the row kind; then the template above
template <class Kind>
static int crop_tensors(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t B, const float* dets, const int32_t* count, int32_t R,
                        const yfv2_crop_rule* rule, const yfv2_crop_tensor* tensor, void* out, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset,
                        int32_t* crop_skipped, int32_t cap, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!tensor) return fail(h, YFV2_ERR_ARG, std::string(what) + ": null pointer");
  if (tensor->dtype != YFV2_F32 && tensor->dtype != YFV2_F16) return fail(h, YFV2_ERR_ARG, std::string(what) + ": dtype must be YFV2_F32 or YFV2_F16");
  return crop_detections<Kind>(h, what, frames, B, dets, count, R, rule, out, crop_src, crop_rect, crop_offset, crop_skipped, cap, stream, tensor);
}

extern "C" {

int yfv2_crop_letterbox(int32_t cw, int32_t ch, int32_t out_h, int32_t out_w, int32_t letterbox, int32_t inner[4]) {
  if (!inner) return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_letterbox: null pointer");
  if (cw < 1 || ch < 1 || out_h < 1 || out_w < 1) return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_letterbox: cw, ch, out_h and out_w must be >= 1");
  if (letterbox < 0 || letterbox > 1) return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_letterbox: letterbox must be 0 or 1");
  int in[4];
  yfv2_crop_letterbox_inner(cw, ch, out_h, out_w, letterbox, in);
  for (int i = 0; i < 4; ++i) inner[i] = in[i];
  return YFV2_OK;
}

int yfv2_crop_tensor_value(int32_t a, float mean, float std, float* f32, uint16_t* f16_bits) {
  if (a < 0 || a > 255) return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_tensor_value: a must be in 0..255");
  if (!std::isfinite(mean) || !std::isfinite(std) || !(std > 0.f))
    return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_tensor_value: mean must be finite and std finite and > 0");
  if (f32) *f32 = yfv2_crop_tensor_f32(a, mean, std);
  if (f16_bits) {
    const _Float16 v = yfv2_crop_tensor_f16(a, mean, std);
    std::memcpy(f16_bits, &v, 2);
  }
  return YFV2_OK;
}

int yfv2_crop_tensors_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, const float* dets, const int32_t* count, int32_t R, const yfv2_crop_rule* rule,
                         const yfv2_crop_tensor* tensor, void* out, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset, int32_t* crop_skipped,
                         int32_t cap, void* stream) {
  return crop_tensors<BgrFrames>(h, "yfv2_crop_tensors_u8", frames, B, dets, count, R, rule, tensor, out, crop_src, crop_rect, crop_offset, crop_skipped, cap, stream);
}

int yfv2_crop_tensors_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B, const float* dets, const int32_t* count, int32_t R, const yfv2_crop_rule* rule,
                          const yfv2_crop_tensor* tensor, void* out, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset, int32_t* crop_skipped,
                          int32_t cap, void* stream) {
  return crop_tensors<YuvFrames>(h, "yfv2_crop_tensors_yuv", frames, B, dets, count, R, rule, tensor, out, crop_src, crop_rect, crop_offset, crop_skipped, cap, stream);
}

int yfv2_crop_rect(const float box[4], int32_t frame_h, int32_t frame_w, float pad_x, float pad_y, int32_t rect[4]) {
  if (!box || !rect) return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_rect: null pointer");
  if (frame_h < 1 || frame_w < 1) return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_rect: frame_h and frame_w must be >= 1");
  if (!std::isfinite(pad_x) || !std::isfinite(pad_y) || pad_x < 0.f || pad_y < 0.f || pad_x > CROP_MAX_PAD || pad_y > CROP_MAX_PAD)
    return fail(nullptr, YFV2_ERR_ARG, "yfv2_crop_rect: pad_x and pad_y must be finite numbers in [0, 16]");
  int rc[4];
  if (!yfv2_crop_row_rect(box, frame_h, frame_w, pad_x, pad_y, rc)) return 0;
  for (int i = 0; i < 4; ++i) rect[i] = rc[i];
  return 1;
}

int yfv2_crop_detections_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, const float* dets, const int32_t* count, int32_t R, const yfv2_crop_rule* rule,
                            uint8_t* crops, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset, int32_t* crop_skipped, int32_t cap, void* stream) {
  return crop_detections<BgrFrames>(h, "yfv2_crop_detections_u8", frames, B, dets, count, R, rule, crops, crop_src, crop_rect, crop_offset, crop_skipped, cap, stream);
}

int yfv2_crop_detections_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B, const float* dets, const int32_t* count, int32_t R, const yfv2_crop_rule* rule,
                             uint8_t* crops, int32_t* crop_src, int32_t* crop_rect, int32_t* crop_offset, int32_t* crop_skipped, int32_t cap, void* stream) {
  return crop_detections<YuvFrames>(h, "yfv2_crop_detections_yuv", frames, B, dets, count, R, rule, crops, crop_src, crop_rect, crop_offset, crop_skipped, cap, stream);
}

int yfv2_resize_u8(yfv2_handle h, const uint8_t* src, int32_t B, int32_t src_h, int32_t src_w, uint8_t* dst, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!src || !dst || B < 1 || src_h < 1 || src_w < 1) return fail(h, YFV2_ERR_ARG, "yfv2_resize_u8: bad argument");
  if ((reinterpret_cast<uintptr_t>(dst) & 3) != 0) return fail(h, YFV2_ERR_ARG, "yfv2_resize_u8: dst must be 4-byte aligned");
  if (yfv2_rows_lds_bytes(YFV2_ROWS_U8, YFV2_FRAMES_BGR, src_w, h->cfg.width) > (size_t)YFV2_LDS_FULL || (long long)B * h->cfg.height > 0x7fffffffll)
    return fail(h, YFV2_ERR_ARG, "yfv2_resize_u8: source rows wider than " + std::to_string(yfv2_rows_max_width(YFV2_ROWS_U8, YFV2_FRAMES_BGR, h->cfg.width)) + " pixels are not supported");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const FrameScales sc = frame_scales(src_w, src_h, h->cfg.width, h->cfg.height);
  ResizeArgs a{};
  a.src = src; a.dst = dst; a.B = B; a.SH = src_h; a.SW = src_w; a.H = h->cfg.height; a.W = h->cfg.width;
  a.scale_x = sc.scale_x; a.scale_y = sc.scale_y;
  yfv2_launch_resize(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_resize_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, uint8_t* dst, void* stream) {
  return resize_frames<BgrFrames>(h, "yfv2_resize_frames_u8", frames, B, dst, stream);
}

int yfv2_resize_frames_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B, uint8_t* dst, void* stream) {
  return resize_frames<YuvFrames>(h, "yfv2_resize_frames_yuv", frames, B, dst, stream);
}

int yfv2_train_batch_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, const float* alpha, const float* beta, float* dst, void* stream) {
  return train_batch_frames<BgrFrames>(h, "yfv2_train_batch_frames_u8", frames, B, alpha, beta, dst, stream);
}

int yfv2_train_batch_frames_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B, const float* alpha, const float* beta, float* dst, void* stream) {
  return train_batch_frames<YuvFrames>(h, "yfv2_train_batch_frames_yuv", frames, B, alpha, beta, dst, stream);
}

int yfv2_detect_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, float conf_thres, double iou_thres, float* dets,
                          int32_t* idx, int32_t* count, void* stream) {
  return detect_frames<BgrFrames>(h, "yfv2_detect_frames_u8", frames, B, conf_thres, iou_thres, dets, idx, count, stream);
}

int yfv2_detect_frames_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t B, float conf_thres, double iou_thres, float* dets,
                           int32_t* idx, int32_t* count, void* stream) {
  return detect_frames<YuvFrames>(h, "yfv2_detect_frames_yuv", frames, B, conf_thres, iou_thres, dets, idx, count, stream);
}

// ---- tiled detection ----------------------------------------------------------------------------------

// One axis of the tile plan: L <= t is the single interval [0, L); otherwise tiles of length t at min(i * (t - o), L - t).
static int64_t tile_axis_count(int32_t L, int32_t t, int32_t o) {
  if (L <= t) return 1;
  const int64_t s = (int64_t)t - o;
  return ((int64_t)L - t + s - 1) / s + 1;
}

int yfv2_tile_plan(int32_t frame_h, int32_t frame_w, int32_t tile_h, int32_t tile_w, int32_t overlap_h, int32_t overlap_w,
                   int32_t include_full, yfv2_tile* tiles, int32_t cap) {
  if (frame_h < 1 || frame_w < 1 || tile_h < 1 || tile_w < 1) return fail(nullptr, YFV2_ERR_ARG, "yfv2_tile_plan: frame and tile sizes must be >= 1");
  if (overlap_h < 0 || overlap_h >= tile_h || overlap_w < 0 || overlap_w >= tile_w)
    return fail(nullptr, YFV2_ERR_ARG, "yfv2_tile_plan: overlap must be in [0, tile)");
  const int64_t ny = tile_axis_count(frame_h, tile_h, overlap_h), nx = tile_axis_count(frame_w, tile_w, overlap_w);
  const int64_t total = ny * nx + (include_full && ny * nx > 1 ? 1 : 0);
  if (total > 0x7fffffffll) return fail(nullptr, YFV2_ERR_ARG, "yfv2_tile_plan: more than 2^31 - 1 tiles");
  if (!tiles) return (int)total;
  if (cap < total) return fail(nullptr, YFV2_ERR_ARG, "yfv2_tile_plan: cap " + std::to_string(cap) + " < " + std::to_string(total) + " tiles");
  const int32_t th = std::min(tile_h, frame_h), tw = std::min(tile_w, frame_w);     // L <= t: the one interval is [0, L)
  const int64_t sy = (int64_t)tile_h - overlap_h, sx = (int64_t)tile_w - overlap_w;
  yfv2_tile* o = tiles;
  for (int64_t iy = 0; iy < ny; ++iy)
    for (int64_t ix = 0; ix < nx; ++ix, ++o) {
      o->frame = 0;
      o->y0 = (int32_t)std::min<int64_t>(iy * sy, frame_h - th);
      o->x0 = (int32_t)std::min<int64_t>(ix * sx, frame_w - tw);
      o->height = th; o->width = tw;
    }
  if (total > ny * nx) { o->frame = 0; o->x0 = 0; o->y0 = 0; o->width = frame_w; o->height = frame_h; }
  return (int)total;
}

constexpr int TILE_MAX_T = 65536, TILE_MAX_F = 65536, TILE_MAX_OUT = 4096;

// What both entry points check of the merge itself; fills the device table's host image: [T][4] x0, y0, k0, k1, then [F][2] k0, k1.
static int check_merge(yfv2_handle h, const char* what, const yfv2_tile* tiles, int32_t T, int32_t F, double merge_thres, int32_t merge_metric,
                       int32_t max_out, std::vector<int32_t>& table) {
  const std::string w_ = what;
  if (!tiles) return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  if (T < 1 || T > TILE_MAX_T) return fail(h, YFV2_ERR_ARG, w_ + ": T must be in 1.." + std::to_string(TILE_MAX_T));
  if (F < 1 || F > TILE_MAX_F) return fail(h, YFV2_ERR_ARG, w_ + ": F must be in 1.." + std::to_string(TILE_MAX_F));
  if (merge_metric != 0 && merge_metric != 1) return fail(h, YFV2_ERR_ARG, w_ + ": merge_metric must be 0 (IoU) or 1 (intersection over the smaller box)");
  if (max_out < 1 || max_out > TILE_MAX_OUT) return fail(h, YFV2_ERR_ARG, w_ + ": max_out must be in 1.." + std::to_string(TILE_MAX_OUT));
  if (!std::isfinite(merge_thres)) return fail(h, YFV2_ERR_ARG, w_ + ": merge_thres must be a finite number");
  table.assign((size_t)4 * T + (size_t)2 * F, 0);
  int32_t* fr = table.data() + (size_t)4 * T;
  for (int32_t k = 0; k < T; ++k) {
    const int32_t f = tiles[k].frame;
    if (f < 0 || f >= F) return fail(h, YFV2_ERR_ARG, w_ + ": tile " + std::to_string(k) + ": frame " + std::to_string(f) + " outside [0, F)");
    if (k > 0 && f < tiles[k - 1].frame)
      return fail(h, YFV2_ERR_ARG, w_ + ": tile " + std::to_string(k) + ": frame index decreases (a frame's tiles must be one contiguous range)");
    if (fr[2 * f + 1] == 0) fr[2 * f] = k;      // first tile of frame f
    fr[2 * f + 1] = k + 1;
  }
  for (int32_t k = 0; k < T; ++k) {
    int32_t* e = table.data() + (size_t)4 * k;
    e[0] = tiles[k].x0; e[1] = tiles[k].y0; e[2] = fr[2 * tiles[k].frame]; e[3] = fr[2 * tiles[k].frame + 1];
  }
  return YFV2_OK;
}

// the tile workspace holds the largest T and the largest F seen so far: it grows exactly when one of the two does
static int ensure_tile_ws(yfv2_handle h, int T, int F) {
  const int ct = std::max(T, h->tile_cap_t), cf = std::max(F, h->tile_cap_f);
  if (int rc = h->tile_ws.reserve(h, (size_t)ct * YFV2_MAX_DET * 32 + sizeof(int32_t) * ((size_t)4 * ct + (size_t)2 * cf), true)) return rc;
  h->tile_cap_t = ct; h->tile_cap_f = cf;
  return YFV2_OK;
}

// uploads the table and enqueues the two launches; everything was checked
static int enqueue_merge(yfv2_handle h, const float* tile_dets, const int32_t* tile_count, const std::vector<int32_t>& table, int32_t T, int32_t F,
                         double merge_thres, int32_t merge_metric, int32_t max_out, float* dets, int32_t* src, int32_t* count, hipStream_t s) {
  char* base = h->tile_ws.as<char>();
  const size_t list = (size_t)h->tile_cap_t * YFV2_MAX_DET * 16;
  int32_t* d_table = reinterpret_cast<int32_t*>(base + 2 * list);
  HIP_TRY(h, hipMemcpyAsync(d_table, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, s));
  TileMergeArgs a{};
  a.tile_dets = tile_dets; a.tile_count = tile_count; a.table = d_table; a.T = T; a.F = F;
  a.geo = reinterpret_cast<float*>(base); a.meta = reinterpret_cast<float*>(base + list);
  a.thres = merge_thres; a.metric = merge_metric; a.max_out = max_out; a.dets = dets; a.src = src; a.count = count;
  yfv2_launch_tile_merge(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_merge_tiles(yfv2_handle h, const float* tile_dets, const int32_t* tile_count, const yfv2_tile* tiles, int32_t T, int32_t F,
                     double merge_thres, int32_t merge_metric, int32_t max_out, float* dets, int32_t* src, int32_t* count, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!tile_dets || !tile_count || !dets || !count) return fail(h, YFV2_ERR_ARG, "yfv2_merge_tiles: null pointer");
  std::vector<int32_t> table;
  if (int rc = check_merge(h, "yfv2_merge_tiles", tiles, T, F, merge_thres, merge_metric, max_out, table)) return rc;
  DeviceGuard guard(h->device);
  if (int rc = ensure_tile_ws(h, T, F)) return rc;
  return enqueue_merge(h, tile_dets, tile_count, table, T, F, merge_thres, merge_metric, max_out, dets, src, count, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// yfv2_detect_tiled_u8 and yfv2_detect_tiled_yuv.  Every check comes first, in this order: the pointers, T, the merge arguments,
// each whole frame, each tile rectangle, the call, then the crops as the batch they are - checked and expanded ONCE, and handed
// to the detect tail as that batch.  Only then are the workspaces touched and anything enqueued.
template <class Kind>
static int detect_tiled(yfv2_handle h, const char* what, const typename Kind::Frame* frames, int32_t F, const yfv2_tile* tiles, int32_t T, float conf_thres,
                        double iou_thres, double merge_thres, int32_t merge_metric, int32_t max_out, float* dets, int32_t* src, int32_t* count, void* stream) {
  const std::string w_ = what;
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!frames || !tiles || !dets || !count) return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  if (T > h->cfg.max_batch)
    return fail(h, YFV2_ERR_BATCH, w_ + ": " + std::to_string(T) + " tiles above max_batch=" + std::to_string(h->cfg.max_batch));
  std::vector<int32_t> table;
  if (int rc = check_merge(h, what, tiles, T, F, merge_thres, merge_metric, max_out, table)) return rc;
  for (int32_t f = 0; f < F; ++f)
    if (int rc = Kind::check(h, w_ + ": frame " + std::to_string(f) + ": ", frames[f])) return rc;
  std::vector<typename Kind::Frame> crops((size_t)T);
  for (int32_t k = 0; k < T; ++k) {
    const yfv2_tile& t = tiles[k];
    const typename Kind::Frame& fr = frames[t.frame];
    const int32_t fw = fr.width, fh = fr.height;
    if (t.width < 1 || t.height < 1 || t.x0 < 0 || t.y0 < 0 || (int64_t)t.x0 + t.width > fw || (int64_t)t.y0 + t.height > fh)
      return fail(h, YFV2_ERR_ARG, w_ + ": tile " + std::to_string(k) + ": [" + std::to_string(t.x0) + ", " + std::to_string((int64_t)t.x0 + t.width) +
                                       ") x [" + std::to_string(t.y0) + ", " + std::to_string((int64_t)t.y0 + t.height) + ") is not a rectangle of at least one pixel inside its " +
                                       std::to_string(fw) + " x " + std::to_string(fh) + " frame");
    crops[(size_t)k] = Kind::crop(fr, t);
  }
  if (int rc = check_call(h, T, true)) return rc;
  FrameBatch fb;
  if (int rc = check_frames<Kind>(h, what, crops.data(), T, fb)) return rc;
  DeviceGuard guard(h->device);
  const size_t mb = (size_t)h->cfg.max_batch;
  if (int rc = h->tile_out.reserve(h, sizeof(float) * mb * YFV2_MAX_DET * 6 + sizeof(int32_t) * (mb * YFV2_MAX_DET + mb), true)) return rc;
  if (int rc = ensure_tile_ws(h, h->cfg.max_batch, F)) return rc;    // for max_batch tiles: no later call on this handle grows it for its tiles
  float* t_dets = h->tile_out.as<float>();
  int32_t* t_idx = reinterpret_cast<int32_t*>(t_dets + mb * YFV2_MAX_DET * 6);
  int32_t* t_count = t_idx + mb * YFV2_MAX_DET;
  if (int rc = detect_frames_tail(h, fb, T, conf_thres, iou_thres, t_dets, t_idx, t_count, stream)) return rc;
  return enqueue_merge(h, t_dets, t_count, table, T, F, merge_thres, merge_metric, max_out, dets, src, count, static_cast<hipStream_t>(stream));
}

extern "C" {

int yfv2_detect_tiled_u8(yfv2_handle h, const yfv2_frame* frames, int32_t F, const yfv2_tile* tiles, int32_t T, float conf_thres, double iou_thres,
                         double merge_thres, int32_t merge_metric, int32_t max_out, float* dets, int32_t* src, int32_t* count, void* stream) {
  return detect_tiled<BgrFrames>(h, "yfv2_detect_tiled_u8", frames, F, tiles, T, conf_thres, iou_thres, merge_thres, merge_metric, max_out, dets, src, count, stream);
}

int yfv2_detect_tiled_yuv(yfv2_handle h, const yfv2_frame_yuv* frames, int32_t F, const yfv2_tile* tiles, int32_t T, float conf_thres, double iou_thres,
                          double merge_thres, int32_t merge_metric, int32_t max_out, float* dets, int32_t* src, int32_t* count, void* stream) {
  return detect_tiled<YuvFrames>(h, "yfv2_detect_tiled_yuv", frames, F, tiles, T, conf_thres, iou_thres, merge_thres, merge_metric, max_out, dets, src, count, stream);
}

// ---- the ncnn sample's path (kernels: yfv2_deploy.hip) ----------------------------------------------------

// floats of export map `sc` per image
static size_t map_elems(const yfv2_ctx* h, int sc) { return (size_t)h->fh[sc] * h->fw[sc] * (size_t)(15 + h->cfg.classes); }

static int export_impl(yfv2_handle h, const float* const out6[6], int32_t B, float* map0, float* map1, hipStream_t s) {
  ExportMapsArgs a{};
  for (int sc = 0; sc < 2; ++sc) {
    a.reg[sc] = out6[sc * 3 + 0]; a.obj[sc] = out6[sc * 3 + 1]; a.cls[sc] = out6[sc * 3 + 2];
    a.fh[sc] = h->fh[sc]; a.fw[sc] = h->fw[sc];
  }
  a.map[0] = map0; a.map[1] = map1; a.B = B; a.classes = h->cfg.classes;
  yfv2_launch_export_maps(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_export_maps(yfv2_handle h, const float* const out6[6], int32_t B, float* map0, float* map1, void* stream) {
  if (int rc = check_call(h, B, false)) return rc;
  if (!out6 || !map0 || !map1) return fail(h, YFV2_ERR_ARG, "yfv2_export_maps: null pointer");
  for (int i = 0; i < 6; ++i)
    if (!out6[i]) return fail(h, YFV2_ERR_ARG, "yfv2_export_maps: null logit tensor");
  if (((reinterpret_cast<uintptr_t>(map0) | reinterpret_cast<uintptr_t>(map1)) & 3) != 0)
    return fail(h, YFV2_ERR_ARG, "yfv2_export_maps: the maps must be 4-byte aligned");
  DeviceGuard guard(h->device);
  return export_impl(h, out6, B, map0, map1, static_cast<hipStream_t>(stream));
}

// what both post entry points check of their own arguments, before anything is enqueued
static int check_deploy(yfv2_handle h, const char* what, float thresh, const void* boxes, const void* count, int32_t max_out) {
  const std::string w_ = what;
  if (!boxes || !count) return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  if (!(thresh >= 0.0f)) return fail(h, YFV2_ERR_ARG, w_ + ": thresh must be a number >= 0");
  if (max_out < 1 || max_out > h->rows) return fail(h, YFV2_ERR_ARG, w_ + ": max_out must be in 1.." + std::to_string(h->rows));
  return YFV2_OK;
}

// zeroes the call's `dropped` word and enqueues the post launch; everything was checked
static int post_deploy(yfv2_handle h, const float* map0, const float* map1, int32_t B, const float* scale, float thresh, float nms_thresh,
                       yfv2_target_box* boxes, int32_t* count, int32_t max_out, hipStream_t s) {
  DeployPostArgs a{};
  a.map[0] = map0; a.map[1] = map1; a.scale = scale; a.B = B; a.classes = h->cfg.classes;
  for (int sc = 0; sc < 2; ++sc) {
    a.fh[sc] = h->fh[sc]; a.fw[sc] = h->fw[sc];
    a.stride[sc] = h->cfg.height / h->fh[sc];                              // yolo-fastestv2.cpp:146, integer
  }
  for (int i = 0; i < 12; ++i) a.anchors[i] = (float)h->cfg.anchors[i];   // :34-37 std::vector<float>
  a.rows = h->rows; a.thresh = thresh; a.nms_thresh = nms_thresh;
  a.boxes = reinterpret_cast<int32_t*>(boxes); a.count = count; a.max_out = max_out;
  a.dropped = h->deploy_word.as<int32_t>();
  HIP_TRY(h, hipMemsetAsync(a.dropped, 0, sizeof(int32_t), s));
  yfv2_launch_deploy_post(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

static int reserve_deploy_word(yfv2_handle h) { return h->deploy_word.reserve(h, 16 + sizeof(float) * 2 * (size_t)h->cfg.max_batch, true); }

int yfv2_deploy_post(yfv2_handle h, const float* map0, const float* map1, int32_t B, const float* scale, float thresh, float nms_thresh,
                     yfv2_target_box* boxes, int32_t* count, int32_t max_out, void* stream) {
  if (int rc = check_call(h, B, false)) return rc;
  if (!map0 || !map1) return fail(h, YFV2_ERR_ARG, "yfv2_deploy_post: null pointer");
  if (int rc = check_deploy(h, "yfv2_deploy_post", thresh, boxes, count, max_out)) return rc;
  DeviceGuard guard(h->device);
  if (int rc = reserve_deploy_word(h)) return rc;
  return post_deploy(h, map0, map1, B, scale, thresh, nms_thresh, boxes, count, max_out, static_cast<hipStream_t>(stream));
}

int yfv2_deploy_dropped(yfv2_handle h, int32_t* dropped, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!dropped) return fail(h, YFV2_ERR_ARG, "yfv2_deploy_dropped: null pointer");
  *dropped = 0;
  if (!h->deploy_word.p) return YFV2_OK;      // no post call has run on this handle
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(h, hipMemcpyAsync(dropped, h->deploy_word.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return YFV2_OK;
}

int yfv2_detect_deploy_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, float thresh, float nms_thresh, yfv2_target_box* boxes,
                                 int32_t* count, int32_t max_out, void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if ((rc = check_deploy(h, "yfv2_detect_deploy_frames_u8", thresh, boxes, count, max_out))) return rc;
  FrameBatch fb;
  if ((rc = check_frames<BgrFrames>(h, "yfv2_detect_deploy_frames_u8", frames, B, fb))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(h->device);
  const size_t mb = (size_t)h->cfg.max_batch;
  if ((rc = h->frames_u8.reserve(h, (size_t)h->cfg.height * h->cfg.width * 3 * mb, true))) return rc;   // the resized batch
  if ((rc = h->deploy_maps.reserve(h, sizeof(float) * mb * (map_elems(h, 0) + map_elems(h, 1)), true))) return rc;
  if ((rc = reserve_deploy_word(h))) return rc;
  std::vector<float> sc((size_t)2 * B);
  for (int32_t b = 0; b < B; ++b) {                                       // yolo-fastestv2.cpp:189-190, float / float
    sc[(size_t)2 * b] = (float)frames[b].width / (float)h->cfg.width;
    sc[(size_t)2 * b + 1] = (float)frames[b].height / (float)h->cfg.height;
  }
  float* d_scale = reinterpret_cast<float*>(h->deploy_word.as<char>() + 16);
  HIP_TRY(h, hipMemcpyAsync(d_scale, sc.data(), sizeof(float) * sc.size(), hipMemcpyHostToDevice, s));
  if ((rc = enqueue_rows(h, fb, B, YFV2_ROWS_U8, h->frames_u8.as<uint8_t>(), s))) return rc;
  float* out6[6];
  for (int i = 0; i < 6; ++i) out6[i] = h->ws.logits[i].p;
  if ((rc = yfv2_forward_u8(h, h->frames_u8.as<uint8_t>(), B, out6, stream))) return rc;   // (on the handle's lanes where the plan has them)
  float* map0 = h->deploy_maps.as<float>();
  float* map1 = map0 + mb * map_elems(h, 0);
  if ((rc = export_impl(h, out6, B, map0, map1, s))) return rc;
  return post_deploy(h, map0, map1, B, d_scale, thresh, nms_thresh, boxes, count, max_out, s);
}

}  // extern "C"
