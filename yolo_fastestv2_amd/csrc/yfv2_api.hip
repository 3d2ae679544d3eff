// yfv2_api.hip - host side of libyfv2.so, first of five units: the handle's lifetime, the lanes, weights and anchors, and the
// forward / decode / NMS / detect entry points declared in include/yfv2.h (frames and tiles: yfv2_api_frames.hip; the tracker: yfv2_api_track.hip; statistics, loss,
// k-means and AP: yfv2_api_eval.hip; dry runs, probes and dumps: yfv2_api_debug.hip; the handle itself: yfv2_ctx.h).  The forward
// is a static list of launches ("plan") built once per weight load (yfv2_plan.hip); running it enqueues the launches on the
// caller's stream, nothing else.  Weight folding / re-layout: yfv2_pack.hip.
#include <algorithm>
#include <cstdio>

#include "yfv2_ctx.h"

// The plan switches, read from the environment when a handle is created (and by the host-only dry runs):
//   YFV2_FUSED=0     every reference layer its own launch (the general plan; also what shapes outside a fused kernel's
//                    static bounds get, block by block)                                 - read by PlanBuilder::build (yfv2_plan.hip)
//   YFV2_BF6=0       every pointwise conv on the fp32 MFMA; blocks whose fused kernel exists only in the bf16x6 form
//                    (the stage-3 chain, stage4.0) then run layer by layer
//   YFV2_POSTFUSE=0  yfv2_detect decodes and suppresses in two launches
//   YFV2_FRONT=0     the stem and stage2.0 as two launches (stem_h3_kernel, s2h_kernel) instead of front_kernel's one
//   YFV2_TPAIR=0     the tower halves of a level larger than 11x11 as four launches instead of two side-by-side pairs
//                                                                                       - read by PlanBuilder::pair_level
void read_plan_switches(yfv2_ctx* h, const yfv2_plan* plan) {
  h->sw.plan = read_sized(plan);
  h->sw.bf6 = !h->sw.plan.fp32_matrix;
  h->postfuse = !h->sw.plan.post_two_launches;
  h->sw.front_wanted = !h->sw.plan.front_two_launches;
}

int run_plan(yfv2_ctx* h, const void* x, bool x_u8, int B, float* const out6[6], hipStream_t stream, hipEvent_t* ev, int only_step) {
  const RunCtx c{h->d_params, x, x_u8, B, out6, stream, h->sw.bf6, h->nonfinite.dev};
  std::string err;
  if (int rc = plan_run(h->plan, c, h->d_trace, h->trace_step, ev, only_step, &err)) return fail(h, rc, err);
  if (only_step < 0) { h->last_x = x; h->last_B = B; h->last_u8 = x_u8; }
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int check_call(yfv2_ctx* h, int B, bool need_weights) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (B < 1 || B > h->cfg.max_batch)
    return fail(h, YFV2_ERR_BATCH, "batch " + std::to_string(B) + " outside [1, max_batch=" + std::to_string(h->cfg.max_batch) + "]");
  if (need_weights && !h->weights_loaded) return fail(h, YFV2_ERR_STATE, "yfv2_load_weights has not been called");
  return YFV2_OK;
}

// configuration checks shared by yfv2_create and the host-only dry run; returns the decode row count through *rows
int check_config(const yfv2_config* cfg, int* rows_out) {
  if (cfg->anchor_num != 3)
    return fail(nullptr, YFV2_ERR_CONFIG, "anchor_num must be 3 (the reference decode hard-codes 3 anchors per scale)");
  // The reference sizes everything from its .data file (utils/utils.py:13-65).  What is static here: the class index travels
  // as one byte through the NMS kernel (255 classes), and that kernel sorts an image's candidates in LDS (4096 decode rows =
  // any input up to 512x512, or e.g. 640x384).  Shapes and class counts outside the fused kernels' own bounds run on the
  // general plan, block by block (PlanBuilder); decode + NMS then run as two launches.
  if (cfg->classes < 1 || cfg->classes > 255)
    return fail(nullptr, YFV2_ERR_CONFIG, "classes must be in [1, 255]");
  if (cfg->height < 32 || cfg->width < 32 || cfg->height % 32 || cfg->width % 32)
    return fail(nullptr, YFV2_ERR_CONFIG, "height/width must be multiples of 32");
  if (cfg->max_batch < 1) return fail(nullptr, YFV2_ERR_CONFIG, "max_batch must be >= 1");
  const long long rows_ll = 3LL * ((long long)(cfg->height / 16) * (cfg->width / 16) + (long long)(cfg->height / 32) * (cfg->width / 32));
  if (rows_ll > yfv2_nms_max_rows())
    return fail(nullptr, YFV2_ERR_CONFIG, "more than " + std::to_string(yfv2_nms_max_rows()) + " decode rows per image (" + std::to_string(rows_ll) +
                                          ": inputs beyond 512x512) is not supported by the NMS kernel");
  const int rows = (int)rows_ll;
  *rows_out = rows;
  return YFV2_OK;
}

namespace {

thread_local std::string g_tls_error;
thread_local bool g_creating_lane = false;   // yfv2_create called for a child handle of a laned handle (create_lanes)

int alloc_buf(yfv2_ctx* h, Buf* b, size_t per_img) {
  b->per_img = per_img;
  HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&b->p), per_img * sizeof(float) * (size_t)h->cfg.max_batch));
  return YFV2_OK;
}

void free_buf(Buf* b) {
  if (b->p) (void)hipFree(b->p);
  b->p = nullptr;
}

size_t logit_elems(const yfv2_ctx* h, int i) { return logit_elems(h->cfg, i); }

constexpr int LANES_DEFAULT = 1, LANES_MAX = 8, LANE_MIN_IMAGES = 32;   // per slice: below that a slice is pure latency (tools/scale_probe.py)

int create_lanes(yfv2_ctx* h) {
  int n = h->sw.plan.lanes > 1 ? h->sw.plan.lanes : LANES_DEFAULT;
  if (h->d_trace || h->in_lane) n = 1;             // cycle stamps are taken on the parent's own launches
  n = n < 1 ? 1 : (n > LANES_MAX ? LANES_MAX : n);
  if (n == 1 || h->cfg.max_batch < n * LANE_MIN_IMAGES) return YFV2_OK;
  h->lane_min = n * LANE_MIN_IMAGES;
  yfv2_config c = h->cfg;
  c.max_batch = (h->cfg.max_batch + n - 1) / n;
  for (int i = 0; i < n; ++i) {
    yfv2_ctx* lane = nullptr;
    yfv2_plan lp = h->sw.plan;            // a lane runs the parent's plan, without lanes or stamps of its own
    lp.lanes = 0; lp.trace = 0;
    g_creating_lane = true;
    const int rc = yfv2_create_ex(&lane, &c, &lp);
    g_creating_lane = false;
    if (rc) return fail(h, rc, "lane " + std::to_string(i) + ": " + g_tls_error);
    lane->nonfinite.dev = h->nonfinite.dev;   // the parent's word (the lane's own `host` stays null: only the parent owns and frees it)
    h->lanes.push_back(lane);
  }
  HIP_TRY(h, hipEventCreateWithFlags(&h->lane_fork, hipEventDisableTiming));
  for (int i = 1; i < n; ++i) {
    hipStream_t st; hipEvent_t ev;
    HIP_TRY(h, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));   // non-blocking: no implicit ordering against the NULL stream, events only
    h->lane_stream.push_back(st);
    HIP_TRY(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    h->lane_join.push_back(ev);
  }
  return YFV2_OK;
}

// run `f(lane, first image, images, stream)` for every slice of a batch of B images; lane 0 on the caller's stream `s`
template <class F>
int run_lanes(yfv2_ctx* h, int B, hipStream_t s, F f) {
  const int n = (int)h->lanes.size();
  const int per = (B + n - 1) / n;
  h->last_split.clear();
  h->last_x = nullptr; h->last_B = 0;   // (this call's input is recorded slice by slice on the lanes; yfv2_debug_activation follows last_split - the
                                        // parent's own record would be a stale pointer)
  HIP_TRY(h, hipEventRecord(h->lane_fork, s));   // nothing is enqueued on a lane stream yet: a plain return is safe here
  int rc = YFV2_OK;
  auto hip_ok = [&](hipError_t e, const char* what) {     // a HIP error inside the fork / join region must NOT return early:
    if (e != hipSuccess && rc == YFV2_OK) rc = fail(h, YFV2_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return e == hipSuccess;                               // work already queued on the lane streams still has to be joined
  };
  std::vector<char> forked((size_t)n, 0);
  // lanes 1.. first: their launches are queued behind the fork before lane 0's own launches occupy the caller's stream
  for (int i = 1; i < n && rc == YFV2_OK; ++i) {
    const int off = i * per, cnt = std::min(per, B - off);
    if (cnt <= 0) break;
    if (!hip_ok(hipStreamWaitEvent(h->lane_stream[i - 1], h->lane_fork, 0), "hipStreamWaitEvent(lane fork)")) break;
    forked[(size_t)i] = 1;
    const int lrc = f(h->lanes[i], off, cnt, h->lane_stream[i - 1]);
    if (lrc) { rc = lrc; h->err = h->lanes[i]->err; }
  }
  if (rc == YFV2_OK) {
    rc = f(h->lanes[0], 0, std::min(per, B), s);
    if (rc) h->err = h->lanes[0]->err;
  }
  // the join, on every path: whatever reached a lane stream (a slice that failed half way included) is ordered in front of
  // the caller's later use of the output and workspace buffers
  for (int i = 1; i < n; ++i) {
    if (!forked[(size_t)i]) continue;
    if (hip_ok(hipEventRecord(h->lane_join[i - 1], h->lane_stream[i - 1]), "hipEventRecord(lane join)"))
      hip_ok(hipStreamWaitEvent(s, h->lane_join[i - 1], 0), "hipStreamWaitEvent(lane join)");
    else
      (void)hipStreamSynchronize(h->lane_stream[i - 1]);   // no event to wait for: the host waits instead
  }
  if (rc == YFV2_OK)
    for (int i = 0; i < n; ++i) { const int cnt = std::min(per, B - i * per); if (cnt > 0) h->last_split.push_back(cnt); }
  return rc;
}

bool use_lanes(const yfv2_ctx* h, int B) { return !h->lanes.empty() && B >= h->lane_min; }

}  // namespace

// The host half of yfv2_load_weights: check the tensors against the architecture's table (nothing is packed from an incomplete
// set), build the plan of `h` and pack its blob into wp.  A failure is the WEIGHTS code, reported on `report` (the handle of a
// real load; nullptr in a dry run), and leaves the handle with an empty plan
int build_plan(yfv2_ctx* h, WeightPacker& wp, const yfv2_tensor_desc* tensors, int32_t n, yfv2_ctx* report) {
  h->plan = Plan{};
  if (!wp.index(h->cfg, tensors, n)) return fail(report, YFV2_ERR_WEIGHTS, wp.missing);
  if (!plan_build(h->cfg, h->sw, h->ws, wp, &h->plan)) return fail(report, YFV2_ERR_WEIGHTS, "weight packing failed");
  return YFV2_OK;
}

void** yfv2_ctx_train_slot(yfv2_ctx* h) { return h ? &h->train : nullptr; }
const yfv2_config* yfv2_ctx_config(yfv2_ctx* h) { return &h->cfg; }
int yfv2_ctx_fail(yfv2_ctx* h, int code, const char* msg) {
  g_tls_error = msg ? msg : "";
  if (h) h->err = g_tls_error;
  return code;
}

DecodeArgs decode_args(yfv2_ctx* h, const float* const out6[6], int32_t B) {
  DecodeArgs a{};
  for (int sc = 0; sc < 2; ++sc) {
    a.reg[sc] = out6[sc * 3 + 0];
    a.obj[sc] = out6[sc * 3 + 1];
    a.cls[sc] = out6[sc * 3 + 2];
    a.fh[sc] = h->fh[sc];
    a.fw[sc] = h->fw[sc];
    // utils.py:332  stride = cfg["height"] / r.shape[0]  (python float -> fp32 scalar multiply)
    a.stride[sc] = (float)((double)h->cfg.height / (double)h->fh[sc]);
  }
  for (int i = 0; i < 12; ++i) a.anchors[i] = h->cfg.anchors[i];
  a.B = B;
  a.classes = h->cfg.classes;
  a.rows = h->rows;
  return a;
}

NmsArgs nms_args(const yfv2_ctx* h, const float* boxes, int compact, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx, int32_t* count) {
  NmsArgs a{};
  a.boxes = boxes; a.compact = compact; a.dets = dets; a.idx = idx; a.count = count;
  a.B = B; a.rows = h->rows; a.nc = h->cfg.classes;
  a.conf_thres = conf_thres; a.iou_thres = iou_thres;
  return a;
}

// image `off` of a batch of fp32 or uint8 images
static const void* image_at(const yfv2_ctx* h, const void* x, bool x_u8, int off) {
  return static_cast<const char*>(x) + (size_t)off * 3 * h->cfg.height * h->cfg.width * (x_u8 ? 1 : sizeof(float));
}

// ===========================================================================
// extern "C" surface
// ===========================================================================
extern "C" {

int yfv2_abi_version(void) { return YFV2_ABI_VERSION; }

const char* yfv2_last_error(yfv2_handle h) { return h ? h->err.c_str() : g_tls_error.c_str(); }

int yfv2_create(yfv2_handle* out, const yfv2_config* cfg) { return yfv2_create_ex(out, cfg, nullptr); }

int yfv2_create_ex(yfv2_handle* out, const yfv2_config* cfg, const yfv2_plan* plan) {
  if (!out || !cfg) return fail(nullptr, YFV2_ERR_ARG, "yfv2_create: null argument");
  *out = nullptr;
  int rows = 0;
  if (int rc = check_config(cfg, &rows)) return rc;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
    return fail(nullptr, YFV2_ERR_DEVICE, "no usable HIP device (this library has no CPU fallback)");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
    return fail(nullptr, YFV2_ERR_DEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, YFV2_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 (MI355X) only");

  yfv2_ctx* h = new yfv2_ctx();
  h->in_lane = g_creating_lane;
  DeviceGuard guard(cfg->device);
  int rc = setup_ctx(h, cfg, rows, alloc_buf);
  if (rc == YFV2_OK && hipMalloc(reinterpret_cast<void**>(&h->d_classes), 258 * sizeof(int32_t)) != hipSuccess)
    rc = fail(h, YFV2_ERR_DEVICE, "hipMalloc(class filter) failed");
  if (rc == YFV2_OK && hipMalloc(reinterpret_cast<void**>(&h->d_frames), sizeof(TrainFrame) * (size_t)cfg->max_batch) != hipSuccess)
    rc = fail(h, YFV2_ERR_DEVICE, "hipMalloc(frame table) failed");
  if (rc == YFV2_OK && hipMalloc(reinterpret_cast<void**>(&h->d_frames_yuv), sizeof(TrainFrameYuv) * (size_t)cfg->max_batch) != hipSuccess)
    rc = fail(h, YFV2_ERR_DEVICE, "hipMalloc(YUV frame table) failed");
  if (rc == YFV2_OK) {
    h->d_stats_flag = h->d_classes + 256;
    if (hipMemset(h->d_stats_flag, 0, 2 * sizeof(int32_t)) != hipSuccess) rc = fail(h, YFV2_ERR_DEVICE, "hipMemset(flags) failed");
  }
  if (rc == YFV2_OK && !h->in_lane) {
    if (!h->nonfinite.alloc()) rc = fail(h, YFV2_ERR_DEVICE, "hipHostMalloc(range-guard word) failed");
    else *reinterpret_cast<volatile int32_t*>(h->nonfinite.host) = 0;
  }
  if (rc != YFV2_OK) {
    g_tls_error = h->err;
    yfv2_destroy(h);
    return rc;
  }
  read_plan_switches(h, plan);
  if (h->sw.plan.trace) {
    h->trace_step = h->sw.plan.trace_step;
    (void)hipMalloc(reinterpret_cast<void**>(&h->d_trace), 8192 * sizeof(long long));
    (void)hipMemset(h->d_trace, 0, 8192 * sizeof(long long));
  }
  if (int rc2 = create_lanes(h)) { g_tls_error = h->err; yfv2_destroy(h); return rc2; }
  *out = h;
  return YFV2_OK;
}

void yfv2_destroy(yfv2_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  h->ws.for_each(h->cfg, h->rows, [](Buf& b, size_t) { free_buf(&b); });
  if (h->d_classes) (void)hipFree(h->d_classes);
  if (h->d_frames) (void)hipFree(h->d_frames);
  if (h->d_frames_yuv) (void)hipFree(h->d_frames_yuv);
  if (h->d_probe) (void)hipFree(h->d_probe);
  if (h->train) { yfv2_train_release(h->train); h->train = nullptr; }
  if (h->d_params) (void)hipFree(h->d_params);
  for (yfv2_ctx* lane : h->lanes) yfv2_destroy(lane);
  for (hipStream_t st : h->lane_stream) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  for (hipEvent_t ev : h->lane_join) (void)hipEventDestroy(ev);
  if (h->lane_fork) (void)hipEventDestroy(h->lane_fork);
  delete h;   // (the DeviceBlock and MappedWord members release themselves here, on the handle's device)
}

int yfv2_load_weights(yfv2_handle h, const yfv2_tensor_desc* tensors, int32_t n) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!tensors || n <= 0) return fail(h, YFV2_ERR_ARG, "yfv2_load_weights: no tensors");
  DeviceGuard guard(h->device);
  WeightPacker wp;
  if (int rc = build_plan(h, wp, tensors, n, h)) {
    h->weights_loaded = false;
    return rc;
  }
  HIP_TRY(h, hipDeviceSynchronize());  // nothing of ours may still read the old blob
  if (h->d_params && h->n_params < wp.blob.size()) { (void)hipFree(h->d_params); h->d_params = nullptr; }
  if (!h->d_params) {
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_params), wp.blob.size() * sizeof(float)));
    h->n_params = wp.blob.size();
  }
  HIP_TRY(h, hipMemcpy(h->d_params, wp.blob.data(), wp.blob.size() * sizeof(float), hipMemcpyHostToDevice));
  h->weights_loaded = true;
  for (yfv2_ctx* lane : h->lanes)
    if (int rc = yfv2_load_weights(lane, tensors, n)) { h->weights_loaded = false; return fail(h, rc, lane->err); }
  return YFV2_OK;
}

int yfv2_set_anchors(yfv2_handle h, const double anchors[12]) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!anchors) return fail(h, YFV2_ERR_ARG, "yfv2_set_anchors: null pointer");
  for (int i = 0; i < 12; ++i) h->cfg.anchors[i] = anchors[i];
  for (yfv2_ctx* lane : h->lanes) (void)yfv2_set_anchors(lane, anchors);
  return YFV2_OK;
}

// yfv2_forward / yfv2_forward_u8: `x` is (B, 3, H, W) fp32 or (x_u8) uint8 - one byte or four per element is all that differs
static int forward_impl(yfv2_handle h, const void* x, bool x_u8, int32_t B, float* const out6[6], void* stream) {
  const std::string name = x_u8 ? "yfv2_forward_u8" : "yfv2_forward";
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (!x || !out6) return fail(h, YFV2_ERR_ARG, name + ": null pointer");
  for (int i = 0; i < 6; ++i)
    if (!out6[i]) return fail(h, YFV2_ERR_ARG, name + ": null output tensor");
  DeviceGuard guard(h->device);
  if (use_lanes(h, B))
    return run_lanes(h, B, static_cast<hipStream_t>(stream), [&](yfv2_ctx* lane, int off, int cnt, hipStream_t st) {
      float* o6[6];
      for (int i = 0; i < 6; ++i) o6[i] = out6[i] + (size_t)off * logit_elems(h, i);
      return forward_impl(lane, image_at(h, x, x_u8, off), x_u8, cnt, o6, st);
    });
  h->last_split.clear();
  return run_plan(h, x, x_u8, B, out6, static_cast<hipStream_t>(stream), nullptr);
}
int yfv2_forward(yfv2_handle h, const float* x, int32_t B, float* const out6[6], void* stream) { return forward_impl(h, x, false, B, out6, stream); }
int yfv2_forward_u8(yfv2_handle h, const uint8_t* x, int32_t B, float* const out6[6], void* stream) { return forward_impl(h, x, true, B, out6, stream); }

// handel_preds + non_max_suppression of the logits out6 (h->logits behind a forward): one launch that decodes each image into
// LDS (default), or decode_kernel<compact> + nms_kernel over candidate rows in HBM (YFV2_POSTFUSE=0, the A/B reference)
static int post_impl(yfv2_handle h, const float* const out6[6], int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx,
                     int32_t* count, void* stream);
static int decode_impl(yfv2_handle h, const float* const out6[6], int32_t B, float* boxes, float* cand, void* stream);
static int nms_impl(yfv2_handle h, const float* boxes, int compact, int32_t B, float conf_thres, double iou_thres,
                    const int32_t* classes, int32_t n_classes, float* dets, int32_t* idx, int32_t* count, void* stream);

int yfv2_decode(yfv2_handle h, const float* const out6[6], int32_t B, float* boxes, void* stream) {
  return decode_impl(h, out6, B, boxes, nullptr, stream);
}

static int decode_impl(yfv2_handle h, const float* const out6[6], int32_t B, float* boxes, float* cand, void* stream) {
  int rc = check_call(h, B, false);
  if (rc) return rc;
  if (!out6 || (!boxes && !cand)) return fail(h, YFV2_ERR_ARG, "yfv2_decode: null pointer");
  for (int i = 0; i < 6; ++i)
    if (!out6[i]) return fail(h, YFV2_ERR_ARG, "yfv2_decode: null logit tensor");
  DeviceGuard guard(h->device);
  DecodeArgs a = decode_args(h, out6, B);
  a.boxes = boxes;
  a.cand = cand;
  yfv2_launch_decode(a, static_cast<hipStream_t>(stream));
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_nms(yfv2_handle h, const float* boxes, int32_t B, float conf_thres, double iou_thres, const int32_t* classes,
             int32_t n_classes, float* dets, int32_t* idx, int32_t* count, void* stream) {
  return nms_impl(h, boxes, 0, B, conf_thres, iou_thres, classes, n_classes, dets, idx, count, stream);
}

static int nms_impl(yfv2_handle h, const float* boxes, int compact, int32_t B, float conf_thres, double iou_thres,
                    const int32_t* classes, int32_t n_classes, float* dets, int32_t* idx, int32_t* count, void* stream) {
  int rc = check_call(h, B, false);
  if (rc) return rc;
  if (!boxes || !dets || !idx || !count) return fail(h, YFV2_ERR_ARG, "yfv2_nms: null pointer");
  if (n_classes < 0 || n_classes > 256 || (n_classes > 0 && !classes))
    return fail(h, YFV2_ERR_ARG, "yfv2_nms: bad class filter");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  NmsArgs a = nms_args(h, boxes, compact, B, conf_thres, iou_thres, dets, idx, count);
  if (n_classes > 0) {  // classes is a HOST array (python list in the reference, utils.py:271-272)
    HIP_TRY(h, hipMemcpyAsync(h->d_classes, classes, sizeof(int32_t) * n_classes, hipMemcpyHostToDevice, s));
    a.classes = h->d_classes; a.n_classes = n_classes;
  }
  yfv2_launch_nms(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

// yfv2_detect / yfv2_detect_u8: the forward into the handle's own logits, then the post launch
static int detect_impl(yfv2_handle h, const void* x, bool x_u8, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx,
                       int32_t* count, void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (use_lanes(h, B)) {
    if (!x || !dets || !idx || !count) return fail(h, YFV2_ERR_ARG, std::string(x_u8 ? "yfv2_detect_u8" : "yfv2_detect") + ": null pointer");
    DeviceGuard guard(h->device);
    return run_lanes(h, B, static_cast<hipStream_t>(stream), [&](yfv2_ctx* lane, int off, int cnt, hipStream_t st) {
      return detect_impl(lane, image_at(h, x, x_u8, off), x_u8, cnt, conf_thres, iou_thres, dets + (size_t)off * YFV2_MAX_DET * 6,
                         idx + (size_t)off * YFV2_MAX_DET, count + off, st);
    });
  }
  // post_impl's check, in front of the forward's enqueue (a null x is the forward's to report)
  if (x && (!dets || !idx || !count)) return fail(h, YFV2_ERR_ARG, "yfv2_detect: null pointer");
  float* out6[6];
  for (int i = 0; i < 6; ++i) out6[i] = h->ws.logits[i].p;
  rc = forward_impl(h, x, x_u8, B, out6, stream);
  if (rc) return rc;
  return post_impl(h, out6, B, conf_thres, iou_thres, dets, idx, count, stream);
}
int yfv2_detect(yfv2_handle h, const float* x, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx, int32_t* count, void* stream) {
  return detect_impl(h, x, false, B, conf_thres, iou_thres, dets, idx, count, stream);
}
int yfv2_detect_u8(yfv2_handle h, const uint8_t* x, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx, int32_t* count, void* stream) {
  return detect_impl(h, x, true, B, conf_thres, iou_thres, dets, idx, count, stream);
}

int yfv2_debug_post(yfv2_handle h, const float* const out6[6], int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx,
                    int32_t* count, void* stream) {
  int rc = check_call(h, B, false);
  if (rc) return rc;
  if (!out6) return fail(h, YFV2_ERR_ARG, "yfv2_debug_post: null pointer");
  for (int i = 0; i < 6; ++i)
    if (!out6[i]) return fail(h, YFV2_ERR_ARG, "yfv2_debug_post: null logit tensor");
  return post_impl(h, out6, B, conf_thres, iou_thres, dets, idx, count, stream);
}

static int post_impl(yfv2_handle h, const float* const out6[6], int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx,
                     int32_t* count, void* stream) {
  if (!dets || !idx || !count) return fail(h, YFV2_ERR_ARG, "yfv2_detect: null pointer");
  if (!h->postfuse || !yfv2_post_fusable(h->cfg.classes, h->rows)) {
    // compact candidate rows instead of the (B,1815,85) tensor: same arithmetic, 10x less traffic
    const int rc = decode_impl(h, out6, B, nullptr, h->ws.cand.p, stream);
    if (rc) return rc;
    return nms_impl(h, h->ws.cand.p, 1, B, conf_thres, iou_thres, nullptr, 0, dets, idx, count, stream);
  }
  DeviceGuard guard(h->device);
  NmsArgs a = nms_args(h, nullptr, 1, B, conf_thres, iou_thres, dets, idx, count);
  a.trace = h->trace_step == -2 ? h->d_trace : nullptr;   // YFV2_TRACE=1 YFV2_TRACE_STEP=-2: stamps of the post launch (tools/trace_post.py)
  yfv2_launch_decode_nms(decode_args(h, out6, B), a, static_cast<hipStream_t>(stream));
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

// the sticky range-guard word of the fp16x3 plan (Yfv2Watch, yfv2_device.h): waits for `stream`, reports and clears it
int yfv2_nonfinite(yfv2_handle h, int32_t* flag, void* stream) {
  if (!h || !flag) return fail(h, YFV2_ERR_ARG, "yfv2_nonfinite: null argument");
  if (!h->nonfinite.host) return fail(h, YFV2_ERR_STATE, "yfv2_nonfinite: this handle owns no guard word");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(h, hipStreamSynchronize(s));        // a kernel's stores to coherent host memory are visible once it has completed
  volatile int32_t* w = h->nonfinite.host;
  const int32_t v = *w;
  if (v) *w = 0;
  *flag = v ? 1 : 0;
  return YFV2_OK;
}

// ... and without waiting for anything: what has landed in the word so far (not cleared).  A caller that never synchronises
// with the host (a detect loop that hands device tensors on) looks before every call and learns of a tripped guard one call late
// instead of never.
int yfv2_nonfinite_peek(yfv2_handle h, int32_t* flag) {
  if (!h || !flag) return fail(h, YFV2_ERR_ARG, "yfv2_nonfinite_peek: null argument");
  if (!h->nonfinite.host) return fail(h, YFV2_ERR_STATE, "yfv2_nonfinite_peek: this handle owns no guard word");
  *flag = *reinterpret_cast<volatile int32_t*>(h->nonfinite.host) ? 1 : 0;
  return YFV2_OK;
}

int32_t yfv2_num_rows(yfv2_handle h) { return h ? h->rows : 0; }

int32_t yfv2_num_stages(yfv2_handle h) { return h ? (int32_t)h->plan.steps.size() : 0; }

int yfv2_stage_info(yfv2_handle h, int32_t i, char* name, int32_t name_cap, double* flops_per_image, double* bytes_per_image,
                    double* external_bytes_per_image) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (i < 0 || i >= (int32_t)h->plan.steps.size()) return fail(h, YFV2_ERR_ARG, "stage index out of range");
  const Step& s = h->plan.steps[i];
  if (name && name_cap > 0) std::snprintf(name, (size_t)name_cap, "%s", s.name.c_str());
  if (flops_per_image) *flops_per_image = s.flops;
  if (bytes_per_image) *bytes_per_image = s.bytes;
  if (external_bytes_per_image) *external_bytes_per_image = s.bytes_ext >= 0 ? s.bytes_ext : s.bytes;
  return YFV2_OK;
}

int yfv2_stage_kernel(yfv2_handle h, int32_t i, char* name, int32_t name_cap) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (i < 0 || i >= (int32_t)h->plan.steps.size() || !name || name_cap < 1) return fail(h, YFV2_ERR_ARG, "yfv2_stage_kernel: bad argument");
  std::snprintf(name, (size_t)name_cap, "%s", step_kernel(h->plan.steps[i]).c_str());
  return YFV2_OK;
}

}  // extern "C"
