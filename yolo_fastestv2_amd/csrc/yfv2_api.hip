// yfv2_api.hip - host side of libyfv2.so: the handle, the lanes, the dry-run hooks and the extern "C" entry points declared in
// include/yfv2.h.  The forward is a static list of launches ("plan") built once per weight load (yfv2_plan.hip); running it
// enqueues the launches on the caller's stream, nothing else.  Weight folding / re-layout: yfv2_pack.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/yfv2.h"
#include "yfv2_internal.h"
#include "yfv2_pack.h"
#include "yfv2_plan.h"

namespace {

thread_local std::string g_tls_error;
thread_local bool g_creating_lane = false;   // yfv2_create called for a child handle of a laned handle (create_lanes)

}  // namespace

struct yfv2_ctx {
  yfv2_config cfg{};
  int device = 0;
  std::string err;
  bool weights_loaded = false;
  int rows = 0;
  int fh[2] = {0, 0}, fw[2] = {0, 0};

  float* d_params = nullptr;
  size_t n_params = 0;
  Plan plan;           // empty until yfv2_load_weights succeeds
  Workspace ws;
  const void* last_x = nullptr; int last_B = 0; bool last_u8 = false;   // the input of the last forward run on THIS handle's workspace (a raw caller pointer: yfv2_debug_activation(0) re-reads it)
  PlanSwitches sw;          // yfv2_create_ex
  bool postfuse = true;     // yfv2_detect: decode + NMS as one launch (yfv2_plan.post_two_launches: two launches)
  int32_t* d_classes = nullptr;  // class filter scratch (<= 256 entries), then one int32 of its own for the statistics overflow flag
  int32_t* d_stats_flag = nullptr;  // = d_classes + 256
  ResizeFrame* d_frames = nullptr;   // frame descriptors of yfv2_resize_frames_u8 / yfv2_detect_frames_u8 (max_batch entries)
  uint8_t* d_frames_u8 = nullptr;    // yfv2_detect_frames_u8's resized batch (max_batch, H, W, 3): allocated by its first call
  // tiled detection (yfv2_merge_tiles / yfv2_detect_tiled_u8).  d_tile_ws: the ordered candidate lists of tile_cap_t tiles (two float4
  // per row) and the tile / frame table of tile_cap_t + tile_cap_f entries; allocated by the first call, grown (one device wait) only by
  // a call with more tiles or frames than any before.  d_tile_out: yfv2_detect_tiled_u8's per-tile results (max_batch, 300, 6) +
  // idx (max_batch, 300) + count (max_batch), allocated by its first call.
  void* d_tile_ws = nullptr;
  int tile_cap_t = 0, tile_cap_f = 0;
  float* d_tile_out = nullptr;
  // the sticky range-guard word of the fp16x3 plan (yfv2_nonfinite): ONE int32 in host-mapped, coherent memory.  The kernels
  // store 1 into it through d_nonfinite (the rare path, a plain store); the host reads h_nonfinite - after waiting for a stream
  // (yfv2_nonfinite: exact) or without waiting (yfv2_nonfinite_peek: what has landed so far).  A lane uses its parent's word.
  int32_t* h_nonfinite = nullptr;
  int32_t* d_nonfinite = nullptr;
  unsigned long long* d_probe = nullptr;   // yfv2_clock_probe_*: [probe_wgs][4] stamps of the last probe launch
  int probe_wgs = 0;
  // training-loss workspace (yfv2_loss): match slots for loss_cap labels, objectness target maps for max_batch images,
  // counters and float64 sums; grown on demand (a growth waits for the device)
  void* d_loss_ws = nullptr;
  size_t loss_ws_bytes = 0;
  // anchor k-means (yfv2_anchor_kmeans): chunk partials, the device `done` word and, when the caller wants no assignments, N
  // int32 of them; grown on demand (a growth waits for the device).  km_word: int32[5] in host-mapped, coherent memory that the
  // finalise launch publishes its verdict to (allocated by the first call)
  void* d_km_ws = nullptr;
  size_t km_ws_bytes = 0;
  int32_t* h_km_word = nullptr;
  int32_t* d_km_word = nullptr;
  int km_group = 8;              // passes enqueued between two looks at km_word (yfv2_debug_kmeans_group); changes no output bit
  // average precision (yfv2_ap_per_class): the result head, the sort's table and ping-pong buffers, the chunk sums (yfv2_ap.hip);
  // grown on demand (a growth waits for the device)
  void* d_ap_ws = nullptr;
  size_t ap_ws_bytes = 0;
  void* train = nullptr;         // training state (yfv2_train.hip), created by yfv2_train_bind
  long long* d_trace = nullptr;  // YFV2_TRACE=1: cycle stamps of the last fused s1 launch (debug)
  int trace_step = -1;           // YFV2_TRACE_STEP=i: only launch i of the plan writes stamps (towers: only then)
  // LANES (YFV2_LANES=N in the environment of yfv2_create): yfv2_forward / yfv2_detect (and their uint8
  // forms) of at least lane_min images cut the batch into N contiguous slices; slice i is run by child handle lanes[i] (own
  // workspace sized max_batch / N, own plan, its own copy of the 1 MB weight blob) on stream lane_stream[i] - lane 0 on the
  // caller's stream - forked from and joined back into the caller's stream with events INSIDE the call: the caller still
  // orders against one stream.  Images are independent, so the result is bit-identical to the unsliced call;
  // what changes is that the one-workgroup-per-image launches of one slice (stages 3 / 4, towers, decode + NMS) share the
  // machine with the streaming launches of another instead of each leaving it under-filled.
  std::vector<yfv2_ctx*> lanes;
  std::vector<hipStream_t> lane_stream;    // [n_lanes - 1]
  std::vector<hipEvent_t> lane_join;       // [n_lanes - 1]
  hipEvent_t lane_fork = nullptr;
  int lane_min = 0;
  bool in_lane = false;                    // this handle IS a lane of another one (never laned itself)
  std::vector<int> last_split;             // slice sizes of the last forward if it ran on the lanes (yfv2_debug_activation)
};

namespace {

int fail(yfv2_ctx* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  g_tls_error = msg;
  return code;
}

#define HIP_TRY(h, expr)                                                                      \
  do {                                                                                        \
    hipError_t e__ = (expr);                                                                  \
    if (e__ != hipSuccess)                                                                    \
      return fail(h, YFV2_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));    \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

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
  h->sw.plan = yfv2_plan{};
  if (plan) {   // (a caller built against an older, shorter struct: the fields it does not have stay 0)
    const size_t n = plan->struct_size > 0 && (size_t)plan->struct_size < sizeof(yfv2_plan) ? (size_t)plan->struct_size : sizeof(yfv2_plan);
    std::memcpy(&h->sw.plan, plan, n);
  }
  h->sw.plan.struct_size = (int32_t)sizeof(yfv2_plan);
  h->sw.bf6 = !h->sw.plan.fp32_matrix;
  h->postfuse = !h->sw.plan.post_two_launches;
  h->sw.front_wanted = !h->sw.plan.front_two_launches;
}

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

int run_plan(yfv2_ctx* h, const void* x, bool x_u8, int B, float* const out6[6], hipStream_t stream, hipEvent_t* ev /*nullable: 2 per step*/,
             int only_step = -1 /* >= 0: this launch alone (yfv2_debug_repeat_step) */) {
  const RunCtx c{h->d_params, x, x_u8, B, out6, stream, h->sw.bf6, h->d_nonfinite};
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

// geometry + workspace of a handle; `alloc` is alloc_buf (device memory) or the dry run's address generator
template <class Alloc>
int setup_ctx(yfv2_ctx* h, const yfv2_config* cfg, int rows, Alloc alloc) {
  h->cfg = *cfg;
  h->device = cfg->device;
  h->rows = rows;
  h->fh[0] = cfg->height / 16; h->fw[0] = cfg->width / 16;
  h->fh[1] = cfg->height / 32; h->fw[1] = cfg->width / 32;
  int rc = YFV2_OK;
  h->ws.for_each(h->cfg, rows, [&](Buf& b, size_t per_img) { if (rc == YFV2_OK) rc = alloc(h, &b, per_img); });
  return rc;
}

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
    lane->d_nonfinite = h->d_nonfinite;   // the parent's word (its h_nonfinite stays null: only the parent owns and frees it)
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

// The host half of yfv2_load_weights: index the tensors, build the plan of `h` and pack its blob into wp.  A failure is the
// WEIGHTS code with the packer's message, reported on `report` (the handle of a real load; nullptr in a dry run), and
// leaves the handle with an empty plan
int build_plan(yfv2_ctx* h, WeightPacker& wp, const yfv2_tensor_desc* tensors, int32_t n, yfv2_ctx* report) {
  wp.index(tensors, n);
  h->plan = Plan{};
  if (!plan_build(h->cfg, h->sw, h->ws, wp, &h->plan)) return fail(report, YFV2_ERR_WEIGHTS, wp.missing.empty() ? "weight packing failed" : wp.missing);
  return YFV2_OK;
}

// What yfv2_create + yfv2_load_weights do on the host, without a device: the configuration check, a handle whose workspace
// gets made-up addresses that are only ever used for pointer arithmetic, the plan and the packed blob.
struct DryRun {
  yfv2_ctx ctx;
  WeightPacker wp;
  int build(const yfv2_config* cfg, const yfv2_plan* plan, const yfv2_tensor_desc* tensors, int32_t n) {
    int rows = 0;
    if (int rc = check_config(cfg, &rows)) return rc;
    uintptr_t next = 0x100000000ull;
    auto fake = [&](yfv2_ctx* hh, Buf* b, size_t per_img) {
      b->per_img = per_img;
      b->p = reinterpret_cast<float*>(next);
      next += (per_img * sizeof(float) * (size_t)hh->cfg.max_batch + 4095) & ~(uintptr_t)4095;
      return (int)YFV2_OK;
    };
    setup_ctx(&ctx, cfg, rows, fake);
    read_plan_switches(&ctx, plan);
    return build_plan(&ctx, wp, tensors, n, nullptr);
  }
};

}  // namespace

void** yfv2_ctx_train_slot(yfv2_ctx* h) { return h ? &h->train : nullptr; }
const yfv2_config* yfv2_ctx_config(yfv2_ctx* h) { return &h->cfg; }
int yfv2_ctx_fail(yfv2_ctx* h, int code, const char* msg) { return fail(h, code, msg ? msg : ""); }

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
  if (rc == YFV2_OK && hipMalloc(reinterpret_cast<void**>(&h->d_frames), sizeof(ResizeFrame) * (size_t)cfg->max_batch) != hipSuccess)
    rc = fail(h, YFV2_ERR_DEVICE, "hipMalloc(frame table) failed");
  if (rc == YFV2_OK) {
    h->d_stats_flag = h->d_classes + 256;
    if (hipMemset(h->d_stats_flag, 0, 2 * sizeof(int32_t)) != hipSuccess) rc = fail(h, YFV2_ERR_DEVICE, "hipMemset(flags) failed");
  }
  if (rc == YFV2_OK && !h->in_lane) {
    void* hp = nullptr; void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
      if (hp) (void)hipHostFree(hp);
      rc = fail(h, YFV2_ERR_DEVICE, "hipHostMalloc(range-guard word) failed");
    } else {
      h->h_nonfinite = static_cast<int32_t*>(hp);
      h->d_nonfinite = static_cast<int32_t*>(dp);
      *reinterpret_cast<volatile int32_t*>(h->h_nonfinite) = 0;
    }
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

// Host-only test hook (CPU suite): validate `cfg`, build the launch plan and pack the weights exactly as
// yfv2_create + yfv2_load_weights do, but without a device - the workspace gets made-up addresses that are only ever
// used for pointer arithmetic.  Reports the number of launches and the size of the packed parameter blob.
int yfv2_debug_plan_dryrun(const yfv2_config* cfg, const yfv2_tensor_desc* tensors, int32_t n, int32_t* n_steps, int64_t* blob_floats) {
  return yfv2_debug_plan_dryrun_ex(cfg, nullptr, tensors, n, n_steps, blob_floats);
}

int yfv2_debug_plan_dryrun_ex(const yfv2_config* cfg, const yfv2_plan* plan, const yfv2_tensor_desc* tensors, int32_t n, int32_t* n_steps, int64_t* blob_floats) {
  if (!cfg || !tensors || n <= 0) return fail(nullptr, YFV2_ERR_ARG, "yfv2_debug_plan_dryrun: bad argument");
  DryRun d;
  if (int rc = d.build(cfg, plan, tensors, n)) return rc;
  for (const Step& st : d.ctx.plan.steps)
    if (step_image(st) > d.wp.blob.size()) return fail(nullptr, YFV2_ERR_WEIGHTS, "step '" + st.name + "': image offset outside the blob");
  if (n_steps) *n_steps = (int32_t)d.ctx.plan.steps.size();
  if (blob_floats) *blob_floats = (int64_t)d.wp.blob.size();
  return YFV2_OK;
}

// Host-only test hook: the packed LDS image of launch `step` (or of one of its jobs, see below) of the plan the dry run builds (at most `cap` floats from the
// image's start to the end of the blob), and the launch's name.  Lets the CPU suite check host packing against a
// numpy model of a kernel's dataflow.  Returns the number of floats copied or a negative error code.
int64_t yfv2_debug_plan_image(const yfv2_config* cfg, const yfv2_tensor_desc* tensors, int32_t n, int32_t step, char* name, int32_t name_cap,
                              float* dst, int64_t cap) {
  return yfv2_debug_plan_image_ex(cfg, nullptr, tensors, n, step, name, name_cap, dst, cap);
}

int64_t yfv2_debug_plan_image_ex(const yfv2_config* cfg, const yfv2_plan* plan, const yfv2_tensor_desc* tensors, int32_t n, int32_t step, char* name,
                                 int32_t name_cap, float* dst, int64_t cap) {
  if (!cfg || !tensors || n <= 0 || (step != -1 && (!dst || cap <= 0))) return fail(nullptr, YFV2_ERR_ARG, "yfv2_debug_plan_image: bad argument");
  DryRun d;
  if (int rc = d.build(cfg, plan, tensors, n)) return rc;
  // step + 1000 (k + 1): job k of a launch that runs several tower halves (towers_kernel's list, towerh_kernel's side-by-side pair)
  const int job = step >= 1000 ? step / 1000 - 1 : -1;
  if (step >= 1000) step %= 1000;
  // the images are those of the launches as packed: under front_kernel (one launch for the stem and stage2.0) the stem's step is
  // put back in front and stage2.0 answers to its own name - step indices are those of the two-launch plan
  std::vector<Step> view = d.ctx.plan.steps;
  if (d.ctx.plan.front_fused) { view.insert(view.begin(), d.ctx.plan.stem_aside); view[1].name = std::get<S2PxStep>(view[1].kind).name_plain; }
  if (step == -1) return (int64_t)view.size();   // the number of steps of THIS index space (launch plan + 1 where the front is one launch)
  if (step < 0 || step >= (int32_t)view.size()) return fail(nullptr, YFV2_ERR_ARG, "yfv2_debug_plan_image: step out of range");
  const TowerStep* tw = std::get_if<TowerStep>(&view[step].kind);
  const int n_jobs = tw && tw->halves.size() > 1 ? (int)tw->halves.size() : 0;   // (a launch of one half has no jobs)
  if (job >= n_jobs) return fail(nullptr, YFV2_ERR_ARG, "yfv2_debug_plan_image: job out of range");
  const std::string& st_name = job >= 0 ? tw->halves[job].name : view[step].name;
  const size_t img = job >= 0 ? tw->halves[job].img : step_image(view[step]);
  if (name && name_cap > 0) std::snprintf(name, (size_t)name_cap, "%s", st_name.c_str());
  const int64_t avail = (int64_t)d.wp.blob.size() - (int64_t)img;
  const int64_t cnt = avail < cap ? avail : cap;
  if (cnt > 0) std::memcpy(dst, &d.wp.blob[img], sizeof(float) * (size_t)cnt);
  return cnt;
}

// Host-only test hook: the channel order in which the plan stores stage 3's output (C2).  label[k] = logical channel at
// physical position k; returns 1 if the plan permutes (chain kernel), 0 if C2 is plain NHWC, or a negative error code.
int yfv2_debug_plan_c2_label(const yfv2_config* cfg, const yfv2_tensor_desc* tensors, int32_t n, int32_t* label) {
  if (!cfg || !tensors || n <= 0 || !label) return fail(nullptr, YFV2_ERR_ARG, "yfv2_debug_plan_c2_label: bad argument");
  DryRun d;
  if (int rc = d.build(cfg, nullptr, tensors, n)) return rc;
  for (int k = 0; k < 96; ++k) label[k] = d.ctx.plan.c2_permuted ? d.ctx.plan.c2_label[k] : k;
  return d.ctx.plan.c2_permuted ? 1 : 0;
}

void yfv2_destroy(yfv2_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  h->ws.for_each(h->cfg, h->rows, [](Buf& b, size_t) { free_buf(&b); });
  if (h->d_classes) (void)hipFree(h->d_classes);
  if (h->d_frames) (void)hipFree(h->d_frames);
  if (h->d_frames_u8) (void)hipFree(h->d_frames_u8);
  if (h->d_tile_ws) (void)hipFree(h->d_tile_ws);
  if (h->d_tile_out) (void)hipFree(h->d_tile_out);
  if (h->h_nonfinite) (void)hipHostFree(h->h_nonfinite);
  if (h->d_probe) (void)hipFree(h->d_probe);
  if (h->d_loss_ws) (void)hipFree(h->d_loss_ws);
  if (h->d_km_ws) (void)hipFree(h->d_km_ws);
  if (h->d_ap_ws) (void)hipFree(h->d_ap_ws);
  if (h->h_km_word) (void)hipHostFree(h->h_km_word);
  if (h->train) { yfv2_train_release(h->train); h->train = nullptr; }
  if (h->d_params) (void)hipFree(h->d_params);
  for (yfv2_ctx* lane : h->lanes) yfv2_destroy(lane);
  for (hipStream_t st : h->lane_stream) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  for (hipEvent_t ev : h->lane_join) (void)hipEventDestroy(ev);
  if (h->lane_fork) (void)hipEventDestroy(h->lane_fork);
  delete h;
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

int yfv2_forward(yfv2_handle h, const float* x, int32_t B, float* const out6[6], void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (!x || !out6) return fail(h, YFV2_ERR_ARG, "yfv2_forward: null pointer");
  for (int i = 0; i < 6; ++i)
    if (!out6[i]) return fail(h, YFV2_ERR_ARG, "yfv2_forward: null output tensor");
  DeviceGuard guard(h->device);
  if (use_lanes(h, B))
    return run_lanes(h, B, static_cast<hipStream_t>(stream), [&](yfv2_ctx* lane, int off, int cnt, hipStream_t st) {
      float* o6[6];
      for (int i = 0; i < 6; ++i) o6[i] = out6[i] + (size_t)off * logit_elems(h, i);
      return yfv2_forward(lane, x + (size_t)off * 3 * h->cfg.height * h->cfg.width, cnt, o6, st);
    });
  h->last_split.clear();
  return run_plan(h, x, false, B, out6, static_cast<hipStream_t>(stream), nullptr);
}

int yfv2_forward_u8(yfv2_handle h, const uint8_t* x, int32_t B, float* const out6[6], void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (!x || !out6) return fail(h, YFV2_ERR_ARG, "yfv2_forward_u8: null pointer");
  for (int i = 0; i < 6; ++i)
    if (!out6[i]) return fail(h, YFV2_ERR_ARG, "yfv2_forward_u8: null output tensor");
  DeviceGuard guard(h->device);
  if (use_lanes(h, B))
    return run_lanes(h, B, static_cast<hipStream_t>(stream), [&](yfv2_ctx* lane, int off, int cnt, hipStream_t st) {
      float* o6[6];
      for (int i = 0; i < 6; ++i) o6[i] = out6[i] + (size_t)off * logit_elems(h, i);
      return yfv2_forward_u8(lane, x + (size_t)off * 3 * h->cfg.height * h->cfg.width, cnt, o6, st);
    });
  h->last_split.clear();
  return run_plan(h, x, true, B, out6, static_cast<hipStream_t>(stream), nullptr);
}

static DecodeArgs decode_args(yfv2_handle h, const float* const out6[6], int32_t B) {
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
  NmsArgs a{};
  a.boxes = boxes; a.compact = compact; a.dets = dets; a.idx = idx; a.count = count;
  a.classes = nullptr; a.n_classes = 0;
  if (n_classes > 0) {  // classes is a HOST array (python list in the reference, utils.py:271-272)
    HIP_TRY(h, hipMemcpyAsync(h->d_classes, classes, sizeof(int32_t) * n_classes, hipMemcpyHostToDevice, s));
    a.classes = h->d_classes; a.n_classes = n_classes;
  }
  a.B = B; a.rows = h->rows; a.nc = h->cfg.classes;
  a.conf_thres = conf_thres; a.iou_thres = iou_thres;
  yfv2_launch_nms(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_detect(yfv2_handle h, const float* x, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx,
                int32_t* count, void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (use_lanes(h, B)) {
    if (!x || !dets || !idx || !count) return fail(h, YFV2_ERR_ARG, "yfv2_detect: null pointer");
    DeviceGuard guard(h->device);
    return run_lanes(h, B, static_cast<hipStream_t>(stream), [&](yfv2_ctx* lane, int off, int cnt, hipStream_t st) {
      return yfv2_detect(lane, x + (size_t)off * 3 * h->cfg.height * h->cfg.width, cnt, conf_thres, iou_thres, dets + (size_t)off * YFV2_MAX_DET * 6,
                         idx + (size_t)off * YFV2_MAX_DET, count + off, st);
    });
  }
  float* out6[6];
  for (int i = 0; i < 6; ++i) out6[i] = h->ws.logits[i].p;
  rc = yfv2_forward(h, x, B, out6, stream);
  if (rc) return rc;
  return post_impl(h, out6, B, conf_thres, iou_thres, dets, idx, count, stream);
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
  const DecodeArgs d = decode_args(h, out6, B);
  NmsArgs a{};
  a.boxes = nullptr; a.compact = 1; a.dets = dets; a.idx = idx; a.count = count;
  a.classes = nullptr; a.n_classes = 0;
  a.B = B; a.rows = h->rows; a.nc = h->cfg.classes;
  a.conf_thres = conf_thres; a.iou_thres = iou_thres;
  a.trace = h->trace_step == -2 ? h->d_trace : nullptr;   // YFV2_TRACE=1 YFV2_TRACE_STEP=-2: stamps of the post launch (tools/trace_post.py)
  yfv2_launch_decode_nms(d, a, static_cast<hipStream_t>(stream));
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_detect_u8(yfv2_handle h, const uint8_t* x, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx,
                   int32_t* count, void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (use_lanes(h, B)) {
    if (!x || !dets || !idx || !count) return fail(h, YFV2_ERR_ARG, "yfv2_detect_u8: null pointer");
    DeviceGuard guard(h->device);
    return run_lanes(h, B, static_cast<hipStream_t>(stream), [&](yfv2_ctx* lane, int off, int cnt, hipStream_t st) {
      return yfv2_detect_u8(lane, x + (size_t)off * 3 * h->cfg.height * h->cfg.width, cnt, conf_thres, iou_thres, dets + (size_t)off * YFV2_MAX_DET * 6,
                            idx + (size_t)off * YFV2_MAX_DET, count + off, st);
    });
  }
  float* out6[6];
  for (int i = 0; i < 6; ++i) out6[i] = h->ws.logits[i].p;
  rc = yfv2_forward_u8(h, x, B, out6, stream);
  if (rc) return rc;
  return post_impl(h, out6, B, conf_thres, iou_thres, dets, idx, count, stream);
}

// enqueue only: the overflow flag is sticky in the handle until yfv2_batch_statistics_overflow reads it
int yfv2_batch_statistics_async(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets, int32_t T,
                                float iou_threshold, int32_t* tp, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (B < 1) return fail(h, YFV2_ERR_BATCH, "yfv2_batch_statistics: B < 1");   // no workspace involved: B is not bound by max_batch
  if (!dets || !count || !tp || T < 0 || (T > 0 && !targets)) return fail(h, YFV2_ERR_ARG, "yfv2_batch_statistics: bad argument");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  StatsArgs a{};
  a.dets = dets; a.count = count; a.targets = targets; a.tp = tp; a.overflow = h->d_stats_flag;
  a.B = B; a.T = T; a.iou_thres = iou_threshold;
  yfv2_launch_stats(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

// the same matching at K thresholds in one launch: bit k of tpmask = tp at thresholds[k]; the same sticky overflow word
int yfv2_batch_statistics_multi_async(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets, int32_t T,
                                      const float* thresholds, int32_t K, uint32_t* tpmask, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (B < 1) return fail(h, YFV2_ERR_BATCH, "yfv2_batch_statistics_multi: B < 1");
  if (K < 1 || K > 32) return fail(h, YFV2_ERR_ARG, "yfv2_batch_statistics_multi: K must be in 1..32");
  if (!dets || !count || !thresholds || !tpmask || T < 0 || (T > 0 && !targets)) return fail(h, YFV2_ERR_ARG, "yfv2_batch_statistics_multi: bad argument");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  StatsMultiArgs a{};
  a.dets = dets; a.count = count; a.targets = targets; a.tpmask = tpmask; a.overflow = h->d_stats_flag;
  a.B = B; a.T = T; a.K = K;
  for (int k = 0; k < K; ++k) a.thr[k] = thresholds[k];      // copied here: the caller's array may go once this returns
  yfv2_launch_stats_multi(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_batch_statistics_overflow(yfv2_handle h, int32_t* overflowed, void* stream) {
  if (!h || !overflowed) return fail(h, YFV2_ERR_ARG, "yfv2_batch_statistics_overflow: null pointer");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t over = 0;
  HIP_TRY(h, hipMemcpyAsync(&over, h->d_stats_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemsetAsync(h->d_stats_flag, 0, sizeof(int32_t), s));
  HIP_TRY(h, hipStreamSynchronize(s));
  *overflowed = over;
  return YFV2_OK;
}

// the sticky range-guard word of the fp16x3 plan (yfv2_internal.h Yfv2Watch): waits for `stream`, reports and clears it
int yfv2_nonfinite(yfv2_handle h, int32_t* flag, void* stream) {
  if (!h || !flag) return fail(h, YFV2_ERR_ARG, "yfv2_nonfinite: null argument");
  if (!h->h_nonfinite) return fail(h, YFV2_ERR_STATE, "yfv2_nonfinite: this handle owns no guard word");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(h, hipStreamSynchronize(s));        // a kernel's stores to coherent host memory are visible once it has completed
  volatile int32_t* w = h->h_nonfinite;
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
  if (!h->h_nonfinite) return fail(h, YFV2_ERR_STATE, "yfv2_nonfinite_peek: this handle owns no guard word");
  *flag = *reinterpret_cast<volatile int32_t*>(h->h_nonfinite) ? 1 : 0;
  return YFV2_OK;
}

// effective shader clock, measured by the shader (yfv2_probe.hip): enqueue on `stream` ...
int yfv2_clock_probe_begin(yfv2_handle h, int32_t workgroups, float milliseconds, int32_t busy, void* stream) {
  if (!h || workgroups < 1 || workgroups > 4096 || !(milliseconds > 0.f) || milliseconds > 10000.f)
    return fail(h, YFV2_ERR_ARG, "yfv2_clock_probe_begin: bad argument");
  DeviceGuard guard(h->device);
  if (!h->d_probe) HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_probe), 4096 * 4 * sizeof(unsigned long long)));
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) khz = 100000;
  ClockProbeArgs a{};
  a.out = h->d_probe; a.busy = busy ? 1 : 0;
  a.ref_ticks = (unsigned long long)((double)milliseconds * (double)khz);
  h->probe_wgs = workgroups;
  if (!yfv2_launch_clock_probe(a, workgroups, static_cast<hipStream_t>(stream))) return fail(h, YFV2_ERR_DEVICE, "clock probe launch failed");
  return YFV2_OK;
}

// ... and read it back (waits for `stream`): out[0..2] = min / mean / max over the probe's workgroups of
// (shader cycles / reference ticks) x reference clock, in MHz; out[3] = the reference clock in MHz; out[4] = mean measured
// interval in milliseconds; out[5] = number of distinct XCDs the workgroups ran on
int yfv2_clock_probe_end(yfv2_handle h, double out[6], void* stream) {
  if (!h || !out) return fail(h, YFV2_ERR_ARG, "yfv2_clock_probe_end: null argument");
  if (!h->d_probe || h->probe_wgs < 1) return fail(h, YFV2_ERR_STATE, "yfv2_clock_probe_end without yfv2_clock_probe_begin");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<unsigned long long> st((size_t)h->probe_wgs * 4);
  HIP_TRY(h, hipMemcpyAsync(st.data(), h->d_probe, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) khz = 100000;
  const double ref_mhz = khz * 1e-3;
  double mn = 1e30, mx = 0., sum = 0., ms = 0.;
  unsigned xcds = 0;
  for (int i = 0; i < h->probe_wgs; ++i) {
    const double cyc = (double)st[4 * i], ref = (double)st[4 * i + 1];
    if (!(ref > 0.)) return fail(h, YFV2_ERR_DEVICE, "clock probe: a workgroup reported no reference ticks");
    const double mhz = cyc / ref * ref_mhz;
    mn = std::min(mn, mhz); mx = std::max(mx, mhz); sum += mhz; ms += ref / ref_mhz * 1e-3;
    xcds |= 1u << (unsigned)(st[4 * i + 2] & 15);
  }
  out[0] = mn; out[1] = sum / h->probe_wgs; out[2] = mx; out[3] = ref_mhz; out[4] = ms / h->probe_wgs; out[5] = (double)__builtin_popcount(xcds);
  h->probe_wgs = 0;
  return YFV2_OK;
}

int yfv2_batch_statistics(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets, int32_t T,
                          float iou_threshold, int32_t* tp, void* stream) {
  int rc = yfv2_batch_statistics_async(h, dets, count, B, targets, T, iou_threshold, tp, stream);
  if (rc) return rc;
  int32_t over = 0;
  rc = yfv2_batch_statistics_overflow(h, &over, stream);
  if (rc) return rc;
  if (over) return fail(h, YFV2_ERR_ARG, "yfv2_batch_statistics: an image has more than 1024 targets");
  return YFV2_OK;
}

int yfv2_batch_statistics_multi(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets, int32_t T,
                                const float* thresholds, int32_t K, uint32_t* tpmask, void* stream) {
  int rc = yfv2_batch_statistics_multi_async(h, dets, count, B, targets, T, thresholds, K, tpmask, stream);
  if (rc) return rc;
  int32_t over = 0;
  rc = yfv2_batch_statistics_overflow(h, &over, stream);
  if (rc) return rc;
  if (over) return fail(h, YFV2_ERR_ARG, "yfv2_batch_statistics_multi: an image has more than 1024 targets");
  return YFV2_OK;
}

int yfv2_loss(yfv2_handle h, const float* const out6[6], int32_t B, const float* targets, int32_t T, float* losses,
              float* const grad6[6], void* stream) {
  int rc = check_call(h, B, false);
  if (rc) return rc;
  if (!out6 || !losses || T < 0 || (T > 0 && !targets)) return fail(h, YFV2_ERR_ARG, "yfv2_loss: bad argument");
  for (int i = 0; i < 6; ++i)
    if (!out6[i] || (grad6 && !grad6[i])) return fail(h, YFV2_ERR_ARG, "yfv2_loss: null logit / gradient tensor");
  if (T > (1 << 20)) return fail(h, YFV2_ERR_ARG, "yfv2_loss: more than 2^20 labels in one batch");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t A = (size_t)h->cfg.anchor_num;
  const size_t cells0 = (size_t)B * A * h->fh[0] * h->fw[0], cells1 = (size_t)B * A * h->fh[1] * h->fw[1];
  // layout: [sums 6 doubles][nb 2 ints + pad][tobj0][tobj1][pad][matches]
  const size_t off_nb = 6 * sizeof(double), off_t0 = off_nb + 16, off_t1 = off_t0 + cells0;
  const size_t zero_bytes = (off_t1 + cells1 + 15) & ~(size_t)15;
  const size_t need = zero_bytes + sizeof(LossMatch) * (size_t)(2 * 5 * 3) * (size_t)(T > 0 ? T : 1);
  if (need > h->loss_ws_bytes) {
    HIP_TRY(h, hipDeviceSynchronize());               // an earlier yfv2_loss may still be using the old block
    if (h->d_loss_ws) { (void)hipFree(h->d_loss_ws); h->d_loss_ws = nullptr; h->loss_ws_bytes = 0; }
    const size_t cap = need + need / 2;
    HIP_TRY(h, hipMalloc(&h->d_loss_ws, cap));
    h->loss_ws_bytes = cap;
  }
  char* ws = static_cast<char*>(h->d_loss_ws);
  HIP_TRY(h, hipMemsetAsync(ws, 0, zero_bytes, s));
  LossArgs a{};
  for (int l = 0; l < 2; ++l) {
    a.reg[l] = out6[3 * l]; a.obj[l] = out6[3 * l + 1]; a.cls[l] = out6[3 * l + 2];
    a.grad_reg[l] = grad6 ? grad6[3 * l] : nullptr; a.grad_obj[l] = grad6 ? grad6[3 * l + 1] : nullptr; a.grad_cls[l] = grad6 ? grad6[3 * l + 2] : nullptr;
    a.fh[l] = h->fh[l]; a.fw[l] = h->fw[l];
    a.stride[l] = (double)h->cfg.width / (double)h->fw[l];        // utils/loss.py:82
    if (grad6) {                                                   // reg / cls gradients are accumulated with atomics: start from zero
      HIP_TRY(h, hipMemsetAsync(grad6[3 * l], 0, sizeof(float) * (size_t)B * 4 * A * h->fh[l] * h->fw[l], s));
      HIP_TRY(h, hipMemsetAsync(grad6[3 * l + 2], 0, sizeof(float) * (size_t)B * h->cfg.classes * h->fh[l] * h->fw[l], s));
    }
  }
  for (int i = 0; i < 12; ++i) a.anchors[i] = h->cfg.anchors[i];
  a.targets = targets;
  a.sums = reinterpret_cast<double*>(ws);
  a.nb = reinterpret_cast<int*>(ws + off_nb);
  a.tobj[0] = reinterpret_cast<unsigned char*>(ws + off_t0);
  a.tobj[1] = reinterpret_cast<unsigned char*>(ws + off_t1);
  a.matches = reinterpret_cast<LossMatch*>(ws + zero_bytes);
  a.losses = losses;
  a.B = B; a.T = T; a.classes = h->cfg.classes;
  yfv2_launch_loss(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

// genanchors.py:67-102 on the device (yfv2_anchors.hip).  Passes are enqueued in groups of km_group; a launch that finds the
// device `done` word set returns at once, so the passes of a group that follow the terminating one change nothing and the
// group size is invisible in the results.
int yfv2_anchor_kmeans(yfv2_handle h, const double* wh, int64_t N, double* centroids, int32_t k, int32_t max_iter, int32_t* assign,
                       double* avg_iou, yfv2_kmeans_info* info, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!wh || !centroids || !avg_iou || !info) return fail(h, YFV2_ERR_ARG, "yfv2_anchor_kmeans: null pointer (wh, centroids, avg_iou and info are required)");
  if (N < 1) return fail(h, YFV2_ERR_ARG, "yfv2_anchor_kmeans: N must be at least 1");
  if (N > (int64_t)0x7fffffff * YFV2_KM_CH) return fail(h, YFV2_ERR_ARG, "yfv2_anchor_kmeans: N beyond 2^31 chunks of 1024 points");
  if (k < 1 || k > YFV2_KM_MAXK) return fail(h, YFV2_ERR_ARG, "yfv2_anchor_kmeans: k must be in 1..32");
  if (max_iter < 1) return fail(h, YFV2_ERR_ARG, "yfv2_anchor_kmeans: max_iter must be at least 1");
  if ((reinterpret_cast<uintptr_t>(wh) & 7) != 0 || (reinterpret_cast<uintptr_t>(centroids) & 7) != 0)
    return fail(h, YFV2_ERR_ARG, "yfv2_anchor_kmeans: wh and centroids must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(avg_iou) & 7) != 0 || (reinterpret_cast<uintptr_t>(assign) & 3) != 0)
    return fail(h, YFV2_ERR_ARG, "yfv2_anchor_kmeans: avg_iou must be 8-byte and assign 4-byte aligned");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!h->h_km_word) {
    void* hp = nullptr; void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
      if (hp) (void)hipHostFree(hp);
      return fail(h, YFV2_ERR_DEVICE, "hipHostMalloc(k-means word) failed");
    }
    h->h_km_word = static_cast<int32_t*>(hp);
    h->d_km_word = static_cast<int32_t*>(dp);
  }
  const int64_t nch = (N + YFV2_KM_CH - 1) / YFV2_KM_CH;
  // layout: [done word, 64 bytes][sums (2k + 1) nch doubles][counts k nch ints][flags nch ints][assignments N ints, if the caller has none]
  const size_t off_sum = 64, off_cnt = off_sum + sizeof(double) * (size_t)(2 * k + 1) * (size_t)nch;
  const size_t off_flag = off_cnt + sizeof(int) * (size_t)k * (size_t)nch, off_asg = off_flag + sizeof(int) * (size_t)nch;
  const size_t need = off_asg + (assign ? 0 : sizeof(int32_t) * (size_t)N);
  if (need > h->km_ws_bytes) {
    HIP_TRY(h, hipDeviceSynchronize());               // an earlier call's launches may still be using the old block
    if (h->d_km_ws) { (void)hipFree(h->d_km_ws); h->d_km_ws = nullptr; h->km_ws_bytes = 0; }
    const size_t cap = need + need / 2;
    HIP_TRY(h, hipMalloc(&h->d_km_ws, cap));
    h->km_ws_bytes = cap;
  }
  char* ws = static_cast<char*>(h->d_km_ws);
  KmArgs a{};
  a.wh = wh; a.N = N; a.centroids = centroids; a.k = k; a.nchunks = nch;
  a.assign = assign ? assign : reinterpret_cast<int32_t*>(ws + off_asg);
  a.avg_iou = avg_iou;
  a.done = reinterpret_cast<int*>(ws);
  a.part_sum = reinterpret_cast<double*>(ws + off_sum);
  a.part_cnt = reinterpret_cast<int*>(ws + off_cnt);
  a.part_flag = reinterpret_cast<int*>(ws + off_flag);
  a.host_word = h->d_km_word;
  volatile int32_t* hw = h->h_km_word;   // every earlier call waited for its stream before it returned: nothing is writing the word now
  for (int i = 0; i < 5; ++i) hw[i] = 0;
  HIP_TRY(h, hipMemsetAsync(a.done, 0, 64, s));
  const int group = h->km_group < 1 ? 1 : h->km_group;
  int pass = 0;
  while (pass < max_iter) {
    for (int g = 0; g < group && pass < max_iter; ++g, ++pass) yfv2_launch_km_pass(a, pass, pass == max_iter - 1 ? 1 : 0, s);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));              // a kernel's stores to coherent host memory are visible once it has completed
    if (hw[0]) break;
  }
  if (!hw[0]) return fail(h, YFV2_ERR_DEVICE, "yfv2_anchor_kmeans: the last pass did not publish its verdict");
  yfv2_kmeans_info out{};
  out.iterations = hw[1]; out.converged = hw[2]; out.empty_cluster = hw[3]; out.bad_input = hw[4];
  // (a caller built against a shorter struct gets the fields it has)
  const size_t n = info->struct_size > 0 && (size_t)info->struct_size < sizeof(yfv2_kmeans_info) ? (size_t)info->struct_size : sizeof(yfv2_kmeans_info);
  out.struct_size = (int32_t)n;
  std::memcpy(info, &out, n);
  return YFV2_OK;
}

// Test hook: passes enqueued between two host looks (1..64; the default is 8).  Exists so that a test can show that the group
// size changes no output bit.
int yfv2_debug_kmeans_group(yfv2_handle h, int32_t group) {
  if (!h || group < 1 || group > 64) return fail(h, YFV2_ERR_ARG, "yfv2_debug_kmeans_group: group must be in 1..64");
  h->km_group = group;
  return YFV2_OK;
}

// both AP entry points after their argument checks: grow the workspace, enqueue everything, copy the max(K, 1) result blocks back, wait
static int ap_run(yfv2_handle h, ApArgs& a, ApHead* heads, hipStream_t s) {
  const size_t need = yfv2_ap_ws_bytes(a.N, a.K);
  if (need > h->ap_ws_bytes) {
    HIP_TRY(h, hipDeviceSynchronize());               // (every earlier call waited for its stream; another stream's work may not have)
    if (h->d_ap_ws) { (void)hipFree(h->d_ap_ws); h->d_ap_ws = nullptr; h->ap_ws_bytes = 0; }
    const size_t cap = need + need / 2;
    HIP_TRY(h, hipMalloc(&h->d_ap_ws, cap));
    h->ap_ws_bytes = cap;
  }
  yfv2_ap_carve(a, static_cast<char*>(h->d_ap_ws));
  yfv2_launch_ap(a, s);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(heads, a.head, (size_t)(a.K > 1 ? a.K : 1) * sizeof(ApHead), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return YFV2_OK;
}

// utils/utils.py:110-192 on the device (yfv2_ap.hip): rank, per-class curve, one fixed summation tree; the means on the host.
int yfv2_ap_per_class(yfv2_handle h, const int32_t* tp, const float* conf, const float* pred_cls, int64_t N, const float* target_cls,
                      int64_t T, yfv2_ap_result* out, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!out) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class: out is required");
  if (N < 0 || T < 0) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class: N and T must not be negative");
  if (N > 0x7fffffffLL || T > 0x7fffffffLL) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class: N and T are limited to 2^31 - 1 (the payload holds tp in bit 31)");
  if (N > 0 && (!tp || !conf || !pred_cls)) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class: null pointer (tp, conf and pred_cls are required when N > 0)");
  if (T > 0 && !target_cls) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class: null pointer (target_cls is required when T > 0)");
  if (((reinterpret_cast<uintptr_t>(tp) | reinterpret_cast<uintptr_t>(conf) | reinterpret_cast<uintptr_t>(pred_cls) | reinterpret_cast<uintptr_t>(target_cls)) & 3) != 0)
    return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class: the arrays must be 4-byte aligned");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ApArgs a{};
  a.tp = tp; a.conf = conf; a.pred_cls = pred_cls; a.N = N; a.target_cls = target_cls; a.T = T;
  ApHead head;
  const int rc = ap_run(h, a, &head, s);
  if (rc) return rc;
  yfv2_ap_result res{};
  yfv2_ap_finish(head, &res);
  // (a caller built against a shorter struct gets the fields it has)
  const size_t n = out->struct_size > 0 && (size_t)out->struct_size < sizeof(yfv2_ap_result) ? (size_t)out->struct_size : sizeof(yfv2_ap_result);
  res.struct_size = (int32_t)n;
  std::memcpy(out, &res, n);
  return YFV2_OK;
}

// ... at K thresholds: one rank, a (class, threshold) grid of walks (yfv2_ap.hip); out[k] is what yfv2_ap_per_class returns for tp = bit k
int yfv2_ap_per_class_multi(yfv2_handle h, const uint32_t* tpmask, const float* conf, const float* pred_cls, int64_t N,
                            const float* target_cls, int64_t T, int32_t K, yfv2_ap_result* out, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!out) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class_multi: out is required");
  if (K < 1 || K > 32) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class_multi: K must be in 1..32");
  if (N < 0 || T < 0) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class_multi: N and T must not be negative");
  if (N > 0x7fffffffLL || T > 0x7fffffffLL) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class_multi: N and T are limited to 2^31 - 1");
  if (N > 0 && (!tpmask || !conf || !pred_cls)) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class_multi: null pointer (tpmask, conf and pred_cls are required when N > 0)");
  if (T > 0 && !target_cls) return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class_multi: null pointer (target_cls is required when T > 0)");
  if (((reinterpret_cast<uintptr_t>(tpmask) | reinterpret_cast<uintptr_t>(conf) | reinterpret_cast<uintptr_t>(pred_cls) | reinterpret_cast<uintptr_t>(target_cls)) & 3) != 0)
    return fail(h, YFV2_ERR_ARG, "yfv2_ap_per_class_multi: the arrays must be 4-byte aligned");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ApArgs a{};
  a.tpmask = tpmask; a.K = K; a.conf = conf; a.pred_cls = pred_cls; a.N = N; a.target_cls = target_cls; a.T = T;
  std::vector<ApHead> heads((size_t)K);
  const int rc = ap_run(h, a, heads.data(), s);
  if (rc) return rc;
  std::vector<yfv2_ap_result> res((size_t)K);
  yfv2_ap_finish_multi(heads.data(), K, res.data());
  // the records lie one caller's struct apart (a caller built against a shorter struct gets the fields it has)
  const size_t n = out->struct_size > 0 && (size_t)out->struct_size < sizeof(yfv2_ap_result) ? (size_t)out->struct_size : sizeof(yfv2_ap_result);
  for (int k = 0; k < K; ++k) {
    res[(size_t)k].struct_size = (int32_t)n;
    std::memcpy(reinterpret_cast<char*>(out) + (size_t)k * n, &res[(size_t)k], n);
  }
  return YFV2_OK;
}

int yfv2_resize_u8(yfv2_handle h, const uint8_t* src, int32_t B, int32_t src_h, int32_t src_w, uint8_t* dst, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!src || !dst || B < 1 || src_h < 1 || src_w < 1) return fail(h, YFV2_ERR_ARG, "yfv2_resize_u8: bad argument");
  if ((reinterpret_cast<uintptr_t>(dst) & 3) != 0) return fail(h, YFV2_ERR_ARG, "yfv2_resize_u8: dst must be 4-byte aligned");
  if (yfv2_resize_lds_bytes(src_w, h->cfg.width) > 160 * 1024 || (long long)B * h->cfg.height > 0x7fffffffll)
    return fail(h, YFV2_ERR_ARG, "yfv2_resize_u8: source rows wider than " + std::to_string((160 * 1024 - 3 * h->cfg.width) / 6 - 2) + " pixels are not supported");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ResizeArgs a{};
  a.src = src; a.dst = dst; a.B = B; a.SH = src_h; a.SW = src_w; a.H = h->cfg.height; a.W = h->cfg.width;
  a.scale_x = 1.0 / ((double)a.W / (double)src_w);      // cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale
  a.scale_y = 1.0 / ((double)a.H / (double)src_h);
  yfv2_launch_resize(a, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

// Ragged batches (yfv2_resize_frames_u8 / yfv2_detect_frames_u8): every frame is checked here, before anything is enqueued,
// and expanded by its scales into t; *max_w = the widest frame (it sizes the resize launch's LDS).  The table is B entries of
// the handle's max_batch, so B is bound by max_batch on both entry points.
static int check_frames(yfv2_handle h, const char* what, const yfv2_frame* frames, int32_t B, std::vector<ResizeFrame>& t, int* max_w) {
  const std::string w_ = what;
  if (!frames) return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  if (B < 1) return fail(h, YFV2_ERR_ARG, w_ + ": B < 1");
  if (B > h->cfg.max_batch)
    return fail(h, YFV2_ERR_BATCH, w_ + ": batch " + std::to_string(B) + " above max_batch=" + std::to_string(h->cfg.max_batch));
  const int H = h->cfg.height, W = h->cfg.width;
  const int limit = (160 * 1024 - 3 * W) / 6 - 2;
  t.assign((size_t)B, ResizeFrame{});
  int mw = 1;
  for (int32_t b = 0; b < B; ++b) {
    const yfv2_frame& f = frames[b];
    const std::string at = w_ + ": frame " + std::to_string(b) + ": ";
    if (f.height < 1 || f.width < 1) return fail(h, YFV2_ERR_ARG, at + "height and width must be >= 1");
    if (!f.data) return fail(h, YFV2_ERR_ARG, at + "null data");
    if (f.row_pitch < 3ll * f.width) return fail(h, YFV2_ERR_ARG, at + "row_pitch " + std::to_string(f.row_pitch) + " < 3 * width");
    if (f.width > limit || yfv2_resize_lds_bytes(f.width, W) > 160 * 1024)
      return fail(h, YFV2_ERR_ARG, at + "frames wider than " + std::to_string(limit) + " pixels are not supported");
    if (f.row_pitch > (1ll << 40) || (long long)(f.height - 1) * f.row_pitch > (1ll << 52))
      return fail(h, YFV2_ERR_ARG, at + "row_pitch out of range");
    ResizeFrame& r = t[(size_t)b];
    r.data = f.data; r.pitch = f.row_pitch; r.h = f.height; r.w = f.width;
    r.scale_x = 1.0 / ((double)W / (double)f.width);      // exactly yfv2_resize_u8's scales
    r.scale_y = 1.0 / ((double)H / (double)f.height);
    r.box_x = (double)f.width / (double)W;                // test.py:58  scale_w = w / cfg["width"]
    r.box_y = (double)f.height / (double)H;
    mw = std::max(mw, (int)f.width);
  }
  if ((long long)B * H > 0x7fffffffll) return fail(h, YFV2_ERR_ARG, w_ + ": batch too large");
  *max_w = mw;
  return YFV2_OK;
}

int yfv2_resize_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, uint8_t* dst, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!dst) return fail(h, YFV2_ERR_ARG, "yfv2_resize_frames_u8: null pointer");
  if ((reinterpret_cast<uintptr_t>(dst) & 3) != 0) return fail(h, YFV2_ERR_ARG, "yfv2_resize_frames_u8: dst must be 4-byte aligned");
  std::vector<ResizeFrame> t;
  int max_w = 0;
  int rc = check_frames(h, "yfv2_resize_frames_u8", frames, B, t, &max_w);
  if (rc) return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(h, hipMemcpyAsync(h->d_frames, t.data(), sizeof(ResizeFrame) * (size_t)B, hipMemcpyHostToDevice, s));
  yfv2_launch_resize_frames(h->d_frames, B, max_w, dst, h->cfg.height, h->cfg.width, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

int yfv2_detect_frames_u8(yfv2_handle h, const yfv2_frame* frames, int32_t B, float conf_thres, double iou_thres, float* dets,
                          int32_t* idx, int32_t* count, void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (!dets || !idx || !count) return fail(h, YFV2_ERR_ARG, "yfv2_detect_frames_u8: null pointer");
  std::vector<ResizeFrame> t;
  int max_w = 0;
  rc = check_frames(h, "yfv2_detect_frames_u8", frames, B, t, &max_w);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(h->device);
  if (!h->d_frames_u8) {   // the resized batch, allocated on first use: handles that never see frames keep their footprint
    HIP_TRY(h, hipDeviceSynchronize());   // like the loss workspace: the allocation waits for the device once
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_frames_u8), (size_t)h->cfg.height * h->cfg.width * 3 * (size_t)h->cfg.max_batch));
  }
  HIP_TRY(h, hipMemcpyAsync(h->d_frames, t.data(), sizeof(ResizeFrame) * (size_t)B, hipMemcpyHostToDevice, s));
  yfv2_launch_resize_frames(h->d_frames, B, max_w, h->d_frames_u8, h->cfg.height, h->cfg.width, s);
  HIP_TRY(h, hipGetLastError());
  rc = yfv2_detect_u8(h, h->d_frames_u8, B, conf_thres, iou_thres, dets, idx, count, stream);
  if (rc) return rc;
  yfv2_launch_frame_boxes(dets, count, h->d_frames, B, s);
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
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

static int ensure_tile_ws(yfv2_handle h, int T, int F) {
  if (h->d_tile_ws && T <= h->tile_cap_t && F <= h->tile_cap_f) return YFV2_OK;
  const int ct = std::max(T, h->tile_cap_t), cf = std::max(F, h->tile_cap_f);
  HIP_TRY(h, hipDeviceSynchronize());            // like the resize buffer: an allocation waits for the device once
  if (h->d_tile_ws) { (void)hipFree(h->d_tile_ws); h->d_tile_ws = nullptr; h->tile_cap_t = h->tile_cap_f = 0; }
  const size_t bytes = (size_t)ct * YFV2_MAX_DET * 32 + sizeof(int32_t) * ((size_t)4 * ct + (size_t)2 * cf);
  HIP_TRY(h, hipMalloc(&h->d_tile_ws, bytes));
  h->tile_cap_t = ct; h->tile_cap_f = cf;
  return YFV2_OK;
}

// uploads the table and enqueues the two launches; everything was checked
static int enqueue_merge(yfv2_handle h, const float* tile_dets, const int32_t* tile_count, const std::vector<int32_t>& table, int32_t T, int32_t F,
                         double merge_thres, int32_t merge_metric, int32_t max_out, float* dets, int32_t* src, int32_t* count, hipStream_t s) {
  char* base = static_cast<char*>(h->d_tile_ws);
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

int yfv2_detect_tiled_u8(yfv2_handle h, const yfv2_frame* frames, int32_t F, const yfv2_tile* tiles, int32_t T, float conf_thres, double iou_thres,
                         double merge_thres, int32_t merge_metric, int32_t max_out, float* dets, int32_t* src, int32_t* count, void* stream) {
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!frames || !tiles || !dets || !count) return fail(h, YFV2_ERR_ARG, "yfv2_detect_tiled_u8: null pointer");
  if (T > h->cfg.max_batch)
    return fail(h, YFV2_ERR_BATCH, "yfv2_detect_tiled_u8: " + std::to_string(T) + " tiles above max_batch=" + std::to_string(h->cfg.max_batch));
  std::vector<int32_t> table;
  if (int rc = check_merge(h, "yfv2_detect_tiled_u8", tiles, T, F, merge_thres, merge_metric, max_out, table)) return rc;
  for (int32_t f = 0; f < F; ++f) {
    const yfv2_frame& fr = frames[f];
    const std::string at = "yfv2_detect_tiled_u8: frame " + std::to_string(f) + ": ";
    if (fr.height < 1 || fr.width < 1) return fail(h, YFV2_ERR_ARG, at + "height and width must be >= 1");
    if (!fr.data) return fail(h, YFV2_ERR_ARG, at + "null data");
    if (fr.row_pitch < 3ll * fr.width) return fail(h, YFV2_ERR_ARG, at + "row_pitch " + std::to_string(fr.row_pitch) + " < 3 * width");
  }
  std::vector<yfv2_frame> crops((size_t)T);
  for (int32_t k = 0; k < T; ++k) {
    const yfv2_tile& t = tiles[k];
    const yfv2_frame& fr = frames[t.frame];
    if (t.width < 1 || t.height < 1 || t.x0 < 0 || t.y0 < 0 || (int64_t)t.x0 + t.width > fr.width || (int64_t)t.y0 + t.height > fr.height)
      return fail(h, YFV2_ERR_ARG, "yfv2_detect_tiled_u8: tile " + std::to_string(k) + ": [" + std::to_string(t.x0) + ", " + std::to_string((int64_t)t.x0 + t.width) +
                                       ") x [" + std::to_string(t.y0) + ", " + std::to_string((int64_t)t.y0 + t.height) + ") is not a rectangle of at least one pixel inside its " +
                                       std::to_string(fr.width) + " x " + std::to_string(fr.height) + " frame");
    crops[(size_t)k] = yfv2_frame{fr.data + (int64_t)t.y0 * fr.row_pitch + 3ll * t.x0, t.height, t.width, fr.row_pitch};
  }
  // everything yfv2_detect_frames_u8 checks, per crop, before the workspaces are touched (it checks again: host work only)
  if (int rc = check_call(h, T, true)) return rc;
  {
    std::vector<ResizeFrame> t;
    int max_w = 0;
    if (int rc = check_frames(h, "yfv2_detect_tiled_u8", crops.data(), T, t, &max_w)) return rc;
  }
  DeviceGuard guard(h->device);
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->d_tile_out) {
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_tile_out), sizeof(float) * mb * YFV2_MAX_DET * 6 + sizeof(int32_t) * (mb * YFV2_MAX_DET + mb)));
  }
  if (int rc = ensure_tile_ws(h, h->cfg.max_batch, F)) return rc;    // for max_batch tiles: no later call on this handle grows it for its tiles
  float* t_dets = h->d_tile_out;
  int32_t* t_idx = reinterpret_cast<int32_t*>(t_dets + mb * YFV2_MAX_DET * 6);
  int32_t* t_count = t_idx + mb * YFV2_MAX_DET;
  if (int rc = yfv2_detect_frames_u8(h, crops.data(), T, conf_thres, iou_thres, t_dets, t_idx, t_count, stream)) return rc;
  return enqueue_merge(h, t_dets, t_count, table, T, F, merge_thres, merge_metric, max_out, dets, src, count, static_cast<hipStream_t>(stream));
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

int yfv2_profile_forward(yfv2_handle h, const float* x, int32_t B, float* const out6[6], int32_t iters, float* ms, void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (!x || !out6 || !ms || iters < 1) return fail(h, YFV2_ERR_ARG, "yfv2_profile_forward: bad argument");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // One untimed pass, then `iters` timed passes queued back to back and ONE synchronisation at the end: a pass's first launch
  // follows the previous pass's last one, as in a running loop.  (Synchronising after every pass - the first form - put the stem
  // behind an idle device each time: 127 us by these events against 114 us in a rocprofv3 trace of the bench loop on the same box.)
  const size_t n = h->plan.steps.size();
  // events and the post launch's output buffers are released on EVERY path out of this function (HIP_TRY returns early)
  struct Scratch {
    std::vector<hipEvent_t> ev;
    float* dets = nullptr; int32_t* idx = nullptr; int32_t* cnt = nullptr;
    ~Scratch() {
      for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
      if (dets) (void)hipFree(dets);
      if (idx) (void)hipFree(idx);
      if (cnt) (void)hipFree(cnt);
    }
  } sc;
  sc.ev.assign(2 * n * (size_t)iters, nullptr);
  for (auto& e : sc.ev) HIP_TRY(h, hipEventCreate(&e));
  std::vector<hipEvent_t>& ev = sc.ev;
  // Between two passes the post launch runs (untimed, on the logits just written, test.py's thresholds 0.3 / 0.4), as it does
  // between two forwards of a detect loop: a pass's first launch then meets the memory system in the state it meets there (behind
  // the last tower launch's 47 MB of logit stores instead, the stem took 121 us by these events against 109 us in the trace).
  const bool with_post = h->postfuse && yfv2_post_fusable(h->cfg.classes, h->rows);
  if (with_post) {
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&sc.dets), (size_t)B * YFV2_MAX_DET * 6 * sizeof(float)));
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&sc.idx), (size_t)B * YFV2_MAX_DET * sizeof(int32_t)));
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&sc.cnt), (size_t)B * sizeof(int32_t)));
  }
  float* const p_dets = sc.dets; int32_t* const p_idx = sc.idx; int32_t* const p_cnt = sc.cnt;
  auto post = [&]() {
    if (!with_post) return;
    const DecodeArgs d = decode_args(h, out6, B);
    NmsArgs a{};
    a.boxes = nullptr; a.compact = 1; a.dets = p_dets; a.idx = p_idx; a.count = p_cnt;
    a.classes = nullptr; a.n_classes = 0;
    a.B = B; a.rows = h->rows; a.nc = h->cfg.classes;
    a.conf_thres = 0.3f; a.iou_thres = 0.4;
    a.trace = nullptr;
    yfv2_launch_decode_nms(d, a, s);
  };
  rc = run_plan(h, x, false, B, out6, s, nullptr);
  post();
  for (int it = 0; it < iters && rc == YFV2_OK; ++it) { rc = run_plan(h, x, false, B, out6, s, ev.data() + 2 * n * (size_t)it); post(); }
  if (rc == YFV2_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(h, YFV2_ERR_DEVICE, "yfv2_profile_forward: synchronize failed");
  if (rc != YFV2_OK) (void)hipStreamSynchronize(s);   // nothing may still be writing the post buffers when Scratch frees them
  std::vector<double> acc(n, 0.0);
  for (int it = 0; it < iters && rc == YFV2_OK; ++it)
    for (size_t i = 0; i < n; ++i) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev[2 * n * (size_t)it + 2 * i], ev[2 * n * (size_t)it + 2 * i + 1]) != hipSuccess) { rc = fail(h, YFV2_ERR_DEVICE, "yfv2_profile_forward: event query failed"); break; }
      acc[i] += t;
    }
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) ms[i] = (float)(acc[i] / iters);
  return YFV2_OK;
}

// Measurement helper: one whole forward (so that every launch's inputs exist), then launch `step` of the plan `iters` times back to
// back on `stream` (every launch reads its inputs and writes its outputs in place again: idempotent).  Enqueue only - the caller
// times it, or reads the device's power sensor while it runs (tools/power_probe.py).
int yfv2_debug_repeat_step(yfv2_handle h, const float* x, int32_t B, float* const out6[6], int32_t step, int32_t iters, void* stream) {
  int rc = check_call(h, B, true);
  if (rc) return rc;
  if (!x || !out6 || iters < 0 || step < 0 || step >= (int32_t)h->plan.steps.size()) return fail(h, YFV2_ERR_ARG, "yfv2_debug_repeat_step: bad argument");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = run_plan(h, x, false, B, out6, s, nullptr);
  for (int it = 0; it < iters && rc == YFV2_OK; ++it) rc = run_plan(h, x, false, B, out6, s, nullptr, step);
  return rc;
}

int64_t yfv2_debug_activation(yfv2_handle h, int32_t which, int32_t B, float* host_dst, int64_t cap) {
  if (h && which == 100 && h->d_trace && host_dst && cap >= 128) {  // debug: cycle stamps as int64 (2 floats each), as many as fit (<= 8192)
    (void)hipDeviceSynchronize();
    const int64_t n64 = cap / 2 < 8192 ? cap / 2 : 8192;
    (void)hipMemcpy(host_dst, h->d_trace, (size_t)n64 * sizeof(long long), hipMemcpyDeviceToHost);
    return n64;
  }
  if (h && which == 101 && h->plan.s2_px && host_dst) {  // debug: both raw stage-2 pair-plane buffers, B images each
    const size_t per = h->plan.dbg[1].per_img, nn = (size_t)B * per;     // -> [buffer][image][..]; on the device an image's two copies are adjacent
    if (cap < (int64_t)(2 * nn)) return YFV2_ERR_ARG;
    (void)hipDeviceSynchronize();
    for (int k = 0; k < 2; ++k)
      (void)hipMemcpy2D(host_dst + (size_t)k * nn, per * sizeof(float), h->ws.s2pp.p + (size_t)k * per, 2 * per * sizeof(float), per * sizeof(float), (size_t)B,
                        hipMemcpyDeviceToHost);
    return (int64_t)(2 * nn);
  }
  if (!h || which < 0 || which > 5 || !h->plan.dbg[which].p || B < 1 || B > h->cfg.max_batch) {
    fail(h, YFV2_ERR_ARG, "yfv2_debug_activation: bad argument");
    return YFV2_ERR_ARG;
  }
  DeviceGuard guard(h->device);
  const int64_t n = (int64_t)h->plan.dbg[which].per_img * B;
  if (!host_dst) return n;
  if (!h->last_split.empty()) {   // the last forward ran on the lanes: every lane holds its slice
    if (cap < n) { fail(h, YFV2_ERR_ARG, "yfv2_debug_activation: destination too small"); return YFV2_ERR_ARG; }
    int off = 0;
    for (size_t i = 0; i < h->last_split.size() && off < B; ++i) {
      const int cnt = std::min(h->last_split[i], B - off);
      const int64_t got = yfv2_debug_activation(h->lanes[i], which, cnt, host_dst + (size_t)off * h->plan.dbg[which].per_img, (int64_t)h->plan.dbg[which].per_img * cnt);
      if (got < 0) return got;
      off += cnt;
    }
    return n;
  }
  if (cap < n) { fail(h, YFV2_ERR_ARG, "yfv2_debug_activation: destination too small"); return YFV2_ERR_ARG; }
  if (which == 0 && h->plan.front_fused) {
    // front_kernel never writes the stem's output: run the stem's own launch on the last forward's input (which the caller must still hold)
    if (!h->last_x || h->last_B < B) { fail(h, YFV2_ERR_STATE, "yfv2_debug_activation(0): no forward of at least this batch has run on the handle"); return YFV2_ERR_STATE; }
    const RunCtx c{h->d_params, h->last_x, h->last_u8, B, nullptr, nullptr, h->sw.bf6, h->d_nonfinite};
    if (hipDeviceSynchronize() != hipSuccess) { fail(h, YFV2_ERR_DEVICE, "yfv2_debug_activation: synchronize failed"); return YFV2_ERR_DEVICE; }
    yfv2_launch_stem(stem_launch_args(std::get<StemStep>(h->plan.stem_aside.kind), c), nullptr);
  }
  if (which == 0 && h->plan.stem_pp) {  // stem output in pair planes [12][PH*PW][2] (stem_px_kernel, YFV2_BF6=0) -> NHWC
    const size_t per = h->plan.dbg[0].per_img, hw = per / 24;
    std::vector<float> tmp((size_t)n);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(tmp.data(), h->plan.dbg[0].p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
      fail(h, YFV2_ERR_DEVICE, "yfv2_debug_activation: copy failed");
      return YFV2_ERR_DEVICE;
    }
    for (int b = 0; b < B; ++b)
      for (int q = 0; q < 12; ++q)
        for (size_t px = 0; px < hw; ++px)
          for (int e = 0; e < 2; ++e) host_dst[((size_t)b * hw + px) * 24 + 2 * q + e] = tmp[(size_t)b * per + ((size_t)q * hw + px) * 2 + e];
    return n;
  }
  if (which == 1 && h->plan.s2_px) {  // stage 2 lives in pair planes: gather the logical NHWC tensor on the host
    const size_t per = h->plan.dbg[1].per_img, hw = per / 48;
    std::vector<float> tmp(2 * (size_t)n);     // [buffer][image][pair][pixel][2]; on the device an image's two copies are adjacent
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy2D(tmp.data(), per * sizeof(float), h->ws.s2pp.p, 2 * per * sizeof(float), per * sizeof(float), (size_t)B, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy2D(tmp.data() + n, per * sizeof(float), h->ws.s2pp.p + per, 2 * per * sizeof(float), per * sizeof(float), (size_t)B, hipMemcpyDeviceToHost) != hipSuccess) {
      fail(h, YFV2_ERR_DEVICE, "yfv2_debug_activation: copy failed");
      return YFV2_ERR_DEVICE;
    }
    for (int b = 0; b < B; ++b)
      for (int q = 0; q < 24; ++q) {
        const float* src = tmp.data() + (size_t)h->plan.s2_buf[q] * n + (size_t)b * per + (size_t)q * hw * 2;
        for (size_t px = 0; px < hw; ++px)
          for (int e = 0; e < 2; ++e) host_dst[((size_t)b * hw + px) * 48 + h->plan.s2_label[2 * q + e]] = src[px * 2 + e];
      }
    return n;
  }
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(host_dst, h->plan.dbg[which].p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
    fail(h, YFV2_ERR_DEVICE, "yfv2_debug_activation: copy failed");
    return YFV2_ERR_DEVICE;
  }
  if (which == 2 && h->plan.c2_permuted) {   // stage 3 lives in the chain kernel's channel order: back to logical NHWC
    float tmp[96];
    for (int64_t px = 0; px < n / 96; ++px) {
      float* row = host_dst + px * 96;
      for (int k = 0; k < 96; ++k) tmp[h->plan.c2_label[k]] = row[k];
      std::memcpy(row, tmp, sizeof(tmp));
    }
  }
  return n;
}

}  // extern "C"
