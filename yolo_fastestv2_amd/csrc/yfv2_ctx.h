// yfv2_ctx.h - the handle behind yfv2_handle and the plumbing the API units share (yfv2_api.hip: lifetime, lanes, weights, forward
// and post; yfv2_api_frames.hip; yfv2_api_track.hip; yfv2_api_eval.hip; yfv2_api_debug.hip): error reporting, the device guard, the two owning memory
// types and the sized struct copies.  Private, like yfv2_plan.h; yfv2_train.hip reaches the handle through yfv2_internal.h's three
// accessors instead.  Brings the HIP runtime and <cstring>, <string>, <vector> to the units that include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/yfv2.h"
#include "yfv2_internal.h"
#include "yfv2_pack.h"
#include "yfv2_plan.h"

// the one error path (yfv2_ctx_fail, yfv2_api.hip): the message goes to the handle, if there is one, and to the thread's last error
inline int fail(yfv2_ctx* h, int code, const std::string& msg) { return yfv2_ctx_fail(h, code, msg.c_str()); }

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

// A device block that grows on demand.  reserve() does nothing while `need` fits; otherwise it waits for the device (an earlier
// call's launches, on any stream, may still be using the old block), frees it and allocates need + need / 2 - or exactly `need`
// for a block whose size never changes (allocated by its first use: handles that never need it keep their footprint).
// Released by the destructor, which calls no HIP function when the block is empty (the dry run's handle lives without a device).
struct DeviceBlock {
  void* p = nullptr;
  size_t bytes = 0;
  DeviceBlock() = default;
  DeviceBlock(const DeviceBlock&) = delete; DeviceBlock& operator=(const DeviceBlock&) = delete;   // one owner: the handle, never copied
  ~DeviceBlock() { if (p) (void)hipFree(p); }
  int reserve(yfv2_ctx* h, size_t need, bool exact = false) {
    if (need <= bytes) return YFV2_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    const size_t cap = exact ? need : need + need / 2;
    HIP_TRY(h, hipMalloc(&p, cap));
    bytes = cap;
    return YFV2_OK;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// 64 bytes of host-mapped, coherent memory that kernels store int32 words into through `dev` (a plain store) and the host reads
// through `host` once the kernel has completed.  `host` null with `dev` set: the word is another handle's (a lane uses its parent's).
struct MappedWord {
  int32_t* host = nullptr;
  int32_t* dev = nullptr;
  MappedWord() = default;
  MappedWord(const MappedWord&) = delete; MappedWord& operator=(const MappedWord&) = delete;
  ~MappedWord() { if (host) (void)hipHostFree(host); }
  bool alloc() {
    void* hp = nullptr; void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
      if (hp) (void)hipHostFree(hp);
      return false;
    }
    host = static_cast<int32_t*>(hp);
    dev = static_cast<int32_t*>(dp);
    return true;
  }
};

// A caller built against an older, shorter struct gets the fields it has (copy_sized: `src` into the caller's `dst`, struct_size =
// the bytes copied, which it returns) and gives the fields it has (read_sized: the rest stay 0).  struct_size <= 0 or too large: ours.
inline size_t sized_bytes(int32_t caller_struct_size, size_t ours) {
  return caller_struct_size > 0 && (size_t)caller_struct_size < ours ? (size_t)caller_struct_size : ours;
}
template <class T>
size_t copy_sized(T* dst, T src, int32_t caller_struct_size) {
  const size_t n = sized_bytes(caller_struct_size, sizeof(T));
  src.struct_size = (int32_t)n;
  std::memcpy(dst, &src, n);
  return n;
}
template <class T>
T read_sized(const T* src) {
  T v{};
  if (src) std::memcpy(&v, src, sized_bytes(src->struct_size, sizeof(T)));
  v.struct_size = (int32_t)sizeof(T);
  return v;
}

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
  ResizeFrame* d_frames = nullptr;   // frame descriptors of yfv2_resize_frames_u8 / yfv2_detect_frames_u8 (max_batch entries of the widest form, TrainFrame)
  ResizeFrameYuv* d_frames_yuv = nullptr;   // ... and of yfv2_resize_frames_yuv / yfv2_detect_frames_yuv (max_batch entries of TrainFrameYuv)
  DeviceBlock frames_u8;             // yfv2_detect_frames_u8's resized batch (max_batch, H, W, 3): allocated by its first call
  // tiled detection (yfv2_merge_tiles / yfv2_detect_tiled_u8).  tile_ws: the ordered candidate lists of tile_cap_t tiles (two float4
  // per row) and the tile / frame table of tile_cap_t + tile_cap_f entries; allocated by the first call, grown (one device wait) only by
  // a call with more tiles or frames than any before.  tile_out: yfv2_detect_tiled_u8's per-tile results (max_batch, 300, 6) +
  // idx (max_batch, 300) + count (max_batch), allocated by its first call.
  DeviceBlock tile_ws;
  int tile_cap_t = 0, tile_cap_f = 0;
  DeviceBlock tile_out;
  // second-stage crops (yfv2_crop_detections_u8 / _yuv, yfv2_crop_tensors_u8 / _yuv): max_batch int32 of per-frame selections, the
  // counted table's head (CropTensorHead: the tensor launches' constants, then the live count) and crop_cap descriptors of the widest
  // kind (TensorFrameYuv), which the plan launch writes and the resize launch reads.  Allocated by the first call (one device wait),
  // grown - another wait - only by a call with a larger cap.
  DeviceBlock crop_ws;
  int crop_cap = 0;
  // the ncnn sample's path (yfv2_deploy_post / yfv2_detect_deploy_frames_u8).  deploy_word: int32 `dropped` of the last call, then
  // max_batch (scaleW, scaleH) float pairs; deploy_maps: yfv2_detect_deploy_frames_u8's two export maps for max_batch images.  Both
  // are allocated by the first call that needs them (one device wait).
  DeviceBlock deploy_word;
  DeviceBlock deploy_maps;
  // the sticky range-guard word of the fp16x3 plan (yfv2_nonfinite): ONE int32.  The kernels store 1 into it (the rare path); the
  // host reads it after waiting for a stream (yfv2_nonfinite: exact) or without waiting (yfv2_nonfinite_peek: what has landed so far).
  MappedWord nonfinite;
  unsigned long long* d_probe = nullptr;   // yfv2_clock_probe_*: [probe_wgs][4] stamps of the last probe launch
  int probe_wgs = 0;
  // training-loss workspace (yfv2_loss): match slots for the labels, objectness target maps for max_batch images, counters and
  // float64 sums
  DeviceBlock loss_ws;
  // anchor k-means (yfv2_anchor_kmeans): chunk partials, the device `done` word and, when the caller wants no assignments, N
  // int32 of them.  km_word: int32[5] that the finalise launch publishes its verdict to (allocated by the first call)
  DeviceBlock km_ws;
  MappedWord km_word;
  int km_group = 8;              // passes enqueued between two looks at km_word (yfv2_debug_kmeans_group); changes no output bit
  // average precision (yfv2_ap_per_class): the result head, the sort's table and ping-pong buffers, the chunk sums (yfv2_ap.hip)
  DeviceBlock ap_ws;
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

// ---- yfv2_api.hip, for the other API units
int check_call(yfv2_ctx* h, int B, bool need_weights);                 // null handle, batch outside [1, max_batch], weights not loaded
int check_config(const yfv2_config* cfg, int* rows_out);               // yfv2_create's configuration checks; the decode row count
void read_plan_switches(yfv2_ctx* h, const yfv2_plan* plan);
int build_plan(yfv2_ctx* h, WeightPacker& wp, const yfv2_tensor_desc* tensors, int32_t n, yfv2_ctx* report);
int run_plan(yfv2_ctx* h, const void* x, bool x_u8, int B, float* const out6[6], hipStream_t stream, hipEvent_t* ev /*nullable: 2 per step*/,
             int only_step = -1 /* >= 0: this launch alone (yfv2_debug_repeat_step) */);
DecodeArgs decode_args(yfv2_ctx* h, const float* const out6[6], int32_t B);
// the NMS half of a post launch: candidates `boxes` (null: the fused launch decodes them itself), no class filter, no stamps
NmsArgs nms_args(const yfv2_ctx* h, const float* boxes, int compact, int32_t B, float conf_thres, double iou_thres, float* dets, int32_t* idx, int32_t* count);

// geometry + workspace of a handle; `alloc` is yfv2_create's hipMalloc or the dry run's address generator
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
