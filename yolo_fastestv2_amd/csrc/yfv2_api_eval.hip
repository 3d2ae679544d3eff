// yfv2_api_eval.hip - host side of libyfv2.so, the entry points of training and evaluation: batch statistics, the loss, anchor
// k-means and average precision.  The handle and the shared plumbing: yfv2_ctx.h.
#include "yfv2_ctx.h"

extern "C" {

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

// the synchronous forms: enqueue, read the overflow word (which waits for `stream`), refuse an overflow
static int stats_sync(yfv2_handle h, int rc, const char* name, void* stream) {
  if (rc) return rc;
  int32_t over = 0;
  rc = yfv2_batch_statistics_overflow(h, &over, stream);
  if (rc) return rc;
  if (over) return fail(h, YFV2_ERR_ARG, std::string(name) + ": an image has more than 1024 targets");
  return YFV2_OK;
}
int yfv2_batch_statistics(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets, int32_t T,
                          float iou_threshold, int32_t* tp, void* stream) {
  return stats_sync(h, yfv2_batch_statistics_async(h, dets, count, B, targets, T, iou_threshold, tp, stream), "yfv2_batch_statistics", stream);
}
int yfv2_batch_statistics_multi(yfv2_handle h, const float* dets, const int32_t* count, int32_t B, const float* targets, int32_t T,
                                const float* thresholds, int32_t K, uint32_t* tpmask, void* stream) {
  return stats_sync(h, yfv2_batch_statistics_multi_async(h, dets, count, B, targets, T, thresholds, K, tpmask, stream), "yfv2_batch_statistics_multi", stream);
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
  if (int rc2 = h->loss_ws.reserve(h, need)) return rc2;
  char* ws = h->loss_ws.as<char>();
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
  if (!h->km_word.host && !h->km_word.alloc()) return fail(h, YFV2_ERR_DEVICE, "hipHostMalloc(k-means word) failed");
  const int64_t nch = (N + YFV2_KM_CH - 1) / YFV2_KM_CH;
  // layout: [done word, 64 bytes][sums (2k + 1) nch doubles][counts k nch ints][flags nch ints][assignments N ints, if the caller has none]
  const size_t off_sum = 64, off_cnt = off_sum + sizeof(double) * (size_t)(2 * k + 1) * (size_t)nch;
  const size_t off_flag = off_cnt + sizeof(int) * (size_t)k * (size_t)nch, off_asg = off_flag + sizeof(int) * (size_t)nch;
  const size_t need = off_asg + (assign ? 0 : sizeof(int32_t) * (size_t)N);
  if (int rc = h->km_ws.reserve(h, need)) return rc;
  char* ws = h->km_ws.as<char>();
  KmArgs a{};
  a.wh = wh; a.N = N; a.centroids = centroids; a.k = k; a.nchunks = nch;
  a.assign = assign ? assign : reinterpret_cast<int32_t*>(ws + off_asg);
  a.avg_iou = avg_iou;
  a.done = reinterpret_cast<int*>(ws);
  a.part_sum = reinterpret_cast<double*>(ws + off_sum);
  a.part_cnt = reinterpret_cast<int*>(ws + off_cnt);
  a.part_flag = reinterpret_cast<int*>(ws + off_flag);
  a.host_word = h->km_word.dev;
  volatile int32_t* hw = h->km_word.host;   // every earlier call waited for its stream before it returned: nothing is writing the word now
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
  copy_sized(info, out, info->struct_size);
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
  if (int rc = h->ap_ws.reserve(h, yfv2_ap_ws_bytes(a.N, a.K))) return rc;
  yfv2_ap_carve(a, h->ap_ws.as<char>());
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
  copy_sized(out, res, out->struct_size);
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
  // the records lie one caller's struct apart
  const int32_t caller_size = out->struct_size;
  char* o = reinterpret_cast<char*>(out);
  for (int k = 0; k < K; ++k) o += copy_sized(reinterpret_cast<yfv2_ap_result*>(o), res[(size_t)k], caller_size);
  return YFV2_OK;
}

}  // extern "C"
