// yfv2_api_debug.hip - host side of libyfv2.so, what measures and inspects: the host-only dry runs of the plan and the packer
// (yfv2_debug_plan_*), the row launches' LDS and width limits (yfv2_debug_rows), the clock probe, the per-launch profile pass, the repeated step and the activation dump.  The handle and
// the shared plumbing: yfv2_ctx.h.
#include <algorithm>
#include <cstdio>
#include <variant>

#include "yfv2_ctx.h"

namespace {

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

// The body of the three yfv2_debug_rows* exports: `who` is the entry point's name, for the message.
int debug_rows(const char* who, int32_t row_kind, Yfv2FrameKind frames, int32_t w, int32_t W, int64_t* lds_bytes, int32_t* max_width) {
  if (row_kind < 0 || row_kind >= YFV2_ROW_KINDS || w < 1 || w > (1 << 26) || W < 1 || W > (1 << 20))
    return fail(nullptr, YFV2_ERR_ARG, std::string(who) + ": bad argument");
  if (lds_bytes) *lds_bytes = (int64_t)yfv2_rows_lds_bytes((Yfv2RowKind)row_kind, frames, w, W);
  if (max_width) *max_width = yfv2_rows_max_width((Yfv2RowKind)row_kind, frames, W);
  return YFV2_OK;
}

}  // namespace

extern "C" {

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

// Host-only test hooks: the one description of the row kernels (yfv2_pre.hip) as the launches and the entry points' checks read it,
// so that the CPU suite can hold it against a restatement (tests/rows_model.py) for every row kind and frame kind.
int yfv2_debug_rows(int32_t row_kind, int32_t yuv, int32_t w, int32_t W, int64_t* lds_bytes, int32_t* max_width) {
  if (yuv < 0 || yuv > 1) return fail(nullptr, YFV2_ERR_ARG, "yfv2_debug_rows: bad argument");
  return debug_rows("yfv2_debug_rows", row_kind, yuv ? YFV2_FRAMES_YUV8 : YFV2_FRAMES_BGR, w, W, lds_bytes, max_width);
}

// ... of the YUV frame kind with two-byte samples (YFV2_YUV_P010 / _I010)
int yfv2_debug_rows16(int32_t row_kind, int32_t w, int32_t W, int64_t* lds_bytes, int32_t* max_width) {
  return debug_rows("yfv2_debug_rows16", row_kind, YFV2_FRAMES_YUV16, w, W, lds_bytes, max_width);
}

// ... and of the general 1-byte YUV frame kind (a batch with a frame that is not 4:2:0)
int yfv2_debug_rows_any(int32_t row_kind, int32_t w, int32_t W, int64_t* lds_bytes, int32_t* max_width) {
  return debug_rows("yfv2_debug_rows_any", row_kind, YFV2_FRAMES_YUV8_ANY, w, W, lds_bytes, max_width);
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
    yfv2_launch_decode_nms(decode_args(h, out6, B), nms_args(h, nullptr, 1, B, 0.3f, 0.4, p_dets, p_idx, p_cnt), s);
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
    const RunCtx c{h->d_params, h->last_x, h->last_u8, B, nullptr, nullptr, h->sw.bf6, h->nonfinite.dev};
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
