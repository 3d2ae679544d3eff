// yfv2_plan.h - the forward launch plan of libyfv2.so: what a handle launches for one forward, in order, built once per
// weight load from the model configuration (yfv2_plan.hip: PlanBuilder) and enqueued on the caller's stream by plan_run.
// Host only: no kernel.  The handle (yfv2_ctx.h), the workspace's memory and the entry points are the API units'.  Not part of the public ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <variant>
#include <vector>

#include "../../include/yfv2.h"
#include "yfv2_internal.h"
#include "yfv2_pack.h"

struct Buf { float* p = nullptr; size_t per_img = 0; };

inline size_t logit_elems(const yfv2_config& cfg, int i) {
  const int sc = i / 3, k = i % 3;
  const int c = k == 0 ? 4 * cfg.anchor_num : (k == 1 ? cfg.anchor_num : cfg.classes);
  return (size_t)c * (cfg.height / (16 << sc)) * (cfg.width / (16 << sc));
}

// workspace of a handle (NHWC fp32), sized for cfg.max_batch
struct Workspace {
  Buf a1, s2[2], s3[2], s4[2], t1, t2, t3, f2, f3, fq, ta, tb;
  Buf s2pp;  // stage 2 in pair planes: an image's two buffers back to back, [max_batch][2][24 pairs][H/8][W/8][2] (every offset a kernel adds to an
             // image base stays below 2 x 48 x H/8 x W/8 floats whatever max_batch is: no batch bound from 32-bit buffer offsets)
  Buf logits[6];
  Buf cand;  // (rows, 8) compact candidate rows of yfv2_detect
  // f(buffer, floats per image) for every buffer, in allocation order
  template <class F>
  void for_each(const yfv2_config& cfg, int rows, F f) {
    const size_t H = cfg.height, W = cfg.width;
    f(a1, (H / 4) * (W / 4) * 24);
    for (int i = 0; i < 2; ++i) {
      f(s2[i], (H / 8) * (W / 8) * 48);
      f(s3[i], (H / 16) * (W / 16) * 96);
      f(s4[i], (H / 32) * (W / 32) * 192);
    }
    f(s2pp, 2 * (H / 8) * (W / 8) * 48);
    f(t1, (H / 4) * (W / 4) * 24);
    f(t2, (H / 4) * (W / 4) * 24);
    f(t3, (H / 4) * (W / 4) * 24);
    f(f2, (H / 16) * (W / 16) * 72);
    f(f3, (H / 32) * (W / 32) * 72);
    f(fq, (H / 32) * (W / 32) * 72);   // the C3 part of fpn.conv1x1_2 (PW_DUAL -> PW_FPNQ)
    f(ta, (H / 16) * (W / 16) * 72);
    f(tb, (H / 16) * (W / 16) * 72);
    for (int i = 0; i < 6; ++i) f(logits[i], logit_elems(cfg, i));
    f(cand, (size_t)rows * 8);
  }
};

// the caller's plan switches (yfv2_create_ex; the library reads no environment) and what the builder derives from them
struct PlanSwitches {
  yfv2_plan plan{};
  bool bf6 = true;           // pointwise convs on the bf16 matrix cores where a kernel has that form (fp32_matrix: fp32 MFMA)
  bool front_wanted = true;  // stem + stage2.0 as one launch where the plan allows it (front_two_launches: two)
};

// ---- a step = one launch of the plan: a prototype of the kernel's argument struct (everything known when the plan is built) and
// the offsets of its packed images in the param blob; the runner completes a copy per call (batch, blob base, input, outputs)
struct StemStep {
  StemArgs args{};
  size_t img = 0, img_u8 = 0, img16 = 0;   // filter image for fp32 input, for uint8 input (1/255 folded in), stem_h3_kernel's two-term fp16 image
};
struct PwStep {
  PwArgs args{};
  int K = 0, mode = 0;
  int px_per_img = 0;          // P = B * px_per_img
  size_t img = 0;
  int head0 = -1, head1 = -1;  // PW_HEAD: indices into out6
};
struct DwStep {
  DwArgs args{};
  int ksize = 0, stride = 0;
  size_t w = 0, scale = 0, shift = 0;   // raw arrays in the blob
};
struct S2Step {   // fused stride-2 block (stage3.0, stage4.0; stage2.0 outside the lane-per-pixel plan)
  BlockS2Args args{};
  int cin = 0;
  size_t img = 0, img16 = 0;   // img16: the two-term fp16 image of s3h_kernel / s4h_kernel (0: none, the block runs on block_s2_kernel)
};
struct S2PxStep {   // stage2.0, lane per pixel
  S2PxArgs args{};
  size_t img_proj = 0, img_main = 0, img16 = 0;   // the two role kernels' images, s2h_kernel's two-term fp16 image (0: none)
  // front: the launch starts from the IMAGE (front_kernel: stem + stage2.0 in one wave); the stem's own step is Plan::stem_aside
  bool front = false;
  int H = 0, W = 0;            // front: the input image
  size_t img_stem16 = 0;       // front: the stem's img16
  std::string name_plain;      // front: the step's name as a launch of its own
};
struct S1PxStep {   // stride-1 block of stage 2, lane per pixel
  S1PxArgs args{};
  size_t img = 0, img16 = 0;   // s1px_kernel's image, s1h_kernel's
};
struct S1Step {     // a chain of stride-1 blocks as one launch
  BlockS1Args args{};
  bool pool = false;           // block_s1pool_kernel (whole activation resident in LDS; stage 4), else block_s1chain_kernel (stage 3)
  size_t img = 0;
};
struct TowerHalf {  // DWConvblock half (dw5x5+bn+relu -> pw+bn), the b halves with the output convs chained on
  std::string name;
  TowerArgs args{};
  size_t img = 0, img16 = 0;   // tower2_kernel's image, towerh_kernel's (0: none)
  bool has_head = false;
  int head0 = -1, head1 = -1;  // has_head: indices into out6
  int tiles = 0;               // output-conv tiles img16 is packed for (0, 1 or 6)
};
struct TowerStep {
  std::vector<TowerHalf> halves;   // 1, 2 or 4: the halves this ONE launch runs one after the other ...
  bool par = false;                // ... or (par) side by side: independent halves (cls a | reg a, cls b | reg b) as workgroup ranges
  int tiles = 0;                   // the launch's output-conv tiles
  unsigned char lane_patch[128] = {};   // TowerJobs::lane_patch where the step is towerp_kernel's (yfv2_towerp_map), set once by PlanBuilder
  bool has_lane_patch = false;          // ... which launch() insists on: an all-zero table would compute silently wrong logits
};

struct Step {
  std::string name;
  double flops = 0, bytes = 0;  // algorithmic, per image; bytes = per-LAYER accounting (every reference layer the launch covers reads its input and writes its output once)
  double bytes_ext = -1;        // SURVEY.md 8(d) for fused launches: EXTERNAL reads + writes of the launch only (-1: same as bytes)
  std::variant<StemStep, PwStep, DwStep, S2Step, S2PxStep, S1PxStep, S1Step, TowerStep> kind;
};

// everything the builder produces
struct Plan {
  std::vector<Step> steps;
  // stem + stage2.0 as ONE launch (front_kernel, yfv2_stage2h.hip): steps[0] is then that launch and the stem's own step is kept HERE, for
  // yfv2_debug_activation(0), which re-runs it on the last input, and for the image view of the dry-run hooks
  bool front_fused = false;
  Step stem_aside;
  bool stem_pp = false;     // the stem writes pair planes [12][H/4][W/4][2] for stage2.0 (the fp32-matrix plan: stem_px -> s2px kernels)
  // pair-plane bookkeeping at the END of stage 2 (for the stride-2 consumer and for yfv2_debug_activation)
  bool s2_px = false;
  int s2_label[48] = {0};   // logical channel stored in slot 2*pair + element
  int s2_buf[24] = {0};     // which of the two buffers holds pair p
  bool c2_permuted = false; // stage 3's output (C2) is stored in the chain kernel's order:
  int c2_label[96] = {0};   //   physical channel position k holds logical channel c2_label[k]
  // which buffers hold the stage outputs of a forward (yfv2_debug_activation): stem, stages 2-4, the two FPN maps
  struct Activation { float* p = nullptr; size_t per_img = 0; int c = 0; } dbg[6];
};

// Builds the plan of a configuration and packs its images into wp, whose index() has accepted the caller's tensors (no fold can
// fail after that).  False: a layout rule did not hold; *out is then untouched.
bool plan_build(const yfv2_config& cfg, const PlanSwitches& sw, const Workspace& ws, WeightPacker& wp, Plan* out);

// kernel (family) a step launches, as it appears in a rocprofv3 kernel trace (prefix of the symbol name)
std::string step_kernel(const Step& st);
// offset of the step's packed image in the blob (the first one where a launch has several; 0 for a depthwise step)
size_t step_image(const Step& st);

// what a launch needs from the call
struct RunCtx {
  const float* params = nullptr;   // device base of the blob
  const void* x = nullptr;         // input images, fp32 or (x_u8) uint8
  bool x_u8 = false;
  int B = 0;
  float* const* out6 = nullptr;
  hipStream_t stream = nullptr;
  bool bf6 = true;
  int32_t* nonfinite = nullptr;    // range-guard word
  long long* trace = nullptr;      // cycle-stamp buffer where the trace names this step, ...
  long long* trace_unnamed = nullptr;   // ... where it names none (only the stage-3 chain stamps then)
};
StemArgs stem_launch_args(const StemStep& st, const RunCtx& c);

// Enqueues the plan (only_step >= 0: that launch alone) on c.stream; ev (nullable): two events per step, the profile pass.
// trace / trace_step: the handle's stamp buffer and the step it names (-1: none).  YFV2_OK, or a code with *err set.
int plan_run(const Plan& plan, const RunCtx& c, long long* trace, int trace_step, hipEvent_t* ev, int only_step, std::string* err);
