// yfv2_internal.h - launch-argument structs, launcher declarations and the launch macros shared by the kernel translation
// units, the host-side weight packer (yfv2_pack.hip) and the host-side plan (yfv2_plan.hip).  No device-only code: what only runs on
// the device and is shared between kernel units lives in yfv2_device.h.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <atomic>
#include <cmath>

#include "../../include/yfv2.h"   // the YFV2_YUV_* format names

// Every launch of the forward path goes through YFV2_LAUNCH.  Normally a plain launch; while yfv2_profile_forward runs a plan step, the
// step's FIRST launch records its own begin and every launch its own end into the calling thread's event pair (hipExtLaunchKernel: the
// dispatch's own timestamps - what rocprofv3 reports - instead of hipEventRecord packets in front of and behind the launch, which
// read 3-12 us more per launch: round 6, profiles/r06_experiments.txt 14).
struct Yfv2LaunchProbe { hipEvent_t start = nullptr, stop = nullptr; int launches = 0; };
extern thread_local Yfv2LaunchProbe yfv2_launch_probe;
#define YFV2_LAUNCH(kernel, grid, block, lds, stream, ...)                                                                        \
  do {                                                                                                                             \
    Yfv2LaunchProbe& yfv2_lp_ = yfv2_launch_probe;                                                                                 \
    hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, yfv2_lp_.launches++ == 0 ? yfv2_lp_.start : nullptr, yfv2_lp_.stop, 0, \
                          __VA_ARGS__);                                                                                            \
  } while (0)
// ---- device facts of the launchers: the ONE place that asks which device is current and how many CUs it has.  A launcher (or the
// plan step above it) asks ONCE per launch and hands the value to its grid and to YFV2_LAUNCH_LDS: one hipGetDevice per launch
struct Yfv2Device { int index, cus; };   // index into 64-entry per-device caches; compute units (256, an MI355X, if the query fails)
inline Yfv2Device yfv2_device() {
  static std::atomic<int> cus_of[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 0;
  int cus = cus_of[dev].load(std::memory_order_relaxed);
  if (cus <= 0) { if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256; cus_of[dev].store(cus, std::memory_order_relaxed); }
  return {dev, cus};
}
inline int yfv2_device_cus() { return yfv2_device().cus; }
// grid of a persistent launch over n work items (images, mostly), one workgroup per CU at most: with n <= CUs every workgroup has
// exactly ONE item - which launch(const TowerStep&) (yfv2_plan.hip) relies on, through this very function
inline int yfv2_image_grid(int n, const Yfv2Device& dev) { return n < dev.cus ? n : dev.cus; }
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-(function, device) attribute: raise it to `bytes` the first time a function
// is launched on each device (`done` = the call site's bit mask of devices already served).  YFV2_LAUNCH_LDS = that + YFV2_LAUNCH,
// and owns the call site's word; YFV2_LDS_FULL = a CU's whole LDS, for kernels without static LDS of their own.
constexpr int YFV2_LDS_FULL = 160 * 1024;
inline void yfv2_allow_lds(const Yfv2Device& dev, const void* fn, int bytes, std::atomic<unsigned long long>& done) {
  const unsigned long long bit = 1ull << dev.index;
  if (done.load(std::memory_order_relaxed) & bit) return;
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done.fetch_or(bit, std::memory_order_relaxed);
}
#define YFV2_LAUNCH_LDS(dev, kernel, limit, grid, block, lds, stream, ...)            \
  do {                                                                                \
    static std::atomic<unsigned long long> yfv2_lds_done_{0};                         \
    yfv2_allow_lds(dev, reinterpret_cast<const void*>(&kernel), limit, yfv2_lds_done_); \
    YFV2_LAUNCH(kernel, grid, block, lds, stream, __VA_ARGS__);                       \
  } while (0)

// ---- stem: conv3x3 s2 (3->24) + BN + ReLU + maxpool3x3 s2, NCHW in -> NHWC out
struct StemArgs {
  const void* x;       // fp32 (B,3,H,W) in [0,1], or (u8_in) uint8 (B,H,W,3) in 0..255
  float* out;          // (B,H/4,W/4,24) NHWC, or pair planes (pp_out)
  const float* img;    // broadcast-form filter [11 regs][64 lanes] (BN scale folded) + shift[24], see WeightPacker::image_stem
  int B, H, W;
  int R;               // pooled rows per band (set by the launcher, divides H/4)
  int u8_in;           // input is uint8 NHWC; img_u8 = the filter image with 1/255 folded in
  const float* img_u8;
  int pp_out;          // 1: write pair planes [B][12][H/4][W/4][2] (stage 2 in lane-per-pixel form), 0: NHWC
  const float* img16;  // yfv2_stem16.hip (fp32 input on the f16 matrix cores): filter as two fp16 terms in MFMA A-operand order
                       // [tile 2][term 2][64 lanes][4 dwords] | shift * 2^sw [32] | 2^-sw (WeightPacker::image_stem16); null: use the 4x4x1 kernel
  int* nonfinite;      // the handle's sticky range-guard word (Yfv2Watch), or null
};

// ---- pointwise 1x1 conv on the fp32 MFMA, NHWC
enum { PW_PLAIN = 0, PW_SHUFFLE = 1, PW_FPN = 2, PW_HEAD = 3,
       // round 6: fpn.conv1x1_2 without its 192 upsampled channels.  A 1x1 conv commutes with the nearest-neighbour upsample, so the C3 part of
       // conv1x1_2 (fpn.py:57-59) is computed ONCE per coarse pixel - Q = scale2 * (W2[:, :192] C3) + shift2, by the launch that computes
       // conv1x1_3 from the same C3 (PW_DUAL: two filter images, even workgroups the first, odd workgroups the second -> `copy`, no ReLU) -
       // and the fine-map launch is a K = 96 conv over C2 whose epilogue adds Q at (y / 2, x / 2) (PW_FPNQ: `in2` = Q)
       PW_DUAL = 4, PW_FPNQ = 5 };
struct PwArgs {
  const float* in;     // NHWC activations (PW_FPN: C3, coarse map)
  const float* in2;    // PW_FPN only: C2, fine map
  float* out;          // NHWC output (unused for PW_HEAD)
  const float* img;    // filter fragments [MT][K/16][64][4] (+ 8-channel tail [MT][64][2]), then scale[MT*16], shift[MT*16]
  int P;               // pixels = B*H*W
  int M;               // real output channels (<= 16*MT)
  int in_stride;       // floats per input pixel
  int in_off;          // first input channel (PW_PLAIN)
  int out_stride;      // floats per output pixel
  int out_off;         // first output channel
  int relu;
  float* copy;         // PW_SHUFFLE: even input channels (pass-through branch) are copied to
  int copy_stride;     //   copy[pix*copy_stride + copy_off + j]
  int copy_off;
  int H, W;            // PW_FPN: fine map size; PW_HEAD: H*W in HW
  int HW;
  float* nchw0;        // PW_HEAD: co <  split -> nchw0[b][co][hw]
  float* nchw1;        // PW_HEAD: co >= split -> nchw1[b][co-split][hw]
  int split;
  int ctot0, coff0;    // PW_HEAD writing a channel RANGE of a wider tensor (more than 93 classes: the class head in slices of 96):
                       // nchw0 has ctot0 channels per image (0: = split) and this launch's channel co lands at coff0 + co
  int bf6;             // run the MFMAs as bf16x6 where the instantiation has that form (handle flag, YFV2_BF6=0 at create time clears it)
  int presplit;        // img holds the filter PRE-SPLIT into bf16 hi/mid/lo operand quads per chunk pair (WeightPacker::image_pw, streamed K = 192 / 288 forms; needs bf6)
  int* nonfinite;      // range-guard word (Yfv2Watch), or null
};

// ---- depthwise kxk conv + BN (+ReLU), NHWC, float4 over channels
struct DwArgs {
  const float* in;
  float* out;
  const float* w;      // [k*k][C]
  const float* scale;  // [C]
  const float* shift;  // [C]
  int B, H, W, C;      // input size, channels (C % 4 == 0)
  int OH, OW;
  int in_stride, in_off;
  int out_stride, out_off;
  int relu;
};

// ---- chains of fused ShuffleV2 stride-1 blocks (yfv2_block.hip)
struct BlockS1Args {
  const float* in;   // (B,H,W,2*C2) NHWC
  float* out;        // (B,H,W,2*C2) NHWC, distinct from in
  const float* img;  // the blocks' LDS images back to back (host-packed, WeightPacker::append_s1_bf6 / image_s1pool)
  long long* trace;  // debug: workgroup 0 / thread 0 writes s_memtime stamps at phase boundaries (or null)
  int B, H, W;
  int R;             // rows per work item (H % R == 0)
  int nblk;          // block_s1chain_kernel: blocks in the chain (img = their images back to back)
  int presplit;      // block_s1pool_kernel: the images hold W1 / W2 pre-split for bf16x6 (yfv2_s1pool_image_floats(true) floats each)
  int* nonfinite;    // range-guard word (Yfv2Watch), or null
  float* park;       // block_s1chain6_kernel: scratch for the parked values, yfv2_s1chain_park_floats() floats per image (any dead buffer)
};

// chain of N stride-1 blocks in one launch (block_s1chain6_kernel, C2 = 48, bf16x6 pointwise convs on host-pre-split
// filters); see PlanBuilder::s1chain_block for the channel bookkeeping shared by host and kernel
bool yfv2_s1chain_supported(int c2, int H, int W);
int yfv2_s1chain_image_floats();                                    // floats per block image (incl. the two int tables)
long yfv2_s1chain_park_floats(int H, int W, int nblk);              // park scratch per image
bool yfv2_launch_block_s1chain(const BlockS1Args& a, hipStream_t s);
// chain of stride-1 blocks with the whole 192-channel activation resident in LDS (block_s1pool_kernel, stage 4 at 11x11):
// natural channel order, no bookkeeping; img = per block three images of yfv2_s1pool_image_floats() floats (one per third)
bool yfv2_s1pool_supported(int c2, int H, int W);
int yfv2_s1pool_image_floats(bool presplit);
bool yfv2_launch_block_s1pool(const BlockS1Args& a, hipStream_t s);

// ---- fused ShuffleV2 stride-2 block (yfv2_block.hip)
struct BlockS2Args {
  const float* in;   // (B,H,W,CIN) NHWC
  float* out;        // (B,H/2,W/2,2*CIN) NHWC
  const float* img;  // LDS image: W1 | W2 | Wproj | main dw taps | proj dw taps | 10 BN vectors [10][KS]
  int B, H, W;       // input size
  int R;             // output rows per work item
  int s4_main_bands; // s4h_kernel, maps up to 16 columns wide: > 0 = one workgroup per image, waves 0 .. n-1 run the MAIN branch on n bands of rows,
                     // wave 3 the PROJ branch on all rows (the main branch is five times the proj branch's instructions); 0 = two units x two roles
  // pair-plane input (stage 2 in lane-per-pixel form, yfv2_stage2.hip): in = buffer 0 of the stage, pair p of
  // image b lives at in + b*pp_imgstride + p*H*W*2 (+ pp_bufstride floats if bit p of pp_mask is set): an image's two buffers are
  // adjacent (pp_bufstride = CIN*H*W, pp_imgstride twice that), so no offset grows with the batch
  int pp_in;
  unsigned pp_mask;
  long long pp_bufstride;
  long long pp_imgstride;
  int bf6;           // pw1 as bf16x6 (pair-plane input form)
  long long* trace;  // debug: per-wave cycle stamps of workgroup 0 (block_s2w_kernel; or null)
  const float* img16;  // s3h_kernel's image (stage3.0 from pair planes in streaming form, yfv2_stage2h.hip; WeightPacker::image_s3h) or null
  int* nonfinite;      // range-guard word (Yfv2Watch), or null
};
bool yfv2_s3h_supported(int H, int W);
void yfv2_launch_s3h(const BlockS2Args& a, hipStream_t s);
bool yfv2_s4h_supported(int H, int W);                         // stage4.0 (96 -> 192, NHWC in) in streaming form with two wave roles
void yfv2_launch_s4h(const BlockS2Args& a, hipStream_t s);

// ---- stage 2 in lane-per-pixel form (yfv2_stage2.hip)
// slot s = 2*pair + element of the pair-plane layout -> logical channel of the stage's FIRST block output
// (the stride-2 block) stored there.  Slots are grouped by the low three bits of the channel: stride-1
// block j of the stage reads exactly the pairs whose slot label has bit j set (see Stage2Layout).
__host__ __device__ inline int yfv2_stage2_channel(int slot) {
  const int p = slot >> 1, e = slot & 1;
  const int b0 = p / 12, b1 = (p % 12) / 6, b2 = (p % 6) / 3, h = 2 * (p % 3) + e;
  return b0 + 2 * b1 + 4 * b2 + 8 * h;
}
struct S1PxArgs {
  float* act;          // the stage: [max_batch][2 buffers][24 pairs][H][W][2] (src_off / dst_off carry the buffer: + 48*H*W floats for buffer 1)
  const float* img;    // w1q[10][64] | w2q[10][64] | (unused 24) | dw taps [9][24]  (WeightPacker::image_s1px)
  int B, H, W;
  int nstrips, nb, R;  // set by the launcher
  int img_stride;      // floats per image (2*48*H*W: both buffers)
  int num_records;     // bytes addressable from an image base (covers its copy in buffer 1)
  int src_off[12];     // byte offsets (from the image base in buffer 0) of the 12 branch pairs: where they are read ...
  int dst_off[12];     // ... and where the block's output for the same pairs is written (the other buffer)
  const float* img16;  // s1h_kernel's image (yfv2_stage2h.hip, WeightPacker::image_s1h); null: s1px_kernel
  int* nonfinite;      // range-guard word (Yfv2Watch), or null
};
// stride-2 block of stage 2 (24 -> 48 channels) in lane-per-pixel form; two wave roles (proj / main branch)
struct S2PxArgs {
  const float* in;     // stem output in pair planes: [B][12 pairs][IH][IW][2]
  float* act;          // stage-2 buffer 0: [max_batch][24 pairs][OH][OW][2]
  const float* img[2]; // role images: [0] proj: pwq[10][64] | taps[54][64]; [1] main: w1q | w2q | taps
  int B, IH, IW;
  int nstrips, nb, R;  // set by the launcher
  int in_stride, out_stride;       // floats per image
  int in_records, out_records;     // bytes addressable from an image base
  int st2_off[2][8];   // per role: byte offsets of the 8 pair planes its output positions 0..15 fill (8-byte stores)
  int st1_off[2][8];   // per role: byte offsets (plane + element) of output positions 16..23 (4-byte stores)
  const float* img16;  // s2h_kernel's image (yfv2_stage2h.hip, WeightPacker::image_s2h: both branches in one wave); null: the two role kernels
  int* nonfinite;      // range-guard word (Yfv2Watch), or null
};
// stem + stage2.0 in one wave (front_kernel, yfv2_stage2h.hip): the fp32 input image straight to stage 2's pair planes
struct FrontArgs {
  const void* x;         // fp32 (B,3,H,W), or (u8_in, front2_kernel only) uint8 (B,H,W,3)
  int H, W;
  int u8_in;
  const float* img_stem; // WeightPacker::image_stem16
  S2PxArgs s2;           // as for s2h_kernel (IH x IW = H/4 x W/4; in unused)
};
void yfv2_launch_front(const FrontArgs& a, hipStream_t s);
void yfv2_launch_s2px(const S2PxArgs& a, hipStream_t s);   // a.img16 set: yfv2_launch_s2h (one kernel); else two kernels (proj role, main role)
void yfv2_launch_s2h(const S2PxArgs& a, hipStream_t s);
bool yfv2_s1px_supported(int H, int W);
void yfv2_launch_s1px(const S1PxArgs& a, hipStream_t s);   // a.img16 set: yfv2_launch_s1h
void yfv2_launch_s1h(const S1PxArgs& a, hipStream_t s);

// ---- fused DWConvblock half (yfv2_block.hip): dw5x5+BN+ReLU -> pw72+BN [-> output conv]
struct TowerArgs {
  const float* in;   // (B,H,W,72) NHWC
  float* out;        // (B,H,W,72) NHWC when there is no chained output conv
  const float* img;  // LDS image: pw [80][84] | output conv [mh16][84] (if any) | dw taps [25][80] | scd shd scp shp bias [5][96]
  int has_head;      // chained output conv present
  int mh, split;     // co < split -> nchw0[b][co][hw], else nchw1[b][co-split][hw]
  float* nchw0; float* nchw1;
  int B, H, W;
  long long* trace;  // debug: per-wave cycle stamps of workgroup 0 (or null)
  int bf6;           // pointwise + chained output conv as bf16x6
  const float* img16;  // towerh_kernel's image (yfv2_towerh.hip), or null: tower2_kernel
  int chain;           // towers_kernel job list: bit 0 = the input is what the previous job left in LDS, bit 1 = the output stays in LDS for the next job (no global round trip)
  int* nonfinite;      // range-guard word (Yfv2Watch), or null
};

// ---- decode (handel_preds) and NMS
struct DecodeArgs {
  const float* reg[2];
  const float* obj[2];
  const float* cls[2];
  float* boxes;        // (B, rows, 5+classes), or
  float* cand;         // (B, rows, 8) compact candidate rows (non-null selects the compact kernel)
  int B, classes;
  int fh[2], fw[2];    // feature map sizes
  float stride[2];     // cfg.height / fh  (fp32, like the reference's python float)
  double anchors[12];
  int rows;            // 3*(fh0*fw0 + fh1*fw1)
};

struct NmsArgs {
  const float* boxes;  // (B, rows, 5+classes), or (B, rows, 8) when compact
  int compact;
  float* dets;         // (B, 300, 6)
  int32_t* idx;        // (B, 300)
  int32_t* count;      // (B)
  const int32_t* classes;  // optional class filter (device), may be null
  int n_classes;
  int B, rows, nc;
  float conf_thres;
  double iou_thres;
  long long* trace;    // debug: workgroup 0 / thread 0 writes cycle stamps at phase boundaries (or null)
};

// launchers (defined next to the kernels)
void yfv2_launch_stem(const StemArgs& a, hipStream_t s);      // picks yfv2_stem16.hip's kernel for fp32 input when a.img16 is set
void yfv2_launch_stem16(const StemArgs& a, hipStream_t s);
// K in {24,48,72,96,192,288}; mode PW_*; returns false if the (K, mode, M) combination has no kernel
bool yfv2_launch_pw(int K, int mode, const PwArgs& a, hipStream_t s);
int yfv2_pw_tiles(int K, int mode, int M);   // M tiles of the kernel instantiation yfv2_launch_pw uses (the host packs for that many)
bool yfv2_pw_presplit_supported(int K, int mode, int M);   // the launch has a pre-split (bf16 hi/mid/lo operand quads) form
bool yfv2_launch_dw(int ksize, int stride, const DwArgs& a, hipStream_t s);
int yfv2_block_s2_rows(int cin, int H, int W);
bool yfv2_launch_block_s2(int cin, const BlockS2Args& a, hipStream_t s);
bool yfv2_tower2_supported(int H, int W);                    // whole-image tower kernel: maps up to 22x22
bool yfv2_launch_tower2(const TowerArgs& a, hipStream_t s);
bool yfv2_towerh_supported(int H, int W);
bool yfv2_towerh_multi(int H, int W);
bool yfv2_towerp_map(int H, int W);   // a supported map whose single halves and side-by-side jobs are towerp_kernel's (even, beyond 11x11)
void towerp_lane_patches(int H, int W, unsigned char (&tbl)[128]);   // host: TowerJobs::lane_patch of such a map, a pure function of (H, W)
struct TowerJobs {   // up to four tower halves of one map size in ONE launch
  TowerArgs j[4];
  int n;
  int par;   // 0: a job LIST - every workgroup runs the jobs one after the other on its image (towers_kernel, maps up to 11x11);
             // 1: INDEPENDENT jobs side by side - workgroups [k gpj, (k + 1) gpj) run job k (towerh_kernel)
  int gpj;   // par: workgroups per job (set by the launcher)
  unsigned char lane_patch[128];   // towerp_kernel: the 2x2 patch of lane l in depthwise round r at [64 r + l] (255: none); the plan's (towerp_lane_patches)
};
bool yfv2_launch_towerh(const TowerJobs& jobs, int mh_tiles, const Yfv2Device& dev, hipStream_t s);   // dev: the caller's yfv2_device()
// ---- evaluation statistics (get_batch_statistics): which detections are true positives
struct StatsArgs {
  const float* dets;     // (B, 300, 6) x1,y1,x2,y2,conf,cls rows of yfv2_nms / yfv2_detect
  const int32_t* count;  // (B)
  const float* targets;  // (T, 6) image index, label, x1, y1, x2, y2 (pixels), the layout evaluation() builds (utils.py:372-376)
  int32_t* tp;           // (B, 300) 1 = true positive
  int32_t* overflow;     // set to 1 if an image has more than STATS_MAX_TARGETS targets (result then invalid)
  int B, T;
  float iou_thres;
};
constexpr int STATS_MAX_TARGETS = 1024;
void yfv2_launch_stats(const StatsArgs& a, hipStream_t s);
struct StatsMultiArgs {   // the same matching at K thresholds: bit k of tpmask = StatsArgs::tp at thr[k]
  const float* dets; const int32_t* count; const float* targets;
  uint32_t* tpmask;      // (B, 300)
  int32_t* overflow;
  int B, T, K;           // 1 <= K <= 32
  float thr[32];
};
void yfv2_launch_stats_multi(const StatsMultiArgs& a, hipStream_t s);
// ---- training loss and its gradient w.r.t. the logits (yfv2_loss.hip; utils/loss.py:8-208)
struct LossMatch {            // one (scale, offset candidate, anchor, label) slot of build_target
  int valid, b, a, gj, gi, cls;
  float tb[4];                // target box: (gx - cell x, gy - cell y, gw, gh) in grid units, fp32
  double aw, ah;              // anchor / stride, float64
};
struct LossArgs {
  const float* reg[2]; const float* obj[2]; const float* cls[2];   // the six logit maps (NCHW)
  float* grad_reg[2]; float* grad_obj[2]; float* grad_cls[2];      // d total / d logits (all null: forward only); reg / cls pre-zeroed
  const float* targets;       // (T, 6) image, class, cx, cy, w, h (normalised), device
  LossMatch* matches;         // 2 * 5 * 3 * T slots
  unsigned char* tobj[2];     // objectness targets (B, 3, H, W), pre-zeroed
  int* nb;                    // matches per scale [2], pre-zeroed
  double* sums;               // per scale: sum(1 - ciou), sum(objectness BCE), sum(class CE)  [2][3], pre-zeroed
  float* losses;              // out: lbox, lobj, lcls, total
  int B, T, classes;
  int fh[2], fw[2];
  double stride[2];           // cfg.width / fw
  double anchors[12];
};
void yfv2_launch_loss(const LossArgs& a, hipStream_t s);
// ---- pre-process: bilinear resize of uint8 HWC frames (yfv2_pre.hip)
struct ResizeArgs {
  const unsigned char* src;  // (B, SH, SW, 3)
  unsigned char* dst;        // (B, H, W, 3), 4-byte aligned, W % 4 == 0
  int B, SH, SW, H, W;
  double scale_x, scale_y;   // 1 / (W / SW), 1 / (H / SH) in double, like cv::resize derives them
};
void yfv2_launch_resize(const ResizeArgs& a, hipStream_t s);   // LDS: yfv2_rows_lds_bytes(YFV2_ROWS_U8, YFV2_FRAMES_BGR, a.SW, a.W)
// The row kernels of a ragged batch (yfv2_pre.hip): one workgroup per (table entry, output row) resizes a frame's row and hands it
// to the epilogue of its row kind.  A row kind and a frame kind name the instantiation and with it the table's descriptor type and
// dst's element type; yfv2_pre.hip holds the one description of each (its LDS layout, hence its bytes and its width limit).
enum Yfv2FrameKind {       // what a frame's samples are
  YFV2_FRAMES_BGR,         // packed B, G, R bytes (yfv2_frame)
  YFV2_FRAMES_YUV8,        // yfv2_frame_yuv, 1-byte samples: NV12, NV21, I420
  YFV2_FRAMES_YUV16,       // yfv2_frame_yuv, 2-byte samples: P010, I010 (the descriptors are the 1-byte kind's, byte for byte)
  YFV2_FRAMES_YUV8_ANY,    // yfv2_frame_yuv, 1-byte samples of ANY sampling: the three above and I422, I440, I444, YUYV, UYVY, GREY - the kind of a
                           // batch with at least one frame that is not 4:2:0 (the same descriptors again)
};
enum Yfv2RowKind {         // descriptor (B, G, R / YUV)            dst
  YFV2_ROWS_U8,            // ResizeFrame / ResizeFrameYuv          uint8 (n, H, W, 3), 4-byte aligned
  YFV2_ROWS_COUNTED_U8,    // CropFrame / CropFrameYuv              uint8 (n, H, W, 3): the live entries of a counted table
  YFV2_ROWS_TRAIN,         // TrainFrame / TrainFrameYuv            fp32 (n, 3, H, W), 16-byte aligned
  YFV2_ROWS_TENSOR_F32,    // TensorFrame / TensorFrameYuv          fp32 (n, 3, H, W), 16-byte aligned: the live entries, letterboxed
  YFV2_ROWS_TENSOR_F16,    // likewise                              fp16
};
constexpr int YFV2_ROW_KINDS = 5;
// grid n * H (n: the batch, or a counted table's capacity), LDS for a source row of max_w pixels
void yfv2_launch_rows(Yfv2RowKind kind, Yfv2FrameKind frames, const void* table, int n, int max_w, void* dst, int H, int W, hipStream_t s);
size_t yfv2_rows_lds_bytes(Yfv2RowKind kind, Yfv2FrameKind frames, int w, int W);   // LDS of one workgroup for a frame w pixels wide, output rows of W
// The widest frame the entry points of the kind admit.  B, G, R: (YFV2_LDS_FULL - the row's own bytes) / 6 - (ALIGN + 2) / 3, every
// row up to it fits; YUV, every kind: the widest frame that fits.  A 16-byte kind never admits a frame that the uint8 kinds
// refuse at the same W, and neither 2-byte samples nor the general 1-byte kind one that the 4:2:0 1-byte kind refuses.
int yfv2_rows_max_width(Yfv2RowKind kind, Yfv2FrameKind frames, int W);
// one frame of a ragged batch (yfv2_resize_frames_u8 / yfv2_detect_frames_u8), expanded on the host and uploaded as a table
struct ResizeFrame {
  const unsigned char* data;  // first byte of the frame (any alignment), device
  long long pitch;            // bytes from one row to the next, >= 3 w
  int h, w;
  double scale_x, scale_y;    // resize: 1 / (W / w), 1 / (H / h), as ResizeArgs
  double box_x, box_y;        // frame-coordinate epilogue: w / W, h / H (test.py:58)
};
// one YUV 4:2:0 frame of a ragged batch (yfv2_resize_frames_yuv / yfv2_detect_frames_yuv): the caller's yfv2_frame_yuv with its
// origin folded into the plane pointers on the host - pixel (r, c) of the frame has its luma at y[r * pitch_y + c] and its chroma
// at row (r + py) >> 1, sample (c + px) >> 1 of ca / cb - so the kernel sees every frame, crop or not, as a plane set of its own
// A frame of 2-byte samples (YFV2_YUV_P010 / _I010: bit 4 of the format) is the same descriptor: every sample index below is doubled
// to a byte offset, the planes are 2-byte aligned and the pitches even, and the coefficients are the 10-bit table's.
struct YuvCoef { int off, cy, cvr, cvg, cug, cub; };   // one row of a colour table (yfv2_pre.hip)
__host__ __device__ constexpr int yfv2_yuv_sample_bytes(int format) { return (format & 16) ? 2 : 1; }
// What a format is (include/yfv2.h YFV2_YUV_*): planar = U and V in planes of their own (I420, I422, I440, I444, I010); packed = one
// plane of 4-byte macropixels (YUYV: Y0 U Y1 V, UYVY: U Y0 V Y1); grey = luma only; and the chroma shifts - pixel (R, C) takes the
// chroma sample (R >> sy, C >> sx).  The five 4:2:0 formats have sx = sy = 1.  Comparisons, not a table: the kernels evaluate them on
// a run-time format.
__host__ __device__ constexpr bool yfv2_yuv_planar(int format) { return format == YFV2_YUV_I420 || format == YFV2_YUV_I010 || (format >= YFV2_YUV_I422 && format <= YFV2_YUV_I444); }
__host__ __device__ constexpr bool yfv2_yuv_packed(int format) { return format == YFV2_YUV_YUYV || format == YFV2_YUV_UYVY; }
__host__ __device__ constexpr bool yfv2_yuv_grey(int format) { return format == YFV2_YUV_GREY; }
__host__ __device__ constexpr int yfv2_yuv_shift_x(int format) { return format == YFV2_YUV_I440 || format == YFV2_YUV_I444 || format == YFV2_YUV_GREY ? 0 : 1; }
__host__ __device__ constexpr int yfv2_yuv_shift_y(int format) { return format == YFV2_YUV_I422 || (format >= YFV2_YUV_I444 && format <= YFV2_YUV_GREY) ? 0 : 1; }
__host__ __device__ constexpr bool yfv2_yuv_is420(int format) { return yfv2_yuv_shift_x(format) == 1 && yfv2_yuv_shift_y(format) == 1; }
struct ResizeFrameYuv {
  const unsigned char* y;     // luma of pixel (0, 0): plane + y0 * pitch_y + x0 (any alignment), device
  const unsigned char* ca;    // NV12 / NV21 / P010: the interleaved plane at chroma row y0 >> 1, sample pair x0 >> 1; I420 / I010: the U plane at (y0 >> 1, x0 >> 1)
  const unsigned char* cb;    // I420 / I010: the V plane likewise; NV12 / NV21 / P010: null
  long long pitch_y, pitch_c; // bytes from one row to the next
  int h, w;
  // (the other 8-bit samplings, yfv2_yuv_move: I422 / I440 / I444 as I420 with their own shifts; YUYV / UYVY: y the luma byte of pixel
  // (0, 0), ca the U byte of its macropixel, cb null, pitch_c = pitch_y; GREY: ca and cb null)
  int px, py;                 // x0 & 1, y0 & 1 on a subsampled axis (0 on any other): the parity of the origin decides which pixels share a chroma sample
  int format;                 // YFV2_YUV_*
  YuvCoef coef;               // the colour standard's row, copied in by the host: the kernel does not wait for a second, dependent load
  double scale_x, scale_y;    // resize: 1 / (W / w), 1 / (H / h), as ResizeArgs
};
// THE FOLD of an origin into the plane pointers, written once for the host (a caller's x0, y0; a tile's) and the device (a crop's
// rectangle, yfv2_crops.hip): the descriptor's pixel (dy, dx) becomes its pixel (0, 0).  h and w stay the caller's to set.
// By format: a pixel is sb bytes of luma (2 in a packed plane); a chroma sample is (dx + px) >> sx columns and (dy + py) >> sy rows
// away, a column being sb bytes of a planar plane, 2 sb of an interleaved one and 4 of a packed one; a parity is kept only on an
// axis that is subsampled; GREY has no chroma to move.  A PACKED frame's one plane is both: y is the luma byte of pixel (0, 0), ca
// the U byte of the macropixel that holds it, pitch_c = pitch_y.  For the five 4:2:0 formats every result is what it was.
__host__ __device__ inline void yfv2_yuv_move(ResizeFrameYuv& r, int dx, int dy) {
  const bool planar = r.cb != nullptr;
  const int sx = yfv2_yuv_shift_x(r.format), sy = yfv2_yuv_shift_y(r.format);
  const int cx = (dx + r.px) >> sx, cy = (dy + r.py) >> sy;  // chroma sample / row of the new origin, from the old one's
  const int sb = yfv2_yuv_sample_bytes(r.format);            // an offset in samples is sb times that in bytes
  const bool packed = yfv2_yuv_packed(r.format);
  const long long coff = (long long)cy * r.pitch_c + (long long)cx * (packed ? 4 : (planar ? 1 : 2) * sb);
  r.y += (long long)dy * r.pitch_y + (long long)dx * (packed ? 2 : sb);
  if (!yfv2_yuv_grey(r.format)) r.ca += coff;
  if (planar) r.cb += coff;
  r.px = sx ? (dx + r.px) & 1 : 0; r.py = sy ? (dy + r.py) & 1 : 0;
}
// The resize scale of one axis, `in` source pixels to `out`: cv::resize's inv_scale = dsize / ssize, scale = 1 / inv_scale, two
// correctly rounded fp64 divisions on either side (no unit that calls it has a fast-math flag).
__host__ __device__ inline double yfv2_resize_scale(int out, int in) { return 1.0 / ((double)out / (double)in); }
YuvCoef yfv2_yuv_coef(int colour, int sample_bytes = 1);   // YFV2_BT601_LIMITED .. YFV2_BT709_FULL -> its row of the 8-bit (1) or 10-bit (2) table
// The training entry points (yfv2_train_batch_frames_u8 / _yuv): a frame's resize descriptor with its contrast / brightness pair
// behind it, in the same table and the same one copy (the handle's tables are sized for these).  The resize kernels keep their own
// descriptors and strides; the training kernels run the same body on the base part.
struct TrainFrame : ResizeFrame { float alpha, beta; };
struct TrainFrameYuv : ResizeFrameYuv { float alpha, beta; };
// The descriptors of the 2-byte instantiations of resize_frames_yuv_kernel: the layouts above, the sample width in the TYPE, so that
// the 1-byte instantiations keep their names and their instruction streams.  The host and the crop plan write the 1-byte types.
template <class D> struct Samples16 : D { static constexpr int SAMPLE_BYTES = 2; };
// ... and of the GENERAL 1-byte instantiations (YFV2_FRAMES_YUV8_ANY), which read every 8-bit format: the same layouts again, and in
// the type the fact that the sampling is not known to be 4:2:0 - the kernel derives it from the format, uniformly over a workgroup.
template <class D> struct AnySampling : D { static constexpr bool ANY_SAMPLING = true; };
// ---- second-stage crops (yfv2_crop_detections_u8 / _yuv; kernels: yfv2_crops.hip, the resize launch: yfv2_launch_rows)
// THE RECTANGLE RULE, one axis of it, written once: yfv2_crop_rect (host) and the plan kernels (device) both call this function;
// include/yfv2.h states it for callers, tests/crops_model.py in Python.  a1, a2: the box's two edges on the axis; pad: the factor;
// n: the frame's length.  IEEE double throughout, every operation rounded on its own (the pragma holds whatever the unit's flags).
// false: the row is skipped.  true: 0 <= o < o + len <= n, so the conversion to int needs no clamp behind it.
__host__ __device__ inline bool yfv2_crop_axis(double a1, double a2, double pad, int n, int& o, int& len) {
#pragma clang fp contract(off)
  const double b = a2 - a1;
  if (!(b > 0.0)) return false;
  const double m = pad * b;
  const double lo = a1 - m, hi = a2 + m;
  const double c1 = lo > 0.0 ? lo : 0.0;                 // max(ax1, 0)
  const double c2 = hi < (double)n ? hi : (double)n;     // min(ax2, n)
  if (!(c2 > c1)) return false;
  o = (int)floor(c1);
  len = (int)ceil(c2) - o;
  return true;
}
// ... and the whole rule for one row: the four coordinates finite, both extents > 0, then each axis.  rect = X0, Y0, width, height.
__host__ __device__ inline bool yfv2_crop_row_rect(const float box[4], int frame_h, int frame_w, float pad_x, float pad_y, int rect[4]) {
  for (int i = 0; i < 4; ++i)
    if (!(fabsf(box[i]) <= 3.402823466e38f)) return false;   // NaN or an infinity
  const double x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
  if (!(x2 - x1 > 0.0) || !(y2 - y1 > 0.0)) return false;
  return yfv2_crop_axis(x1, x2, (double)pad_x, frame_w, rect[0], rect[2]) && yfv2_crop_axis(y1, y2, (double)pad_y, frame_h, rect[1], rect[3]);
}
// A descriptor table the DEVICE writes: the resize kernels' descriptors with a head of 16 bytes directly in front of entry 0 whose
// first int32 is the number of live entries.  A workgroup of a counted instantiation whose entry is not live returns at once.
template <class D> struct Counted : D { static constexpr bool COUNTED = true; };
struct CountedHead { int32_t live; int32_t pad[3]; };
using CropFrame = Counted<ResizeFrame>;
using CropFrameYuv = Counted<ResizeFrameYuv>;
struct CropPlanArgs {
  const float* dets;           // (B, R, 6): x1, y1, x2, y2, conf, cls in frame coordinates
  const int32_t* count;        // (B)
  int B, R;
  int out_h, out_w;
  float pad_x, pad_y;
  int max_per_frame;
  uint32_t classes[8];         // bit c: class c passes (0..254); all 255 set = no filter
  int32_t* n_sel;              // workspace (B): the frame's selected rows, written by the count launch, read by the write launch
  int32_t* src;                // (cap) b * R + r
  int32_t* rect;               // (cap, 4)
  int32_t* offset;             // (B + 1)
  int32_t* skipped;            // (B) or null
  int cap;
  CountedHead* head;           // directly in front of the descriptor table
};
// ---- second-stage crops as network input (yfv2_crop_tensors_u8 / _yuv): the same plan, the same resize body, the
// row leaves as fp32 / fp16 planes.  THE TWO RULES of it, each written once: yfv2_crop_letterbox / yfv2_crop_tensor_value (host) and
// the kernels (device) call these functions; include/yfv2.h states them for callers, tests/crop_tensors_model.py in numpy.
// Where a cw x ch rectangle lands in the (H, W) output: inner = ox0, oy0, iw, ih.  Integers throughout, int64 intermediates.
__host__ __device__ inline void yfv2_crop_letterbox_inner(int cw, int ch, int H, int W, int letterbox, int inner[4]) {
  long long iw = W, ih = H;
  if (letterbox) {
    if ((long long)W * ch <= (long long)H * cw) ih = (2ll * ch * W + cw) / (2ll * cw);   // round-half-up of ch * W / cw, <= H
    else iw = (2ll * cw * H + ch) / (2ll * ch);
    if (ih < 1) ih = 1;
    if (iw < 1) iw = 1;
  }
  inner[0] = letterbox ? (int)((W - iw) >> 1) : 0;
  inner[1] = letterbox ? (int)((H - ih) >> 1) : 0;
  inner[2] = (int)iw; inner[3] = (int)ih;
}
// What byte a becomes in a plane with (mean, std): two fp32 divisions and a subtraction, each rounded on its own - torchvision's
// ToTensor then Normalize.  (__fdiv_rn: the device's IEEE-correct division whatever the unit's flags; the host's / is one.)
__host__ __device__ inline float yfv2_crop_tensor_f32(int a, float mean, float std) {
#pragma clang fp contract(off)
#ifdef __HIP_DEVICE_COMPILE__
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)a, 255.f), mean), std);
#else
  const float x = (float)a / 255.f;
  const float d = x - mean;
  return d / std;
#endif
}
// ... and its binary16 form: one more rounding, to nearest even; overflow gives an infinity
__host__ __device__ inline _Float16 yfv2_crop_tensor_f16(int a, float mean, float std) { return (_Float16)yfv2_crop_tensor_f32(a, mean, std); }
// The descriptors of the tensor launches: the crop's counted descriptor with the inner rectangle behind it; scale_x / scale_y are
// those of the INNER size (iw, ih), not of (H, W).  The call's constants travel in front of the table's CountedHead, written by
// the plan's write launch: the descriptor load stays 16 bytes above the crop's, and the resize templates keep their signatures.
struct CropTensorParams {
  float mean[3], std[3];       // by OUTPUT plane
  uint32_t fill;               // B | G << 8 | R << 16, the frame's byte order
  int32_t rgb;                 // 1: plane c is byte channel 2 - c
};
struct CropTensorHead { CropTensorParams p; CountedHead head; };   // head last: entry 0 follows it, as in every counted table
template <class D> struct Letterboxed : Counted<D> { int ox0, oy0, iw, ih; static constexpr bool LETTERBOX = true; };
using TensorFrame = Letterboxed<ResizeFrame>;
using TensorFrameYuv = Letterboxed<ResizeFrameYuv>;
struct CropTensorPlanArgs : CropPlanArgs { CropTensorParams p; int letterbox; };   // the crop kinds' arguments stay what they were
// The plan of either family, two launches: frames = the batch's ResizeFrame / ResizeFrameYuv table (yuv, either sample
// width: the fold reads the format), table = the counted table it writes - CropFrame / CropFrameYuv, whose kernels take the
// CropPlanArgs part of a by value, or (tensor) TensorFrame / TensorFrameYuv.  The rows of the table's live entries are then
// yfv2_launch_rows' (YFV2_ROWS_COUNTED_U8, YFV2_ROWS_TENSOR_*).
void yfv2_launch_crop_plan(const CropTensorPlanArgs& a, bool tensor, bool yuv, const void* frames, void* table, hipStream_t s);
// ---- the per-stream IoU tracker (yfv2_track_update; kernel and the IoU's one function: yfv2_track.hip)
constexpr int TRACK_MAX_R = 4096, TRACK_MAX_M = 1024;
constexpr int TRACK_HEADER = 8, TRACK_SLOT = 10;     // int32 words of a stream's header and of one slot (include/yfv2.h)
constexpr int TRACK_CHUNK = 768;                     // frames of one launch: their streams are 3 KB of the launch's arguments
// the motion form (yfv2_track_update_motion): a slot is 32 words, words 10..29 the filters of cx, cy, w, h (5 each)
constexpr int TRACK_SLOT_MOTION = 32, TRACK_FILTER = 10;
struct TrackMotion { float std_pos, std_vel, std_meas; };
struct TrackArgs {
  const float* dets;           // (B, R, 6), offset to the launch's first frame
  const int32_t* count;        // (B), likewise
  int R, M;
  int32_t* state;              // S * (TRACK_HEADER + TRACK_SLOT * M) words
  double thres;
  int class_aware;
  float init_conf;
  int max_misses, confirm_hits;
  int32_t* track_id;           // (B, R), offset like dets
  int32_t* track_hits;         // (B, R) or null
  float* fresh_dets;           // (B, R, 6) or null; fresh_src (B, R) and fresh_count (B) with it
  int32_t* fresh_src;
  int32_t* fresh_count;
  int32_t stream_of[TRACK_CHUNK];   // workgroup g updates stream stream_of[g]
};
struct TrackMotionArgs : TrackArgs {   // the plain form's arguments stay what they were: its kernel is the one it was
  TrackMotion motion;
  float* track_box;            // (B, R, 4) or null, offset like dets
};
// the two-pass form (yfv2_track_update_two_pass): either layout, the rounds run over the HIGH rows and then the LOW
struct TrackTwoArgs : TrackMotionArgs {   // the other forms' arguments stay what they were: their kernels are the ones they were
  float high_conf, low_conf;   // a valid row is HIGH at conf >= high_conf, LOW at low_conf <= conf < high_conf, else takes no part
  double thres_low;            // the second pass's edge: double(IoU) > thres_low
  int tracked_only;            // != 0: a slot with misses != 0 at the frame's start is not offered to the second pass
  int32_t* track_pass;         // (B, R) or null, offset like dets
};
// the appearance form (yfv2_track_update_appearance): either layout, one pass or two; a track's feature is a slot of
// TRACK_FEAT_HEAD + D words in a buffer of its own (word 0: n_feat, then zeros, then the D fp32 bits of the unit feature)
constexpr int TRACK_FEAT_HEAD = 4, TRACK_APP_MIN_D = 16, TRACK_APP_MAX_D = 2048;
// LDS of one workgroup: the other forms' 24 R + 48 M (launch_track, yfv2_track.hip) and, in the appearance form, 4 bytes per row (its
// norm) and 4 per slot (its n_feat).  TRACK_APP_LDS_MAX: a CU's 160 KiB less 512 bytes for the kernel's static LDS (336 used).
constexpr size_t yfv2_track_lds_bytes(bool appearance, int R, int M) { return (size_t)(appearance ? 28 : 24) * R + (size_t)(appearance ? 52 : 48) * M; }
constexpr size_t TRACK_APP_LDS_MAX = (size_t)YFV2_LDS_FULL - 512;
struct TrackAppArgs : TrackTwoArgs {   // the other forms' arguments stay what they were: their kernels are the ones they were
  const float* emb;            // (B, R, D), offset like dets
  int32_t* feat;               // S * M * (TRACK_FEAT_HEAD + D) words
  float* track_cos;            // (B, R) or null, offset like dets
  int D;
  double prox, app;            // the cosine counts when double(IoU) > prox and double(cosine) > app
  float alpha, beta;           // the feature's moving average: alpha * f + beta * e / |e|, beta = 1.0f - alpha
};
// The limits of the entry points (yfv2_api_track.hip) and of the host arithmetic (yfv2_track.hip), each written once.
inline bool yfv2_track_tracks_ok(int32_t M) { return M >= 1 && M <= TRACK_MAX_M; }
inline bool yfv2_track_dim_ok(int32_t D) { return D >= TRACK_APP_MIN_D && D <= TRACK_APP_MAX_D && D % 16 == 0; }
inline bool yfv2_track_motion_ok(float std_pos, float std_vel, float std_meas) {
  return std::isfinite(std_pos) && std_pos > 0.f && std::isfinite(std_vel) && std_vel > 0.f && std::isfinite(std_meas) && std_meas > 0.f;
}
// The one launcher: form picks the instantiation of track_kernel, which takes the part of `a` that is its own argument type (the
// plain kernel its TrackArgs part, ...).  One workgroup per frame, frames <= TRACK_CHUNK; motion: a.state in 32-word slots.
struct TrackForm { bool motion, two_pass, appearance; };
void yfv2_launch_track(const TrackAppArgs& a, TrackForm form, int frames, hipStream_t s);
// dets columns 0-3 of the first count[b] rows of frame b times frames[b].box_x / box_y (yfv2_post.hip)
void yfv2_launch_frame_boxes(float* dets, const int32_t* count, const ResizeFrame* frames, int B, hipStream_t s);
void yfv2_launch_decode(const DecodeArgs& a, hipStream_t s);
void yfv2_launch_nms(const NmsArgs& a, hipStream_t s);
void yfv2_launch_decode_nms(const DecodeArgs& d, const NmsArgs& a, hipStream_t s);   // yfv2_detect: decode + NMS in one launch
bool yfv2_post_fusable(int classes, int rows);   // ... which exists for up to 96 classes and 2048 decode rows; beyond: two launches
int yfv2_nms_max_rows();                         // decode rows per image nms_kernel handles (4096)
// ---- tiled detection (yfv2_tiles.hip): a frame's tile detections -> one conf-descending list -> greedy walk
struct TileMergeArgs {
  const float* tile_dets;      // (T, 300, 6): rows of yfv2_detect_frames_u8, conf-descending per tile, tile coordinates
  const int32_t* tile_count;   // (T)
  const int32_t* table;        // device int32: [T][4] = x0, y0, k0, k1 (k0 <= k < k1: the tiles of tile k's frame), then [F][2] = k0, k1
  int T, F;
  float* geo;                  // workspace [T * 300] float4: x1, y1, x2, y2 in frame coordinates; frame f's ordered list starts at k0 * 300
  float* meta;                 // workspace [T * 300] float4: conf, class, origin k * 300 + r (int bits), area
  double thres;
  int metric;                  // 0: IoU, 1: intersection over the smaller box
  int max_out;                 // 1 .. 4096 (the kept set lives in LDS: 24 bytes per row)
  float* dets;                 // (F, max_out, 6)
  int32_t* src;                // (F, max_out) or null
  int32_t* count;              // (F)
};
void yfv2_launch_tile_merge(const TileMergeArgs& a, hipStream_t s);   // two launches: rank + scatter, then one workgroup per frame
// ---- the ncnn sample's deployment path (yfv2_deploy.hip; sample/ncnn/src/yolo-fastestv2.cpp)
struct ExportMapsArgs {
  const float* reg[2]; const float* obj[2]; const float* cls[2];   // the six NCHW logit maps
  float* map[2];               // (B, fh, fw, 15 + classes) NHWC: sigmoid(12 reg) | sigmoid(3 obj) | softmax(classes)
  int B, classes;
  int fh[2], fw[2];
};
void yfv2_launch_export_maps(const ExportMapsArgs& a, hipStream_t s);
struct DeployPostArgs {
  const float* map[2];         // the two maps of ExportMapsArgs (any producer)
  const float* scale;          // device (B, 2) fp32 scaleW, scaleH, or null = 1, 1
  int B, classes;
  int fh[2], fw[2];
  int stride[2];               // inputHeight / outH, integer (yolo-fastestv2.cpp:146)
  float anchors[12];           // the handle's anchors as the sample's std::vector<float> holds them
  int rows;                    // 3 * (fh0 fw0 + fh1 fw1) <= 4096
  float thresh, nms_thresh;
  int32_t* boxes;              // (B, max_out) records of 6 words: x1, y1, x2, y2, cate, score bits (yfv2_target_box)
  int32_t* count;              // (B): all survivors, also beyond max_out
  int max_out;                 // 1 .. rows
  int32_t* dropped;            // one device word, zeroed before the launch: candidates whose box is not representable
};
void yfv2_launch_deploy_post(const DeployPostArgs& a, hipStream_t s);
// ---- anchor k-means (yfv2_anchors.hip; genanchors.py:67-102): one pass = assign + partial sums, then finalise
constexpr int YFV2_KM_CH = 1024;    // points per chunk: part of the RESULT's definition (the summation tree), never tuned per device
constexpr int YFV2_KM_MAXK = 32;
struct KmArgs {
  const double* wh;      // (N, 2) label sizes
  int64_t N;
  double* centroids;     // (k, 2): read by the assign launch, rewritten by the finalise launch
  int k;
  int64_t nchunks;       // ceil(N / YFV2_KM_CH)
  int32_t* assign;       // (N): the previous pass's assignment in, this pass's out
  double* avg_iou;       // 1 double
  double* part_sum;      // [2k + 1][nchunks]: sum of w per cluster, sum of h per cluster, sum of max IoU
  int* part_cnt;         // [k][nchunks]
  int* part_flag;        // [nchunks]: bit 0 an assignment changed, bit 1 a w or h is not a finite number > 0
  int* done;             // device word: set by the finalise launch that ends the loop; every later launch returns at once
  int32_t* host_word;    // host-mapped int32[5]: done, iterations, converged, empty_cluster, bad_input
};
void yfv2_launch_km_pass(const KmArgs& a, int pass, int last, hipStream_t s);
// ---- average precision per class (yfv2_ap.hip; utils/utils.py:110-192 compute_ap + ap_per_class)
constexpr int YFV2_AP_CH = 1024;     // terms per chunk of the AP sum: part of the RESULT's definition (the summation tree), never tuned
constexpr int YFV2_AP_TILE = 2048;   // detections per workgroup of a radix-sort pass (changes no output bit: the sort is stable)
struct ApHead {                      // zeroed before every call, copied to the host in one piece after it
  long long n_gt[256], n_pred[256];
  double p[256], r[256], ap[256];
  int32_t bad, pad;
};
struct ApArgs {
  const int32_t* tp; const float* conf; const float* pred_cls;   // (N); tp is null in the multi-threshold form
  const uint32_t* tpmask;                                         // (N), multi-threshold form: bit k = tp at threshold k
  int K;                                                          // 0: the single-threshold form; 1..32: thresholds
  int64_t N;
  const float* target_cls;                                        // (T)
  int64_t T;
  uint32_t* key[2];    // (N) each: the order-preserving image of -conf, ping-pong
  uint32_t* val[2];    // (N) each: input index | tp << 31, ping-pong; the ranked list ends in val[1]
  uint32_t* hist;      // [256 digits][nblk]: per-workgroup digit counts, scanned in place along each row
  uint32_t* tot;       // [256]: row totals of the current pass
  double* part;        // chunk sums of the AP terms: class c's start at floor(segment start / YFV2_AP_CH) + c; threshold k's set at k * part_stride
  int64_t part_stride;
  uint32_t* pmask;     // (N), multi-threshold form: tpmask in rank order, bits at and above K cleared
  ApHead* head;        // max(K, 1) blocks; n_gt and bad live in block 0 alone
  int nblk;            // ceil(N / YFV2_AP_TILE)
};
size_t yfv2_ap_ws_bytes(int64_t N, int K);                            // the whole workspace, ApHead first (K = 0: the single-threshold form)
void yfv2_ap_carve(ApArgs& a, char* ws);                              // sets the workspace pointers of a (N and K already set)
void yfv2_launch_ap(const ApArgs& a, hipStream_t s);                  // memset of the head + every launch
struct yfv2_ap_result;
void yfv2_ap_finish(const ApHead& head, yfv2_ap_result* out);         // host: head -> result, means sequential over the present classes
void yfv2_ap_finish_multi(ApHead* heads, int K, yfv2_ap_result* out); // host: block 0's n_gt and bad into every block, then yfv2_ap_finish on each
// ---- measurement: effective shader clock (yfv2_probe.hip)
struct ClockProbeArgs {
  unsigned long long* out;       // [workgroups][4]: shader cycles, reference ticks, XCC id, (unused)
  unsigned long long ref_ticks;  // how long to stay, in ticks of the constant reference clock (s_memrealtime)
  int busy;                      // 1: dependent FMAs between the stamps, 0: s_sleep (runs beside other work without disturbing it)
};
bool yfv2_launch_clock_probe(const ClockProbeArgs& a, int workgroups, hipStream_t s);

// ---- training path (yfv2_train.hip): its state hangs off the handle through an opaque slot of the handle (yfv2_ctx.h)
struct yfv2_ctx;
struct yfv2_config;
void** yfv2_ctx_train_slot(yfv2_ctx* h);                       // null handle -> null
const yfv2_config* yfv2_ctx_config(yfv2_ctx* h);
int yfv2_ctx_fail(yfv2_ctx* h, int code, const char* msg);      // records the message, returns code
void yfv2_train_release(void* train_state);                    // called by yfv2_destroy
