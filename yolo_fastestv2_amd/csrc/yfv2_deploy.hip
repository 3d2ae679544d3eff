// yfv2_deploy.hip - the ncnn sample's deployment path on the device: the export layout of
// Detector(export_onnx=True) (model/detector.py:33-44) and the sample's own post-process, predHandle + nmsHandle
// (sample/ncnn/src/yolo-fastestv2.cpp:58-183).  Built with FP contraction off: every fp32 and fp64 operation below rounds on
// its own, as the C++ of the sample does on a machine without fused multiply-add and as the numpy model of the rule does
// (tests/deploy_model.py); one fused operation changes a truncated integer.
//
//   export_maps_kernel  six NCHW logit maps -> two NHWC maps (B, fh, fw, 15 + classes): sigmoid(12 reg) | sigmoid(3 obj) |
//                       softmax(classes).  The geometry is decode_kernel's (yfv2_post.hip): up to 64 consecutive cells of one
//                       (image, scale) per workgroup, 4 lanes per cell for the softmax - the same device functions
//                       (yfv2_device.h), so obj and cls are the bits of yfv2_decode's columns 4 and 5.. - and the NCHW -> NHWC
//                       turn goes through LDS: every logit is read once, along the map (consecutive lanes = consecutive cells of a
//                       channel), the workgroup's cells are assembled as [cell][15 + classes] rows (row pitch made odd: the
//                       channel-major writes then spread over the banks) and leave as ONE contiguous span of the output.  95
//                       floats per pixel is no multiple of 4, so the span starts at any dword: up to three single stores bring
//                       it to a 16-byte boundary, 16-byte stores follow, up to three single stores end it.
//   deploy_post_kernel  one workgroup per image, everything in LDS:
//     1. candidates  getCategory per row in the sample's order (scale 0 then 1; h, w, anchor): 4 lanes share a cell's class vector
//                    (lane p takes classes p, p + 4, ..: the quad reads 16 contiguous bytes), each keeps per anchor the first
//                    maximum of fl32(cls * obj) above 0 in its slice, two exchanges pick the larger, on ties the lower class -
//                    the running max with strict > from tmp = 0.  A row whose score > thresh gets its box as C++ evaluates
//                    :163-171 (double arithmetic, float bcx / bw, truncation to int) and a slot; slots are handed out by an
//                    LDS atomic, in any order - the key carries the row.
//     2. order       keys (score bits << 32 | (4095 - row) << 12 | slot), bitonic sort, descending: score descending (a score
//                    above thresh >= 0 is positive: its bits order like its value), TIES BY CANDIDATE ORDER (lower row first).
//                    std::sort leaves ties unspecified; this is the rule the library pins.
//     3. greedy      :85-103.  Candidates are walked in order; one that no kept candidate has suppressed is kept, written to
//                    the output, and all threads mark the later candidates of its class whose IoU with it is > nmsThresh
//                    (intersection_area's four compares with > and <, int differences converted to float, float products,
//                    (area_i + area_j) - inter, IEEE division; 0 / 0 = NaN suppresses nothing).  One barrier per KEPT candidate.
//   LDS: 8 bytes per key (rows rounded up to a power of two) + 24 bytes per candidate record + 1 flag byte: 59 KB at 352x352
//   (1815 rows), 132 KB at the handle's limit of 4096 rows.
#include <hip/hip_runtime.h>

#include "yfv2_device.h"

namespace {

// ============================================================================
// export maps
// ============================================================================
template <int MAXPER>
__global__ __launch_bounds__(256) void export_maps_kernel(ExportMapsArgs a, int blocks0, int blocks1) {
  constexpr int CELLS = MAXPER > 24 ? 32 : 64, THREADS = 4 * CELLS;   // as decode_kernel: the wide form (up to 255 classes) halves the cells
  extern __shared__ __attribute__((aligned(16))) float stage[];       // [CELLS][CP]
  const int per_img = blocks0 + blocks1;
  const int b = blockIdx.x / per_img;
  int blk = blockIdx.x - b * per_img;
  const int sc = blk >= blocks0 ? 1 : 0;
  if (sc) blk -= blocks0;
  const int hw = a.fh[sc] * a.fw[sc];
  const int cell0 = blk * CELLS;
  const int ncell = min(CELLS, hw - cell0);
  const int nc = a.classes, C = 15 + nc, CP = C | 1;
  const int tid = threadIdx.x;
  const int lc = tid >> 2, part = tid & 3;
  const bool ok = lc < ncell;
  const int cc = ok ? cell0 + lc : cell0;   // clamp so that the quad exchanges stay convergent

  float ev[MAXPER];
  yfv2_softmax_quad<MAXPER>(a.cls[sc] + (size_t)b * nc * hw, nc, hw, cc, part, ev);
  if (ok) {
    const int per = (nc + 3) >> 2;
    const int c_lo = part * per, c_hi = min(nc, c_lo + per);
    float* srow = stage + lc * CP + 15;
#pragma unroll
    for (int i = 0; i < MAXPER; ++i)
      if (c_lo + i < c_hi) srow[c_lo + i] = ev[i];
  }
  // 12 reg + 3 obj channels: consecutive lanes read consecutive cells of one channel
  for (int i = tid; i < 15 * CELLS; i += THREADS) {
    const int ch = i / CELLS, l = i - ch * CELLS;
    if (l < ncell) {
      const float* src = ch < 12 ? a.reg[sc] + ((size_t)b * 12 + ch) * hw : a.obj[sc] + ((size_t)b * 3 + (ch - 12)) * hw;
      stage[l * CP + ch] = sigmoid_f32(src[cell0 + l]);
    }
  }
  __syncthreads();

  float* dst = a.map[sc] + ((size_t)b * hw + cell0) * C;     // the workgroup's cells are one contiguous span of n floats
  const int n = ncell * C;
  const float inv_c = 1.0f / (float)C;                       // 16 <= C <= 270, i < 64 * 270: yfv2_fdiv is exact here
  const int head = min(n, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u));
  const int body4 = (n - head) >> 2;
  const int tail0 = head + 4 * body4;
  auto at = [&](int i) { const int cell = yfv2_fdiv(i, inv_c); return stage[cell * CP + (i - cell * C)]; };
  if (tid < head) dst[tid] = at(tid);
  for (int q = tid; q < body4; q += THREADS) {
    const int i = head + 4 * q;
    int cell = yfv2_fdiv(i, inv_c), ch = i - cell * C;
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = stage[cell * CP + ch];
      if (++ch == C) { ch = 0; ++cell; }
    }
    *reinterpret_cast<f32x4*>(dst + i) = v;                  // 16-byte aligned by construction of `head`
  }
  if (tid < n - tail0) dst[tail0 + tid] = at(tail0 + tid);
}

// ============================================================================
// predHandle + nmsHandle
// ============================================================================
constexpr int DP_THREADS = 1024;   // 16 waves: one workgroup per image is latency-bound (as nms_kernel)
constexpr int DP_MAX_ROWS = 4096;  // 12 bits of row and 12 bits of slot in a key

// the value the sample converts with (int): representable, or the conversion is undefined in C++ (NaN, beyond int32)
__device__ __forceinline__ bool int_ok(double d) { return d > -2147483649.0 && d < 2147483648.0; }

__global__ __launch_bounds__(DP_THREADS) void deploy_post_kernel(DeployPostArgs a, int cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int rows = a.rows;
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(lds);   // [cap], cap = rows rounded up to a power of two
  int* const rec = reinterpret_cast<int*>(keys + cap);                           // [6][rows]: x1, y1, x2, y2, cate, score bits
  unsigned char* const supp = reinterpret_cast<unsigned char*>(rec + 6 * rows);  // [rows]
  __shared__ int n_cand, n_drop;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int nc = a.classes, C = 15 + nc;
  const int cells0 = a.fh[0] * a.fw[0], cells1 = a.fh[1] * a.fw[1];
  if (tid == 0) { n_cand = 0; n_drop = 0; }
  for (int i = tid; i < rows; i += DP_THREADS) supp[i] = 0;
  __syncthreads();

  // ---- 1. candidates
  const float scale_w = a.scale ? a.scale[2 * b] : 1.0f, scale_h = a.scale ? a.scale[2 * b + 1] : 1.0f;
  const int part = tid & 3;
  for (int q = tid >> 2; q < cells0 + cells1; q += DP_THREADS / 4) {              // (the four lanes of a quad share q)
    const int sc = q >= cells0 ? 1 : 0;
    const int cell = sc ? q - cells0 : q;
    const int fw = a.fw[sc];
    const int hh = cell / fw, ww = cell - hh * fw;
    const float* v = a.map[sc] + ((size_t)b * (sc ? cells1 : cells0) + cell) * C;
    const float o0 = v[12], o1 = v[13], o2 = v[14];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;                                            // getCategory: tmp = 0
    int j0 = -1, j1 = -1, j2 = -1;
    for (int c = part; c < nc; c += 4) {
      const float p = v[15 + c];
      const float t0 = __fmul_rn(p, o0), t1 = __fmul_rn(p, o1), t2 = __fmul_rn(p, o2);
      if (t0 > s0) { s0 = t0; j0 = c; }                                            // strict: the first maximum of this lane's classes
      if (t1 > s1) { s1 = t1; j1 = c; }
      if (t2 > s2) { s2 = t2; j2 = c; }
    }
    // the larger of two lanes, on ties the lower class (-1 = none, the largest unsigned): the first maximum over all classes
    auto merge = [&](float& s, int& j, int lane_xor) {
      const float os = __shfl_xor(s, lane_xor);
      const int oj = __shfl_xor(j, lane_xor);
      if (os > s || (os == s && (unsigned)oj < (unsigned)j)) { s = os; j = oj; }
    };
    merge(s0, j0, 1); merge(s1, j1, 1); merge(s2, j2, 1);
    merge(s0, j0, 2); merge(s1, j1, 2); merge(s2, j2, 2);
    const int cate = part == 0 ? j0 : (part == 1 ? j1 : j2);
    const float score = part == 0 ? s0 : (part == 1 ? s1 : s2);
    if (part < 3 && cate >= 0 && score > a.thresh) {                               // (cate < 0: score = -1, never above thresh >= 0)
      const int row = (sc ? 3 * cells0 : 0) + cell * 3 + part;
      const float r0 = v[4 * part + 0], r1 = v[4 * part + 1], r2 = v[4 * part + 2], r3 = v[4 * part + 3];
      const double st = (double)a.stride[sc];
      // :163-166  double arithmetic, one rounding to float each
      const float bcx = (float)((((double)r0 * 2. - 0.5) + (double)ww) * st);
      const float bcy = (float)((((double)r1 * 2. - 0.5) + (double)hh) * st);
      const double tw = (double)r2 * 2., th = (double)r3 * 2.;
      const float bw = (float)((tw * tw) * (double)a.anchors[(sc * 3 + part) * 2 + 0]);   // pow(x, 2) = x * x, exact for a float x
      const float bh = (float)((th * th) * (double)a.anchors[(sc * 3 + part) * 2 + 1]);
      // :168-171  double arithmetic, truncated toward zero
      const double dx1 = ((double)bcx - 0.5 * (double)bw) * (double)scale_w, dy1 = ((double)bcy - 0.5 * (double)bh) * (double)scale_h;
      const double dx2 = ((double)bcx + 0.5 * (double)bw) * (double)scale_w, dy2 = ((double)bcy + 0.5 * (double)bh) * (double)scale_h;
      if (int_ok(dx1) && int_ok(dy1) && int_ok(dx2) && int_ok(dy2)) {
        const int slot = atomicAdd(&n_cand, 1);                                    // < rows: one per row at most
        rec[0 * rows + slot] = (int)dx1; rec[1 * rows + slot] = (int)dy1; rec[2 * rows + slot] = (int)dx2; rec[3 * rows + slot] = (int)dy2;
        rec[4 * rows + slot] = cate; rec[5 * rows + slot] = __float_as_int(score);
        keys[slot] = ((unsigned long long)(unsigned)__float_as_int(score) << 32) | (unsigned long long)(((DP_MAX_ROWS - 1 - row) << 12) | slot);
      } else {
        atomicAdd(&n_drop, 1);                                                     // the sample is undefined here; the row is dropped and counted
      }
    }
  }
  __syncthreads();

  // ---- 2. order: bitonic sort of the first P >= n keys, descending (empty keys = 0 sink to the end)
  const int n = n_cand;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += DP_THREADS) keys[i] = 0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += DP_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long x = keys[i], y = keys[l];
        const bool desc = (i & k) == 0;
        if ((x < y) == desc) { keys[i] = y; keys[l] = x; }
      }
      __syncthreads();
    }
  }

  // ---- 3. greedy walk
  const int M = a.max_out;
  int32_t* const out = a.boxes + (size_t)b * M * 6;
  const float thr = a.nms_thresh;
  int nk = 0;
  for (int i = 0; i < n; ++i) {
    if (supp[i]) continue;                       // one LDS address for everybody; final: every kept candidate before i has finished its marks
    const int si = (int)(keys[i] & 0xfffull);
    const int bx1 = rec[si], by1 = rec[rows + si], bx2 = rec[2 * rows + si], by2 = rec[3 * rows + si], bc = rec[4 * rows + si];
    if (tid < 6 && nk < M) out[nk * 6 + tid] = rec[tid * rows + si];
    ++nk;
    const float barea = __fmul_rn((float)(int)((unsigned)bx2 - (unsigned)bx1), (float)(int)((unsigned)by2 - (unsigned)by1));   // TargetBox::area()
    for (int j = i + 1 + tid; j < n; j += DP_THREADS) {
      if (supp[j]) continue;
      const int sj = (int)(keys[j] & 0xfffull);
      if (rec[4 * rows + sj] != bc) continue;
      const int ax1 = rec[sj], ay1 = rec[rows + sj], ax2 = rec[2 * rows + sj], ay2 = rec[3 * rows + sj];
      float inter = 0.f;                                                          // intersection_area :58-70
      if (!(ax1 > bx2 || ax2 < bx1 || ay1 > by2 || ay2 < by1))
        inter = __fmul_rn((float)(int)((unsigned)min(ax2, bx2) - (unsigned)max(ax1, bx1)), (float)(int)((unsigned)min(ay2, by2) - (unsigned)max(ay1, by1)));
      const float aarea = __fmul_rn((float)(int)((unsigned)ax2 - (unsigned)ax1), (float)(int)((unsigned)ay2 - (unsigned)ay1));
      const float uni = __fsub_rn(__fadd_rn(aarea, barea), inter);                // :91
      if (__fdiv_rn(inter, uni) > thr) supp[j] = 1;                               // :92-94 (NaN: not above)
    }
    __syncthreads();
  }
  // records beyond min(count, max_out) are zero; count is the full number of survivors
  for (int i = min(nk, M) * 6 + tid; i < M * 6; i += DP_THREADS) out[i] = 0;
  if (tid == 0) {
    a.count[b] = nk;
    if (n_drop) atomicAdd(a.dropped, n_drop);
  }
}

}  // namespace

void yfv2_launch_export_maps(const ExportMapsArgs& a, hipStream_t s) {
  const int cells = a.classes <= 96 ? 64 : 32;
  const int b0 = (a.fh[0] * a.fw[0] + cells - 1) / cells, b1 = (a.fh[1] * a.fw[1] + cells - 1) / cells;
  const size_t lds = (size_t)cells * ((15 + a.classes) | 1) * sizeof(float);   // at most 64 x 111 or 32 x 271 floats: below 64 KB
  if (a.classes <= 96)
    YFV2_LAUNCH(export_maps_kernel<24>, dim3(a.B * (b0 + b1)), dim3(4 * cells), lds, s, a, b0, b1);
  else
    YFV2_LAUNCH(export_maps_kernel<64>, dim3(a.B * (b0 + b1)), dim3(4 * cells), lds, s, a, b0, b1);
}

void yfv2_launch_deploy_post(const DeployPostArgs& a, hipStream_t s) {
  int cap = 1;
  while (cap < a.rows) cap <<= 1;
  const size_t lds = (size_t)cap * 8 + (size_t)a.rows * 24 + (((size_t)a.rows + 15) & ~(size_t)15);
  // up to 132 KB of dynamic LDS next to the two static counters: raise the function's limit to exactly the 4096-row need, once per device
  YFV2_LAUNCH_LDS(yfv2_device(), deploy_post_kernel, DP_MAX_ROWS * (8 + 24 + 1), dim3((unsigned)a.B), dim3(DP_THREADS), lds, s, a, cap);
}
