// yfv2_pre.hip - the pre-process in front of the path: bilinear resize of uint8 HWC frames
// to the network input size, the arithmetic of `cv2.resize(img, (width, height), interpolation=cv2.INTER_LINEAR)`
// (test.py:35, utils/datasets.py:107) for 8-bit images: OpenCV's fixed-point path (imgproc/resize.cpp, pinned by the
// reference at opencv_python 4.2.0.34): per output column  fx = float((dx + 0.5) * scale_x - 0.5), sx = floor(fx),
// coefficients round_half_even((1 - fx) * 2048), round_half_even(fx * 2048) as int16 (sx < 0 or sx >= src_w - 1:
// clamp, fx = 0); the same per output row except that the two row INDICES are clipped instead of the weight; horizontal
// pass S = p[sx] * a0 + p[sx + 1] * a1 (int32), vertical pass ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.
// OpenCV itself is not in this image: the tests bit-compare this kernel with a numpy restatement of the same published
// algorithm - "parity unpinned" against cv2 proper.
//
// HBM-bound byte work.  One workgroup = one output row of one frame: the two source rows it blends are staged in LDS
// with aligned 4-byte loads (source row starts are arbitrary byte addresses), the blend reads LDS bytes, the output row
// is assembled in LDS and leaves as aligned 4-byte stores (width % 4 == 0, so every output row starts 4-byte aligned).
// Built with -ffp-contract=off: the coefficient arithmetic must round like the separate C operations it restates.
//
// The ragged-batch kernels are two templates over <Frame, Row> - the descriptor (B, G, R or YUV; plain, counted, with an augmentation
// pair, letterboxed) and where the blended row goes (uint8 batch, fp32 training batch, fp32 / fp16 tensor) - in twenty instantiations: five of the B, G, R template and fifteen of the YUV one (five each for 1-byte 4:2:0 samples, for 2-byte
// samples - P010, I010 - and for the general 1-byte kind, any 8-bit sampling).  With resize_u8_kernel the unit has 21 kernels.
// Each output kind is described ONCE: the Row states its ALIGN and its own LDS bytes, yfv2_slot places the staging slots for kernel and
// host alike, FrameRows<Frame> gives the launch's LDS and the width limit of the frame kind, launch_rows<Frame, Row> is the one launch
// body.  Other units reach the family through Yfv2RowKind, Yfv2FrameKind and yfv2_launch_rows / yfv2_rows_lds_bytes / yfv2_rows_max_width
// (yfv2_internal.h); yfv2_debug_rows shows the last two to tests/test_rows_host.py, which sweeps them against tests/rows_model.py.
#include <algorithm>
#include <type_traits>

#include "../../include/yfv2.h"
#include "yfv2_device.h"

// A staged source row in LDS: its bytes, up to 3 more in front (the row starts at any byte, the staging loads are aligned dwords),
// rounded up to `align` - 4, or what the Row behind the slots needs.  THE layout function: the kernels place their slots with it and
// the host sizes the launch with it (FrameRows below), so the two cannot drift apart.
__host__ __device__ constexpr int yfv2_slot(int bytes, int align) { return (bytes + 3 + align - 1) & ~(align - 1); }

struct RowCoef { int s0, s1, c0, c1; };

__device__ __forceinline__ RowCoef yfv2_axis_coef(int d, double scale, int n, bool clamp_weight) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  RowCoef r;
  if (clamp_weight) {            // columns: the weight is dropped at the borders
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
    r.s0 = s; r.s1 = min(s + 1, n - 1);
  } else {                       // rows: both indices are clipped, the weights stay
    r.s0 = min(max(s, 0), n - 1); r.s1 = min(max(s + 1, 0), n - 1);
  }
  r.c0 = __float2int_rn((1.f - f) * 2048.f);
  r.c1 = __float2int_rn(f * 2048.f);
  return r;
}

// One channel of one output pixel from its four taps (row s0 / s1 x column sx0 / sx1): the horizontal pass of each row, then the
// vertical pass and the clamp.  Every kernel below blends with this one expression.
__device__ __forceinline__ unsigned char yfv2_blend(int t00, int t01, int t10, int t11, const RowCoef& rx, const RowCoef& ry) {
  const int S0 = t00 * rx.c0 + t01 * rx.c1;
  const int S1 = t10 * rx.c0 + t11 * rx.c1;
  const int v = (((ry.c0 * (S0 >> 4)) >> 16) + ((ry.c1 * (S1 >> 4)) >> 16) + 2) >> 2;
  return (unsigned char)min(max(v, 0), 255);
}

// The output row assembled in OUT (LDS) leaves as aligned dwords: the barrier behind the blend, then row oy of image b of dst.
template <int THREADS>
__device__ __forceinline__ void yfv2_emit_row(const unsigned char* OUT, unsigned char* dst, int b, int oy, int H, int W) {
  __syncthreads();
  unsigned* drow = reinterpret_cast<unsigned*>(dst + ((size_t)b * H + oy) * W * 3);
  for (int i = threadIdx.x; i < (W * 3) >> 2; i += THREADS) drow[i] = reinterpret_cast<const unsigned*>(OUT)[i];
}

// ---- where a blended row of a ragged batch goes: the two epilogues of resize_frames_u8_kernel / resize_frames_yuv_kernel ----
// Those kernels are templates over their frame descriptor and a Row.  The kernel hands the Row the LDS behind its staging slots
// (ALIGN-byte aligned; the slots are rounded to it): begin, before the staging barrier; put, every blended byte (output column ox,
// channel c); end, the row is complete.  Everything in front of the Row - staging, guards, coefficients, blend - is the one body.
// A Row also states what the host needs of it: ALIGN and lds_bytes(W), its own LDS behind the slots for an output row of W pixels.
//
// RowU8: the uint8 (B, H, W, 3) batch of the resize entry points.  The row is assembled in LDS and leaves through yfv2_emit_row.
template <int THREADS>
struct RowU8 {
  using Out = unsigned char;
  static constexpr int ALIGN = 4;
  static constexpr bool AUGMENT = false;
  __host__ __device__ static constexpr int lds_bytes(int W) { return 3 * W; }
  unsigned char* dst;
  __device__ __forceinline__ void put(unsigned char* lds, int ox, int c, int W, unsigned char v) { lds[ox * 3 + c] = v; }
  __device__ __forceinline__ void end(const unsigned char* lds, int b, int oy, int H, int W) { yfv2_emit_row<THREADS>(lds, dst, b, oy, H, W); }
};

// THE AUGMENTATION TABLE (the specification; include/yfv2.h states it for callers, tests/train_batch_model.py in numpy): what
// utils/datasets.py:10-16 contrast_and_brightness, then train.py:101's .float() / 255.0, make of byte a with the frame's (alpha, beta):
//   t = fl32(fl32(float(a) * alpha) + beta)          two roundings, never an fma
//   q = rint_half_even(min(max(t, 0), 255))
//   table[a] = fl32(float(q) / 255)                  IEEE-correct fp32 division
// which is OpenCV's scalar saturate_cast<uchar>(a * alpha + 0 * (1 - alpha) + beta) for 8-bit addWeighted (the zero image makes the
// middle term exactly 0).  OpenCV's own vector body fuses the multiply-add and its tail does not, and OpenCV is not in this image:
// parity with cv2 proper is unpinned, exactly as for the resize above.  alpha = 1, beta = 0 is the identity (imgaug=False).
constexpr int YFV2_AUG_TABLE_BYTES = 256 * (int)sizeof(float);
__device__ __forceinline__ float yfv2_aug_entry(int a, float alpha, float beta) {
  const float t = __fadd_rn(__fmul_rn((float)a, alpha), beta);
  const int q = __float2int_rn(fminf(fmaxf(t, 0.f), 255.f));
  return __fdiv_rn((float)q, 255.f);
}

// RowTrain: the fp32 (B, 3, H, W) batch of the training entry points (the <TrainFrame, RowTrain> / <TrainFrameYuv, RowTrain> instantiations below).  Its LDS:
// the frame's table, filled by the workgroup itself before the staging barrier, then the row as three planes of W floats - the
// byte -> plane transposition: a thread's B, G, R of column ox go to planes[c][ox] (consecutive lanes, consecutive words).  After
// a barrier the planes leave as 16-byte stores, three contiguous runs of W floats out[b][c][oy][0 .. W): W % 32 == 0 and dst is
// 16-byte aligned, so every run is.
template <int THREADS>
struct RowTrain {
  using Out = float;
  static constexpr int ALIGN = 16;
  static constexpr bool AUGMENT = true;
  __host__ __device__ static constexpr int lds_bytes(int W) { return YFV2_AUG_TABLE_BYTES + 3 * W * (int)sizeof(float); }
  float* dst;
  __device__ __forceinline__ void begin(unsigned char* lds, float alpha, float beta) {
    for (int a = threadIdx.x; a < 256; a += THREADS) reinterpret_cast<float*>(lds)[a] = yfv2_aug_entry(a, alpha, beta);
  }
  __device__ __forceinline__ void put(unsigned char* lds, int ox, int c, int W, unsigned char byte) {
    reinterpret_cast<float*>(lds + YFV2_AUG_TABLE_BYTES)[c * W + ox] = reinterpret_cast<const float*>(lds)[byte];
  }
  __device__ __forceinline__ void end(const unsigned char* lds, int b, int oy, int H, int W) {
    __syncthreads();
    const float4* planes = reinterpret_cast<const float4*>(lds + YFV2_AUG_TABLE_BYTES);
    const int quads = W >> 2;                         // per plane
    for (int i = threadIdx.x; i < 3 * quads; i += THREADS) {
      const int c = i / quads, q = i - c * quads;
      reinterpret_cast<float4*>(dst + (((size_t)b * 3 + c) * H + oy) * W)[q] = planes[i];
    }
  }
};

// RowTensor: the (cap, 3, H, W) fp32 or fp16 tensor of the crop-tensor entry points (yfv2_crop_tensors_u8 / _yuv):
// a crop as a second network takes it.  The call's constants - mean, std, fill, the plane order - lie in front of the table's
// CountedHead (CropTensorHead); begin reads them, uniformly, and re-indexes mean / std by BYTE channel, so that the unrolled put
// indexes nothing at run time.  Every value is yfv2_crop_tensor_f32 / _f16 of its byte, evaluated directly: a crop's row is tens to
// a few hundred pixels, fewer values than the 768 entries a per-workgroup table would hold.  Its LDS: the row as three planes of W
// values in OUTPUT-plane order.  After a barrier the planes leave as 16-byte stores, three contiguous runs out[k][c][oy][0 .. W):
// W % 4 == 0 and dst is 16-byte aligned, so every fp32 run is; an fp16 run is when W % 8 == 0 and is 8-byte aligned otherwise, and
// then leaves as 8-byte stores.  A row outside the inner rectangle (letterbox) is a fill row: no staging, no LDS, no barrier.
template <int THREADS, bool HALF>
struct RowTensor {
  using Out = std::conditional_t<HALF, _Float16, float>;
  template <int N> using Vec = Out __attribute__((ext_vector_type(N)));
  static constexpr int ALIGN = 16;
  static constexpr bool AUGMENT = false;
  static constexpr bool TENSOR = true;
  static constexpr int N16 = 16 / (int)sizeof(Out);   // values of a 16-byte store
  __host__ __device__ static constexpr int lds_bytes(int W) { return 3 * W * (int)sizeof(Out); }
  Out* dst;
  float mean[3], std[3];      // by byte channel (B, G, R)
  int fill[3];
  int flip;                   // output plane of byte channel c: flip ? 2 - c : c
  template <class Frame>
  __device__ __forceinline__ void begin(const Frame* frames) {
    const CropTensorParams& p = reinterpret_cast<const CropTensorHead*>(frames)[-1].p;
    flip = p.rgb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mean[c] = flip ? p.mean[2 - c] : p.mean[c];
      std[c] = flip ? p.std[2 - c] : p.std[c];
      fill[c] = (int)((p.fill >> (8 * c)) & 255u);
    }
  }
  __device__ __forceinline__ int plane(int c) const { return flip ? 2 - c : c; }
  __device__ __forceinline__ Out value(int a, int c) const {
    if constexpr (HALF) return yfv2_crop_tensor_f16(a, mean[c], std[c]);
    else return yfv2_crop_tensor_f32(a, mean[c], std[c]);
  }
  __device__ __forceinline__ void put(unsigned char* lds, int ox, int c, int W, unsigned char byte) {
    reinterpret_cast<Out*>(lds)[plane(c) * W + ox] = value(byte, c);
  }
  __device__ __forceinline__ void put_fill(unsigned char* lds, int ox, int W) {
#pragma unroll
    for (int c = 0; c < 3; ++c) put(lds, ox, c, W, (unsigned char)fill[c]);
  }
  __device__ __forceinline__ Out* run(int b, int p, int oy, int H, int W) const { return dst + (((size_t)b * 3 + p) * H + oy) * W; }
  template <int N>
  __device__ __forceinline__ void emit(const unsigned char* lds, int b, int oy, int H, int W) {
    const int per = W / N;                              // stores per plane
    for (int i = threadIdx.x; i < 3 * per; i += THREADS) {
      const int p = i / per, q = i - p * per;
      reinterpret_cast<Vec<N>*>(run(b, p, oy, H, W))[q] = reinterpret_cast<const Vec<N>*>(lds)[i];
    }
  }
  __device__ __forceinline__ void end(const unsigned char* lds, int b, int oy, int H, int W) {
    __syncthreads();
    if (HALF && (W & 7)) emit<N16 / 2>(lds, b, oy, H, W);
    else emit<N16>(lds, b, oy, H, W);
  }
  template <int N>
  __device__ __forceinline__ void fill_run(Out* r, Out v, int W) {
    Vec<N> pat;
#pragma unroll
    for (int j = 0; j < N; ++j) pat[j] = v;
    for (int i = threadIdx.x; i < W / N; i += THREADS) reinterpret_cast<Vec<N>*>(r)[i] = pat;
  }
  __device__ __forceinline__ void fill_row(int b, int oy, int H, int W) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (HALF && (W & 7)) fill_run<N16 / 2>(run(b, plane(c), oy, H, W), value(fill[c], c), W);
      else fill_run<N16>(run(b, plane(c), oy, H, W), value(fill[c], c), W);
    }
  }
};

__global__ __launch_bounds__(256) void resize_u8_kernel(ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.H, oy = blockIdx.x - b * a.H;
  const RowCoef ry = yfv2_axis_coef(oy, a.scale_y, a.SH, false);
  const int row_bytes = a.SW * 3;
  const int slot = yfv2_slot(row_bytes, 4);           // staged bytes per source row (head misalignment + tail round-up)
  unsigned char* R0 = smem;
  unsigned char* R1 = smem + slot;
  unsigned char* OUT = smem + 2 * slot;
  // ---- stage the two source rows: aligned dwords covering [g, g + row_bytes)
  const size_t total = (size_t)a.B * a.SH * row_bytes;
  const size_t g0 = ((size_t)b * a.SH + ry.s0) * row_bytes, g1 = ((size_t)b * a.SH + ry.s1) * row_bytes;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.src);
  const int m0 = (int)((base + g0) & 3), m1 = (int)((base + g1) & 3);
  const int nd0 = (m0 + row_bytes + 3) >> 2, nd1 = (m1 + row_bytes + 3) >> 2;
  auto stage = [&](unsigned char* dst, size_t g, int mis, int nd) {
    const unsigned char* p = a.src + g - mis;        // 4-byte aligned
    for (int i = tid; i < nd; i += 256) {
      // the first / last dword of the very first / last row of the buffer may reach outside the allocation: bytes there
      const bool inside = (i > 0 || mis == 0 || g >= (size_t)mis) && (g - mis + 4 * (size_t)i + 4 <= total);
      unsigned v;
      if (inside) v = *reinterpret_cast<const unsigned*>(p + 4 * i);
      else {
        v = 0;
        for (int k = 0; k < 4; ++k) {
          const long long off = (long long)g - mis + 4ll * i + k;
          if (off >= 0 && (size_t)off < total) v |= (unsigned)a.src[off] << (8 * k);
        }
      }
      *reinterpret_cast<unsigned*>(dst + 4 * i) = v;
    }
  };
  stage(R0, g0, m0, nd0);
  stage(R1, g1, m1, nd1);
  __syncthreads();
  // ---- blend: one thread per output pixel (3 channels)
  const unsigned char* r0 = R0 + m0;
  const unsigned char* r1 = R1 + m1;
  for (int ox = tid; ox < a.W; ox += 256) {
    const RowCoef rx = yfv2_axis_coef(ox, a.scale_x, a.SW, true);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      OUT[ox * 3 + c] = yfv2_blend(r0[rx.s0 * 3 + c], r0[rx.s1 * 3 + c], r1[rx.s0 * 3 + c], r1[rx.s1 * 3 + c], rx, ry);
  }
  yfv2_emit_row<256>(OUT, a.dst, b, oy, a.H, a.W);
}

// The same resize for a batch of frames of DIFFERENT sizes (yfv2_resize_frames_u8): frame b's descriptor (pointer, size, row
// pitch, the two scales computed on the host exactly as yfv2_resize_u8 computes them) comes from a device table.  One workgroup
// per (frame, output row), the staging scheme of resize_u8_kernel with the same yfv2_axis_coef, so every frame's output is
// bit-identical to yfv2_resize_u8 of that frame alone.  What changes is the guard of the staged dwords: a frame may be a crop
// view (pitch > 3w) starting at any byte, and the bytes around it may belong to no allocation, so a dword is loaded whole only
// when all four of its bytes lie in the frame's own extent [data, data + (h-1) pitch + 3w); any other dword is gathered byte by
// byte from the bytes of it that do (tests/test_frames_host.py models this guard).  LDS is sized for the widest frame.
// The kernel is a template over the descriptor and the epilogue (Row, above) - a template, not a shared function called by two
// kernels: a function boundary alone reorders the uint8 instantiation's blend (profiles/train_batch_isa.txt), and the uint8
// instantiation <ResizeFrame, RowU8> must stay the instruction stream it was.  <TrainFrame, RowTrain> is the training entry point's
// launch: the same staging, guards, coefficients and blend, so its batch is the resize's
// bytes looked up in the frame's table.
// A third pair of instantiations reads a table the DEVICE wrote (second-stage crops, yfv2_crops.hip): descriptors
// Counted<...> with a CountedHead in front of entry 0.  The host does not know how many entries are live, so the grid covers the
// table's capacity and a workgroup whose entry is not live returns here - before the descriptor load and before any barrier, on a
// value every thread of the workgroup reads alike.  For a descriptor without COUNTED the test is no code at all: the four host-table
// instantiations are the instruction streams they were (profiles/crops_isa.txt).
// A fourth pair, over Letterboxed<...> descriptors and RowTensor, writes the crops as a network's input: the row
// and column of the resized view are the output's minus the inner rectangle's origin, the scales are those of the inner size, and
// what lies outside the inner rectangle is fill.  All of it sits behind `if constexpr` on Row::TENSOR: the six other instantiations
// are the instruction streams they were (profiles/crop_tensors_isa.txt).
template <class Frame>
__device__ __forceinline__ bool yfv2_not_live(const Frame* frames, int b) {
  if constexpr (requires { Frame::COUNTED; }) return b >= reinterpret_cast<const CountedHead*>(frames)[-1].live;
  else return false;
}

constexpr int RF_THREADS = 128;   // 2 waves: 12 workgroups (rows) per CU fit the LDS of 1920-wide frames, 8 of 4 waves would
template <class Frame, class Row>
__global__ __launch_bounds__(RF_THREADS, 6) void resize_frames_u8_kernel(const Frame* __restrict__ frames, typename Row::Out* __restrict__ dst, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Row row{dst};
  const int tid = threadIdx.x;
  const int b = blockIdx.x / H, oy = blockIdx.x - b * H;
  if (yfv2_not_live(frames, b)) return;
  const Frame f = frames[b];
  int iy = oy;                                           // the row of the resized view: oy itself, except inside a letterbox
  if constexpr (requires { Row::TENSOR; }) {
    row.begin(frames);
    iy = oy - f.oy0;
    if (iy < 0 || iy >= f.ih) { row.fill_row(b, oy, H, W); return; }   // uniform, in front of every barrier
  }
  const RowCoef ry = yfv2_axis_coef(iy, f.scale_y, f.h, false);
  const int row_bytes = f.w * 3;
  const int slot = yfv2_slot(row_bytes, Row::ALIGN);
  unsigned char* R0 = smem;
  unsigned char* R1 = smem + slot;
  unsigned char* OUT = smem + 2 * slot;
  if constexpr (Row::AUGMENT) row.begin(OUT, f.alpha, f.beta);
  const long long extent = (long long)(f.h - 1) * f.pitch + row_bytes;   // bytes of the frame from f.data on
  const long long g0 = (long long)ry.s0 * f.pitch, g1 = (long long)ry.s1 * f.pitch;
  const uintptr_t base = reinterpret_cast<uintptr_t>(f.data);
  const int m0 = (int)((base + g0) & 3), m1 = (int)((base + g1) & 3);
  const int nd0 = (m0 + row_bytes + 3) >> 2, nd1 = (m1 + row_bytes + 3) >> 2;
  // Both rows' dwords form one index space [0, nd0 + nd1); each thread issues up to STAGE_U loads before it writes any of them
  // to LDS, so a workgroup has its whole staging in flight at once instead of one load round trip per loop iteration.
  const long long first0 = g0 - m0, first1 = g1 - m1;      // offset of each row's dword 0 from f.data (f.data + first is 4-byte aligned)
  const int ntot = nd0 + nd1;
  constexpr int STAGE_U = 16;
  for (int i0 = tid; i0 < ntot; i0 += RF_THREADS * STAGE_U) {
    unsigned v[STAGE_U];
#pragma unroll
    for (int u = 0; u < STAGE_U; ++u) {
      const int i = i0 + RF_THREADS * u;
      v[u] = 0;
      if (i < ntot) {
        const long long lo = i < nd0 ? first0 + 4ll * i : first1 + 4ll * (i - nd0);
        if (lo >= 0 && lo + 4 <= extent) v[u] = *reinterpret_cast<const unsigned*>(f.data + lo);
        else                                          // a dword that straddles an end of the extent: only its bytes inside
          for (int k = 0; k < 4; ++k)
            if (lo + k >= 0 && lo + k < extent) v[u] |= (unsigned)f.data[lo + k] << (8 * k);
      }
    }
#pragma unroll
    for (int u = 0; u < STAGE_U; ++u) {
      const int i = i0 + RF_THREADS * u;
      if (i < ntot) *reinterpret_cast<unsigned*>(i < nd0 ? R0 + 4 * i : R1 + 4 * (i - nd0)) = v[u];
    }
  }
  __syncthreads();
  const unsigned char* r0 = R0 + m0;
  const unsigned char* r1 = R1 + m1;
  for (int ox = tid; ox < W; ox += RF_THREADS) {
    int ix = ox;                                         // the column of the resized view, likewise
    if constexpr (requires { Row::TENSOR; }) {
      ix = ox - f.ox0;
      if (ix < 0 || ix >= f.iw) { row.put_fill(OUT, ox, W); continue; }
    }
    const RowCoef rx = yfv2_axis_coef(ix, f.scale_x, f.w, true);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      row.put(OUT, ox, c, W, yfv2_blend(r0[rx.s0 * 3 + c], r0[rx.s1 * 3 + c], r1[rx.s0 * 3 + c], r1[rx.s1 * 3 + c], rx, ry));
  }
  row.end(OUT, b, oy, H, W);
}

// ---- the same ragged batch from decoder-format frames: YUV 4:2:0 planes read in place (yfv2_resize_frames_yuv) ----
// THE COLOUR FORMULA (the specification; include/yfv2.h states it for callers, tests/yuv_model.py in numpy).  All int32, SHIFT = 20,
// every coefficient rint(k * 2^20); the limited-range rows carry 255/219 in the luma and 255/224 in the chroma coefficients:
//                         off  CY       CVR      CVG      CUG      CUB
//   YFV2_BT601_LIMITED    16   1220542  1673527  -852492  -409993  2116026     OpenCV's COLOR_YUV2BGR_NV12 / _I420 literals
//   YFV2_BT709_LIMITED    16   1220945  1879825  -558796  -223607  2215014     Kr / Kb = 0.2126 / 0.0722
//   YFV2_BT601_FULL       0    1048576  1470104  -748826  -360853  1858077     JPEG; Kr / Kb = 0.299 / 0.114
//   YFV2_BT709_FULL       0    1048576  1651297  -490864  -196424  1945738
//   yy = max(Y - off, 0) * CY;  u = U - 128;  v = V - 128
//   R = clamp((yy + (1 << 19) + CVR * v) >> 20, 0, 255)               (arithmetic shift: floor for negatives)
//   G = clamp((yy + (1 << 19) + CVG * v + CUG * u) >> 20, 0, 255)
//   B = clamp((yy + (1 << 19) + CUB * u) >> 20, 0, 255)               output order B, G, R: the network's channel order
// The accumulators stay below 5.8e8 in magnitude over all 2^24 (Y, U, V) (tests/test_yuv_host.py sweeps them).  Chroma is replicated,
// not interpolated.  OpenCV is not in this image: parity with cv2 proper is unpinned, exactly as for the resize above.
//
// THE 10-BIT COLOUR FORMULA (YFV2_YUV_P010 / _I010; include/yfv2.h states it for callers, tests/yuv_model.py in numpy): the same
// expression on 10-bit codes, the 8-bit B, G, R rounded ONCE from 10-bit precision.  Every literal is rint(k * 2^20) of the real
// coefficient per 10-bit code - limited range: luma 255 / (219 * 4), chroma 255 / (224 * 4) times 2(1-Kr), -2Kr(1-Kr)/Kg,
// -2Kb(1-Kb)/Kg, 2(1-Kb); full range: 255 / 1023 in place of both - computed from those formulas, not OpenCV literals (cv2 has no
// P010 conversion to agree with):
//                         off  CY      CVR     CVG      CUG      CUB
//   YFV2_BT601_LIMITED    64   305236  418389  -213115  -102698  528805
//   YFV2_BT709_LIMITED    64   305236  469956  -139699  -55902   553753
//   YFV2_BT601_FULL       0    261375  366448  -186658  -89949   463157
//   YFV2_BT709_FULL       0    261375  411614  -122356  -48962   485008
//   yy = max(Y - off, 0) * CY;  u = U - 512;  v = V - 512;  R, G, B as above
// The accumulators stay within [-2.83e8, 5.77e8] over the 10-bit cube (tests/test_yuv16_host.py bounds them by the corners).
static const YuvCoef YUV_COEF[2][4] = {   // [sample bytes - 1][colour]
    {{16, 1220542, 1673527, -852492, -409993, 2116026},
     {16, 1220945, 1879825, -558796, -223607, 2215014},
     {0, 1048576, 1470104, -748826, -360853, 1858077},
     {0, 1048576, 1651297, -490864, -196424, 1945738}},
    {{64, 305236, 418389, -213115, -102698, 528805},
     {64, 305236, 469956, -139699, -55902, 553753},
     {0, 261375, 366448, -186658, -89949, 463157},
     {0, 261375, 411614, -122356, -48962, 485008}},
};

// MID: the chroma midpoint, 128 for 8-bit samples and 512 for 10-bit ones.  Every factor fits 24 bits (8 bits: |coefficient| < 2^23,
// |Y - off|, |u|, |v| <= 255; 10 bits: |coefficient| < 2^20, |Y - off| <= 1023, |u|, |v| <= 512) and every product int32, so the
// multiplies are __mul24: full-rate v_mul_i32_i24 / v_mad_i32_i24 where a 32-bit integer multiply runs at a quarter of the rate - the
// same values.
template <int MID>
__device__ __forceinline__ void yfv2_yuv_to_bgr(int Y, int U, int V, const YuvCoef& k, int (&p)[3]) {
  const int yy = __mul24(max(Y - k.off, 0), k.cy) + (1 << 19), u = U - MID, v = V - MID;
  p[0] = min(max((yy + __mul24(k.cub, u)) >> 20, 0), 255);
  p[1] = min(max((yy + __mul24(k.cvg, v) + __mul24(k.cug, u)) >> 20, 0), 255);
  p[2] = min(max((yy + __mul24(k.cvr, v)) >> 20, 0), 255);
}

// The sample width of a YUV descriptor type: 2 for Samples16<...> (yfv2_internal.h), 1 for every other.
template <class Frame>
constexpr int yfv2_sample_bytes() {
  if constexpr (requires { Frame::SAMPLE_BYTES; }) return Frame::SAMPLE_BYTES;
  else return 1;
}
// Whether a YUV descriptor type is of the general 1-byte kind, AnySampling<...> (yfv2_internal.h): any 8-bit format, not 4:2:0 only.
template <class Frame>
constexpr bool yfv2_any_sampling() {
  if constexpr (requires { Frame::ANY_SAMPLING; }) return true;
  else return false;
}
// THE VALUE OF A WORD, the two rules of the 2-byte formats: P010 carries its 10 bits in the high bits (word >> 6; the low 6 are
// ignored), I010 in the low bits (word & 1023; the high 6 are ignored).  shift = 6 / 0 is uniform over a workgroup.
__device__ __forceinline__ int yfv2_sample10(const unsigned short* p, int i, int shift) { return ((int)p[i] >> shift) & 1023; }

// One workgroup per (frame, output row), the scheme of resize_frames_u8_kernel.  Staged in LDS, as aligned dwords with the same
// guard - a dword is loaded whole only when its four bytes lie in the frame's own extent OF THAT PLANE (first row's first needed byte
// to last row's last needed byte), otherwise byte by byte from those that do: luma rows s0 and s1, w bytes each, and the chroma rows
// (s0 + py) >> 1 and (s1 + py) >> 1 - ONCE when the two coincide (every other output row of an up-scale, most rows near 1:1) -
// which are cw = ((w - 1 + px) >> 1) + 1 samples: 2 cw bytes of the interleaved plane, or cw bytes of each of U and V.  That is
// 3 w to 4 w bytes per output row where the B, G, R kernel stages 6 w.  Each output pixel converts its four taps (s0 / s1 x sx0 /
// sx1) to B, G, R and blends them with resize_frames_u8_kernel's expression: convert-then-blend is the only order that is
// bit-identical to converting the frame and resizing it (the clamps and the rounding do not commute with the blend).
// LDS per workgroup: two luma slots of yfv2_slot(w), two chroma rows of two half-slots of yfv2_slot((w >> 1) + 1) each (a half-slot
// holds one I420 plane row at any misalignment, the two together one interleaved row), then the Row's own bytes (RowU8: 3 W).
// Threads and occupancy: a 1920-wide frame takes 2 * 1924 + 4 * 964 + 1056 = 8760 bytes, so 18 workgroups per CU fit the LDS -
// more than the 16 that two-wave workgroups reach under the CU's 32-wave limit, so LDS does not bound this kernel (it bounds the
// B, G, R one at 12-13).  Two waves keep the 352 output pixels' 5.5 waves of blend work at 6 wave-iterations (four waves would run
// 8).  The kernel needs 59 VGPRs, so the launch bound asks for all 8 waves per SIMD = those 16 workgroups: like its neighbour the
// launch is a chain of round trips per workgroup (descriptor, staging loads, barrier, blend, barrier, stores), and what hides them is
// workgroups in flight - measured 258 us at 8 waves per SIMD against 283 us at 6 on the probe's mix.
// Like its neighbour a template over descriptor and epilogue: <ResizeFrameYuv, RowU8> is the resize, <TrainFrameYuv, RowTrain> the
// training batch (43 VGPRs - the fp32 row goes to LDS where the uint8 row went).
// TWO-BYTE SAMPLES (YFV2_YUV_P010 / _I010): the descriptor type Samples16<D> makes SB = 2, and the same body stages
// twice the bytes - two luma slots of yfv2_slot(2 w), four chroma half-slots of yfv2_slot(2 * ((w >> 1) + 1)), then the Row's bytes.
// The dword staging and its guard are unchanged (the planes are 2-byte aligned and the pitches even, so smis is 0 or 2); only the tap
// reads (16-bit LDS reads: a sub-dword LDS read is one instruction whatever its width, so the blend issues what the byte kernel
// issues plus the bit-field extracts) and yfv2_sample10 are new code.  For SB = 1 nothing below differs from what it was
// (profiles/yuv16_isa.txt: the ten existing instantiations' streams, hashed, parent against child).  Same launch bound:
// <Samples16<ResizeFrameYuv>, RowU8> needs 61 VGPRs (the counted twin 61, training 43, the tensors 46 / 44), so 8 waves per SIMD
// still fit the registers, and no instantiation spills to scratch.  By LDS a 1920-wide frame takes 2 * 3844 + 4 * 1928 + 1056 =
// 16456 bytes: 9 workgroups per CU (18 of its 32 waves) where the byte kernel reaches its 16 - at 1080p this kernel is LDS-bound, at
// 1280 wide it has 14, from 640 wide down the 16 of the launch bound again.
// ANY 8-BIT SAMPLING (YFV2_YUV_I422 / _I440 / _I444 / _YUYV / _UYVY / _GREY beside the three 4:2:0 formats): the
// descriptor type AnySampling<D> makes ANY true, and the same body takes the sampling from f.format - the chroma shifts sx, sy
// (pixel (r, c): chroma row (r + py) >> sy, sample (c + px) >> sx; with sy = 0 the two chroma rows coincide exactly when the two luma
// rows do), packed or not, grey or not - all uniform over the workgroup.  What is staged per blended source row: planar and
// interleaved formats the luma row and the chroma row(s) of the format's own width, as above; a PACKED row once, as chroma segment
// a, from the macropixel of pixel 0 to that of pixel w - 1 (4 cw bytes; luma, U and V are then three taps into it, luma at stride
// 2, chroma at stride 4), with no luma segment; GREY the luma row alone, U = V = 128 being one dword the workgroup writes into the
// free U slot and reads at chroma stride 0.  The guard is the one above, per plane; a packed plane's extent runs from the first to
// the last macropixel of the rectangle.  The LDS layout is the general kind's own (FrameRows below): six slots of yfv2_slot(w), about
// 6 bytes per source pixel like the B, G, R kernel.  A 4:2:0 frame in such a launch goes through the same arithmetic on the same
// bytes as in a 4:2:0-only launch: the same bits.  For a descriptor that is not AnySampling<...> every ANY term is a constant
// (sx = sy = 1, packed = grey = false) and the fifteen other instantiations are the instruction streams they were
// (profiles/yuv_any_isa.txt).  Same launch bound: <AnySampling<ResizeFrameYuv>, RowU8> needs 60 VGPRs (the counted twin 59, training
// 42, the tensors 44 / 42), no instantiation uses scratch.  By LDS a 1920-wide frame takes 6 * 1924 + 1056 = 12600 bytes: 13
// workgroups per CU (26 of its 32 waves), the 16 of the launch bound from 1525 wide down.
constexpr int RY_THREADS = 128;
template <class Frame, class Row>
__global__ __launch_bounds__(RY_THREADS, 8) void resize_frames_yuv_kernel(const Frame* __restrict__ frames, typename Row::Out* __restrict__ dst, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Row row{dst};
  const int tid = threadIdx.x;
  const int b = blockIdx.x / H, oy = blockIdx.x - b * H;
  if (yfv2_not_live(frames, b)) return;
  const Frame f = frames[b];
  int iy = oy;
  if constexpr (requires { Row::TENSOR; }) {
    row.begin(frames);
    iy = oy - f.oy0;
    if (iy < 0 || iy >= f.ih) { row.fill_row(b, oy, H, W); return; }
  }
  const RowCoef ry = yfv2_axis_coef(iy, f.scale_y, f.h, false);
  constexpr int SB = yfv2_sample_bytes<Frame>();          // bytes of a sample: everything counted in bytes below carries it
  constexpr bool ANY = yfv2_any_sampling<Frame>();        // the general kind: the sampling comes from f.format, uniform over the workgroup
  const bool packed = ANY && yfv2_yuv_packed(f.format), grey = ANY && yfv2_yuv_grey(f.format);
  const bool planar = ANY ? yfv2_yuv_planar(f.format) : f.format == (SB == 1 ? YFV2_YUV_I420 : YFV2_YUV_I010);
  const int sx = ANY ? yfv2_yuv_shift_x(f.format) : 1, sy = ANY ? yfv2_yuv_shift_y(f.format) : 1;   // pixel (r, c): chroma (r >> sy, c >> sx)
  const int cw = ((f.w - 1 + f.px) >> sx) + 1, ch = ((f.h - 1 + f.py) >> sy) + 1;   // chroma samples per row, chroma rows of the frame
  const int cbytes = grey ? 0 : packed ? 4 * cw : SB * (planar ? cw : 2 * cw);      // (packed: the macropixels of the row, luma and all)
  const int cr0 = (ry.s0 + f.py) >> sy, cr1 = (ry.s1 + f.py) >> sy;
  const bool one_chroma_row = cr0 == cr1;
  // 4:2:0 kinds: [luma 0][luma 1][chroma 0: two half-slots][chroma 1: likewise].  The general kind: six slots of yfv2_slot(w), a group
  // of three per blended row, [luma][U][V] - an interleaved row lies over U and V, a packed row over all three (FrameRows below).
  const int yslot = yfv2_slot(SB * f.w, Row::ALIGN), chalf = ANY ? yslot : yfv2_slot(SB * ((f.w >> 1) + 1), Row::ALIGN);
  unsigned char* LY0 = smem;
  unsigned char* LY1 = smem + (ANY ? 3 : 1) * yslot;
  unsigned char* LC0 = ANY ? smem + (packed ? 0 : yslot) : smem + 2 * yslot;
  unsigned char* LC1 = ANY ? LC0 + 3 * yslot : LC0 + 2 * chalf;
  unsigned char* OUT = ANY ? smem + 6 * yslot : LC0 + 4 * chalf;
  if constexpr (Row::AUGMENT) row.begin(OUT, f.alpha, f.beta);
  const long long extent_y = (long long)(f.h - 1) * f.pitch_y + SB * f.w;
  const long long extent_c = (long long)(ch - 1) * f.pitch_c + cbytes;
  // Six row segments: luma s0, s1; chroma plane a rows cr0, cr1; chroma plane b (I420's V) rows cr0, cr1.  A segment that is not
  // staged (the second chroma row when it is the first, plane b of an interleaved format) has no dwords.  Everything about a segment
  // is wave-uniform, the guard included once it is counted in bytes from the segment's dword 0 (sptr, 4-byte aligned): the bytes
  // [blo, bhi) of that stream lie in the plane's extent, so dword i is loaded whole iff blo <= 4 i and 4 i + 4 <= bhi.
  // A packed plane is staged as the chroma segments a, from the macropixel of pixel 0 (f.ca is its U byte: byte 1 of a YUYV, byte 0
  // of a UYVY macropixel) to that of pixel w - 1; it has no luma segments.  GREY has no chroma segments.
  const int uoff = packed && f.format == YFV2_YUV_YUYV ? 1 : 0;
  const unsigned char* sbase[6] = {f.y, f.y, f.ca - uoff, f.ca - uoff, f.cb, f.cb};
  unsigned char* slds[6] = {LY0, LY1, LC0, LC1, LC0 + chalf, LC1 + chalf};
  const unsigned char* sptr[6];
  int smis[6], snd[6], sblo[6], sbhi[6];
  int maxnd = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const long long g = k < 2 ? (long long)(k == 0 ? ry.s0 : ry.s1) * f.pitch_y : (long long)((k & 1) ? cr1 : cr0) * f.pitch_c;
    const int n = k < 2 ? (packed ? 0 : SB * f.w) : (((k & 1) && one_chroma_row) || (k >= 4 && !planar) ? 0 : cbytes);
    smis[k] = (int)((reinterpret_cast<uintptr_t>(sbase[k]) + g) & 3);
    const long long first = g - smis[k];                  // offset of the segment's dword 0 from its plane's base
    sptr[k] = sbase[k] + first;
    snd[k] = n ? (smis[k] + n + 3) >> 2 : 0;
    sblo[k] = first < 0 ? (int)-first : 0;
    sbhi[k] = (int)min((k < 2 ? extent_y : extent_c) - first, 4ll * snd[k]);
    maxnd = max(maxnd, snd[k]);
  }
  // as resize_frames_u8_kernel: each thread issues its loads - up to STAGE_U per segment, 16 for the four or six segments of a
  // 1920-wide frame, which one trip covers - before it writes any of them to LDS.  Only a segment's first and last dword can
  // straddle an end of the extent (the row itself lies inside it): twelve threads gather those byte by byte, in the same flight.
  constexpr int STAGE_U = 4;
  for (int i0 = tid; i0 < maxnd; i0 += RY_THREADS * STAGE_U) {
    unsigned v[6][STAGE_U];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int u = 0; u < STAGE_U; ++u) {
        const int o = 4 * (i0 + RY_THREADS * u);
        if (o >= sblo[k] && o + 4 <= sbhi[k]) v[k][u] = *reinterpret_cast<const unsigned*>(sptr[k] + o);
      }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int u = 0; u < STAGE_U; ++u) {
        const int o = 4 * (i0 + RY_THREADS * u);
        if (o >= sblo[k] && o + 4 <= sbhi[k]) *reinterpret_cast<unsigned*>(slds[k] + o) = v[k][u];
      }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if ((tid >> 1) == k && snd[k] > 0) {
      const int o = (tid & 1) ? 4 * (snd[k] - 1) : 0;
      if (o < sblo[k] || o + 4 > sbhi[k]) {               // a dword that straddles an end of the plane's extent: only its bytes inside
        unsigned e = 0;
        for (int j = 0; j < 4; ++j)
          if (o + j >= sblo[k] && o + j < sbhi[k]) e |= (unsigned)sptr[k][o + j] << (8 * j);
        *reinterpret_cast<unsigned*>(slds[k] + o) = e;
      }
    }
  if constexpr (ANY)
    if (grey && tid == 0) *reinterpret_cast<unsigned*>(LC0) = 0x80808080u;   // U = V = 128, the one chroma sample of a GREY frame (cstep 0)
  __syncthreads();
  // U and V of chroma sample j of blended row 0 / 1: pu[j * cstep], pv[j * cstep]
  const int cstep = grey ? 0 : packed ? 4 : planar ? 1 : 2;
  const YuvCoef kc = f.coef;
  // Taps: sample s of a staged row is its byte s (1-byte samples) or its 16-bit word s, of which yfv2_sample10 takes the value - a
  // slot is 4-byte aligned and a 2-byte plane's misalignment is 0 or 2, so every word is aligned.  Everything else is one body.
  using Sample = std::conditional_t<SB == 1, unsigned char, unsigned short>;
  const int vshift = planar ? 0 : 6;                       // (2-byte samples only)
  auto at = [&](const unsigned char* lds, int mis) { return reinterpret_cast<const Sample*>(lds + mis); };
  const Sample* a0 = at(LC0, grey ? 0 : smis[2]);
  const Sample* a1 = one_chroma_row ? a0 : at(LC1, smis[3]);
  const Sample* b0 = planar ? at(LC0 + chalf, smis[4]) : a0 + 1;      // (ANY: LC0 + chalf, the V slot of the row's group)
  const Sample* b1 = planar ? (one_chroma_row ? b0 : at(LC1 + chalf, smis[5])) : a1 + 1;
  const bool swapped = SB == 1 && f.format == YFV2_YUV_NV21;
  const Sample* pu0 = swapped ? b0 : a0;
  const Sample* pv0 = swapped ? a0 : b0;
  const Sample* pu1 = swapped ? b1 : a1;
  const Sample* pv1 = swapped ? a1 : b1;
  const Sample* y0 = at(LY0, smis[0]);
  const Sample* y1 = at(LY1, smis[1]);
  if constexpr (ANY) {
    if (packed) {             // a0 / a1: byte 0 of the row's first macropixel.  U at uoff, V two bytes on; luma of pixel s at 2 (s + px) + 1 - uoff
      pu0 = a0 + uoff; pv0 = pu0 + 2; pu1 = a1 + uoff; pv1 = pu1 + 2;
      y0 = a0 + 2 * f.px + 1 - uoff; y1 = a1 + 2 * f.px + 1 - uoff;
    }
    if (grey) { pv0 = pu0; pu1 = pu0; pv1 = pu0; }
  }
  const int ysh = packed ? 1 : 0;                          // luma of pixel s: y[s << ysh]
  auto tap = [&](const Sample* y, const Sample* pu, const Sample* pv, int s, int j, int (&p)[3]) {
    if constexpr (ANY) yfv2_yuv_to_bgr<128>(y[s << ysh], pu[j], pv[j], kc, p);
    else if constexpr (SB == 1) yfv2_yuv_to_bgr<128>(y[s], pu[j], pv[j], kc, p);
    else yfv2_yuv_to_bgr<512>(yfv2_sample10(y, s, vshift), yfv2_sample10(pu, j, vshift), yfv2_sample10(pv, j, vshift), kc, p);
  };
  for (int ox = tid; ox < W; ox += RY_THREADS) {
    int ix = ox;
    if constexpr (requires { Row::TENSOR; }) {
      ix = ox - f.ox0;
      if (ix < 0 || ix >= f.iw) { row.put_fill(OUT, ox, W); continue; }
    }
    const RowCoef rx = yfv2_axis_coef(ix, f.scale_x, f.w, true);
    const int j0 = ANY ? __mul24((rx.s0 + f.px) >> sx, cstep) : ((rx.s0 + f.px) >> 1) * cstep;
    const int j1 = ANY ? __mul24((rx.s1 + f.px) >> sx, cstep) : ((rx.s1 + f.px) >> 1) * cstep;
    int p00[3], p01[3], p10[3], p11[3];      // B, G, R of the taps (row s0 / s1, column sx0 / sx1)
    tap(y0, pu0, pv0, rx.s0, j0, p00);
    tap(y0, pu0, pv0, rx.s1, j1, p01);
    tap(y1, pu1, pv1, rx.s0, j0, p10);
    tap(y1, pu1, pv1, rx.s1, j1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) row.put(OUT, ox, c, W, yfv2_blend(p00[c], p01[c], p10[c], p11[c], rx, ry));
  }
  row.end(OUT, b, oy, H, W);
}

YuvCoef yfv2_yuv_coef(int colour, int sample_bytes) { return YUV_COEF[sample_bytes - 1][colour]; }

// ---- the host side of the row kernels: ONE description per frame kind, used by every launch and every limit -----------------
// FrameRows<Frame> is what the descriptor's frame kind (B, G, R: ResizeFrame and what derives from it; YUV: ResizeFrameYuv likewise)
// decides: the kernel template, its block size, the LDS of a workgroup of <Frame, Row> for a frame w pixels wide - the staging slots
// as the kernel places them (yfv2_slot) and the Row's own bytes - and the widest frame an entry point of that Row admits.
template <class Frame, bool YUV = std::is_base_of_v<ResizeFrameYuv, Frame>>
struct FrameRows {       // B, G, R: two source rows of 3 w bytes
  static constexpr int THREADS = RF_THREADS;
  template <class Row> static constexpr auto& kernel = resize_frames_u8_kernel<Frame, Row>;
  template <class Row> static size_t lds_bytes(int w, int W) { return 2 * (size_t)yfv2_slot(3 * w, Row::ALIGN) + (size_t)Row::lds_bytes(W); }
  // In closed form: a slot is at most 3 w + ALIGN + 2 bytes, so every row up to this fits.  For W % 4 == 0 it lies 1 to 5 pixels below
  // the widest row that fits (27128 against 27129 for RowU8 at W = 352): the figure the entry points' messages and include/yfv2.h name.
  template <class Row> static int max_width(int W) { return (YFV2_LDS_FULL - Row::lds_bytes(W)) / 6 - (Row::ALIGN + 2) / 3; }
};
template <class Frame>
struct FrameRows<Frame, true> {   // YUV: two luma slots, two chroma rows of two half-slots each, of SB-byte samples
  static constexpr int THREADS = RY_THREADS;
  static constexpr int SB = yfv2_sample_bytes<Frame>();
  static constexpr bool ANY = yfv2_any_sampling<Frame>();
  static constexpr int PER_PIXEL = ANY ? 6 : 4 * SB;      // staged bytes per source pixel, about
  template <class Row> static constexpr auto& kernel = resize_frames_yuv_kernel<Frame, Row>;
  // The general kind (AnySampling<...>): SIX slots of yfv2_slot(w), a group of three per blended row - [luma][U][V], each a full-width
  // row of a 4:4:4 frame at any misalignment; an interleaved chroma row (at most w + 2 bytes) lies over U and V, a packed row (the
  // macropixels of the row, at most 2 w + 4 bytes, at any misalignment at most 2 w + 8 staged) over all three: 3 (w + 3) >= 2 w + 8.
  template <class Row> static size_t lds_bytes(int w, int W) {
    if constexpr (ANY) return 6 * (size_t)yfv2_slot(w, Row::ALIGN) + (size_t)Row::lds_bytes(W);
    else return 2 * (size_t)yfv2_slot(SB * w, Row::ALIGN) + 4 * (size_t)yfv2_slot(SB * ((w >> 1) + 1), Row::ALIGN) + (size_t)Row::lds_bytes(W);
  }
  // The exact maximum: the function above grows by about PER_PIXEL bytes per pixel and never falls, so the answer is next to
  // (YFV2_LDS_FULL - the Row's bytes) / PER_PIXEL and two short walks find it.
  template <class Row> static int max_width(int W) {
    int w = (int)std::max<long long>(1, ((long long)YFV2_LDS_FULL - Row::lds_bytes(W)) / PER_PIXEL);
    while (w > 1 && lds_bytes<Row>(w, W) > (size_t)YFV2_LDS_FULL) --w;
    while (lds_bytes<Row>(w + 1, W) <= (size_t)YFV2_LDS_FULL) ++w;
    return w;
  }
};

// The launch of every kind: one workgroup per (entry, output row) - n = the batch, or a counted table's capacity (the host does not
// know how many entries are live) - and LDS for the widest FRAME of the call (an upper bound of every crop of it).
template <class Frame, class Row>
static void launch_rows(const void* table, int n, int max_w, void* dst, int H, int W, hipStream_t s) {
  using F = FrameRows<Frame>;
  YFV2_LAUNCH_LDS(yfv2_device(), (F::template kernel<Row>), YFV2_LDS_FULL, dim3((unsigned)(n * H)), dim3(F::THREADS), F::template lds_bytes<Row>(max_w, W), s,
                  static_cast<const Frame*>(table), static_cast<typename Row::Out*>(dst), H, W);
}

// What the other units see of the family: a row kind, a frame kind, three functions.  THE TABLE of the twenty instantiations: f is
// called as f.operator()<Frame, Row>().  (The device compiler emits the kernels in the order they are named here - training first,
// the tensors by frame kind, within a row kind B, G, R, then 1-byte 4:2:0, then 2-byte, then general 1-byte YUV.)
template <class Fn>
static auto with_rows(Yfv2RowKind kind, Yfv2FrameKind frames, Fn f) {
  using U8 = RowU8<RF_THREADS>;                 using U8Y = RowU8<RY_THREADS>;
  using Train = RowTrain<RF_THREADS>;           using TrainY = RowTrain<RY_THREADS>;
  using F32 = RowTensor<RF_THREADS, false>;     using F32Y = RowTensor<RY_THREADS, false>;
  using F16 = RowTensor<RF_THREADS, true>;      using F16Y = RowTensor<RY_THREADS, true>;
  const bool half = kind == YFV2_ROWS_TENSOR_F16;
  // one row kind: its B, G, R descriptor and Row, its YUV descriptor (1-byte 4:2:0; Samples16<...> of it for 2-byte samples,
  // AnySampling<...> of it for the general 1-byte kind) and Row
  auto pick = [&]<class Bgr, class RowBgr, class Yuv, class RowYuv>() {
    if (frames == YFV2_FRAMES_BGR) return f.template operator()<Bgr, RowBgr>();
    if (frames == YFV2_FRAMES_YUV8) return f.template operator()<Yuv, RowYuv>();
    if (frames == YFV2_FRAMES_YUV16) return f.template operator()<Samples16<Yuv>, RowYuv>();
    return f.template operator()<AnySampling<Yuv>, RowYuv>();
  };
  switch (kind) {
    case YFV2_ROWS_TRAIN:      return pick.template operator()<TrainFrame, Train, TrainFrameYuv, TrainY>();
    case YFV2_ROWS_U8:         return pick.template operator()<ResizeFrame, U8, ResizeFrameYuv, U8Y>();
    case YFV2_ROWS_COUNTED_U8: return pick.template operator()<CropFrame, U8, CropFrameYuv, U8Y>();
    default:                   // YFV2_ROWS_TENSOR_F32, YFV2_ROWS_TENSOR_F16
      return half ? pick.template operator()<TensorFrame, F16, TensorFrameYuv, F16Y>() : pick.template operator()<TensorFrame, F32, TensorFrameYuv, F32Y>();
  }
}

size_t yfv2_rows_lds_bytes(Yfv2RowKind kind, Yfv2FrameKind frames, int w, int W) {
  return with_rows(kind, frames, [&]<class Frame, class Row>() { return FrameRows<Frame>::template lds_bytes<Row>(w, W); });
}

int yfv2_rows_max_width(Yfv2RowKind kind, Yfv2FrameKind frames, int W) {
  return with_rows(kind, frames, [&]<class Frame, class Row>() { return FrameRows<Frame>::template max_width<Row>(W); });
}

void yfv2_launch_rows(Yfv2RowKind kind, Yfv2FrameKind frames, const void* table, int n, int max_w, void* dst, int H, int W, hipStream_t s) {
  with_rows(kind, frames, [&]<class Frame, class Row>() { launch_rows<Frame, Row>(table, n, max_w, dst, H, W, s); });
}

void yfv2_launch_resize(const ResizeArgs& a, hipStream_t s) {
  YFV2_LAUNCH_LDS(yfv2_device(), resize_u8_kernel, YFV2_LDS_FULL, dim3((unsigned)(a.B * a.H)), dim3(256), yfv2_rows_lds_bytes(YFV2_ROWS_U8, YFV2_FRAMES_BGR, a.SW, a.W), s, a);
}
