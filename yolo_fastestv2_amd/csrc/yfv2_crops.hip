// yfv2_crops.hip - second-stage crops: detection rows -> the descriptor table the resize kernels read, on the
// device, so the host never learns how many boxes there are.  THE RULE is yfv2_crop_row_rect (yfv2_internal.h; include/yfv2.h states it
// for callers, tests/crops_model.py in Python); this unit is the selection and the numbering around it:
//   candidates of frame b   rows r < min(max(count[b], 0), R) whose class passes the mask
//   skipped                 a candidate without a rectangle; counted per frame, takes no slot
//   selected                the first max_per_frame candidates with a rectangle, in row order: n_b of them
//   crop k = offset[b] + j  the j-th selected row of frame b, offset = the exclusive prefix sum of n_b; written iff k < cap
// Two launches of one kernel template, one workgroup per frame.  COUNT walks the frame's rows in chunks of the workgroup, ranks the
// selected rows of a chunk by ballot + population count (in row order, whatever the geometry) and leaves n_b and the skipped
// count.  WRITE adds up n_i over the frames in front of it (integers: any order gives the sum), walks its rows again - the rule is
// a handful of fp64 operations per row, cheaper than carrying its result through memory - and writes src, rect and the crop's
// descriptor at slot k.  Workgroup 0 also writes offset[B] and the table head's live count min(total, cap), which is what the resize
// launch's workgroups test.  Every output is an integer or a double the rule defines; nothing is accumulated where order could show.
// The same two launches serve yfv2_crop_tensors_*  through two more kinds, whose descriptor carries the letterbox's
// inner rectangle; COUNT and WRITE are what they are for the crops.
// Built with -ffp-contract=off like every unit whose doubles must round as written (the rule carries its own pragma as well).
#include "../../include/yfv2.h"
#include "yfv2_device.h"

constexpr int CP_THREADS = 256;

// ---- the two kinds: the crop (X0, Y0, cw, ch) of frame f as a descriptor of its own, resized to (H, W)
struct CropBgr {
  using Frame = ResizeFrame;
  using Out = CropFrame;
  using Args = CropPlanArgs;
  static __device__ __forceinline__ void crop(const Frame& f, const int (&rc)[4], int H, int W, Out& o) {
    o.data = f.data + (long long)rc[1] * f.pitch + 3ll * rc[0];
    o.pitch = f.pitch;
    o.h = rc[3]; o.w = rc[2];
    o.scale_x = yfv2_resize_scale(W, rc[2]); o.scale_y = yfv2_resize_scale(H, rc[3]);
    o.box_x = (double)rc[2] / (double)W; o.box_y = (double)rc[3] / (double)H;
  }
};
struct CropYuv {
  using Frame = ResizeFrameYuv;
  using Out = CropFrameYuv;
  using Args = CropPlanArgs;
  static __device__ __forceinline__ void crop(const Frame& f, const int (&rc)[4], int H, int W, Out& o) {
    static_cast<Frame&>(o) = f;
    yfv2_yuv_move(o, rc[0], rc[1]);
    o.h = rc[3]; o.w = rc[2];
    o.scale_x = yfv2_resize_scale(W, rc[2]); o.scale_y = yfv2_resize_scale(H, rc[3]);
  }
};
// ... and the two of the tensor launches (yfv2_crop_tensors_u8 / _yuv): the same view, resized to the INNER size
// yfv2_crop_letterbox_inner gives it - (H, W) itself without letterbox - which the descriptor carries behind the crop's fields.
// TENSOR: the write launch's workgroup 0 also leaves the call's constants in front of the table's head, where RowTensor reads them.
template <class Base, class Desc>
struct TensorKind {
  using Frame = typename Base::Frame;
  using Out = Desc;
  using Args = CropTensorPlanArgs;
  static constexpr bool TENSOR = true;
  static __device__ __forceinline__ void crop(const Frame& f, const int (&rc)[4], const Args& a, Out& o) {
    int in[4];
    yfv2_crop_letterbox_inner(rc[2], rc[3], a.out_h, a.out_w, a.letterbox, in);
    typename Base::Out view;
    Base::crop(f, rc, in[3], in[2], view);
    static_cast<typename Base::Out&>(o) = view;
    o.ox0 = in[0]; o.oy0 = in[1]; o.iw = in[2]; o.ih = in[3];
  }
};
using TensorBgr = TensorKind<CropBgr, TensorFrame>;
using TensorYuv = TensorKind<CropYuv, TensorFrameYuv>;

// a row passes iff its class column is a finite integer in 0..254 whose bit is set
__device__ __forceinline__ bool crop_class_passes(float c, const uint32_t (&mask)[8]) {
  if (!(c >= 0.f && c <= 254.f)) return false;          // NaN fails both
  const int ci = (int)c;
  return (float)ci == c && ((mask[ci >> 5] >> (ci & 31)) & 1u) != 0;
}

template <class Kind, bool WRITE>
__global__ __launch_bounds__(CP_THREADS) void crop_plan_kernel(typename Kind::Args a, const typename Kind::Frame* __restrict__ frames, typename Kind::Out* __restrict__ table) {
  constexpr int WAVES = CP_THREADS / 64;
  __shared__ int s_sel[WAVES], s_skip[WAVES], s_sum[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const typename Kind::Frame f = frames[b];
  const int n = min(max(a.count[b], 0), a.R);
  int first = 0, total = 0;                               // WRITE: offset[b] and offset[B]
  if constexpr (WRITE) {
    if (tid < 2) s_sum[tid] = 0;
    __syncthreads();
    int pre = 0, all = 0;
    for (int i = tid; i < a.B; i += CP_THREADS) {
      const int v = a.n_sel[i];
      all += v;
      if (i < b) pre += v;
    }
    pre = wave_fold(pre); all = wave_fold(all);
    if (lane == 0) { atomicAdd(&s_sum[0], pre); atomicAdd(&s_sum[1], all); }   // integer sums: the order cannot show
    __syncthreads();
    first = s_sum[0]; total = s_sum[1];
  }
  int taken = 0, skipped = 0;                             // of the chunks walked so far; uniform over the workgroup
  for (int r0 = 0; r0 < n; r0 += CP_THREADS) {            // n is uniform: every thread reaches every barrier
    const int r = r0 + tid;
    bool ok = false, skip = false;
    int rc[4] = {0, 0, 0, 0};
    if (r < n) {
      const float* row = a.dets + ((size_t)b * a.R + r) * 6;
      if (crop_class_passes(row[5], a.classes)) {
        const float box[4] = {row[0], row[1], row[2], row[3]};
        ok = yfv2_crop_row_rect(box, f.h, f.w, a.pad_x, a.pad_y, rc);
        skip = !ok;
      }
    }
    const unsigned long long m_ok = __ballot(ok), m_skip = __ballot(skip);
    if (lane == 0) { s_sel[wave] = __popcll(m_ok); s_skip[wave] = __popcll(m_skip); }
    __syncthreads();
    int before = 0, chunk = 0, chunk_skip = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) before += s_sel[w];
      chunk += s_sel[w]; chunk_skip += s_skip[w];
    }
    if constexpr (WRITE) {
      const int j = taken + before + __popcll(m_ok & ((1ull << lane) - 1ull));   // rank among the frame's rows with a rectangle
      const long long k = (long long)first + j;
      if (ok && j < a.max_per_frame && k < a.cap) {
        a.src[k] = b * a.R + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) a.rect[4 * k + i] = rc[i];
        typename Kind::Out o;
        if constexpr (requires { Kind::TENSOR; }) Kind::crop(f, rc, a, o);
        else Kind::crop(f, rc, a.out_h, a.out_w, o);
        table[k] = o;
      }
    }
    taken += chunk; skipped += chunk_skip;
    __syncthreads();                                      // s_sel / s_skip are rewritten by the next chunk
  }
  if (tid == 0) {
    if constexpr (WRITE) {
      a.offset[b] = first;
      if (b == 0) { a.offset[a.B] = total; a.head->live = min(total, a.cap); }
      if constexpr (requires { Kind::TENSOR; })
        if (b == 0) reinterpret_cast<CropTensorHead*>(a.head + 1)[-1].p = a.p;
    } else {
      a.n_sel[b] = min(taken, a.max_per_frame);
      if (a.skipped) a.skipped[b] = skipped;
    }
  }
}

template <class Kind>
static void launch_crop_plan(const typename Kind::Args& a, const void* frames, void* table, hipStream_t s) {
  const auto* f = static_cast<const typename Kind::Frame*>(frames);
  auto* t = static_cast<typename Kind::Out*>(table);
  YFV2_LAUNCH((crop_plan_kernel<Kind, false>), dim3((unsigned)a.B), dim3(CP_THREADS), 0, s, a, f, t);
  YFV2_LAUNCH((crop_plan_kernel<Kind, true>), dim3((unsigned)a.B), dim3(CP_THREADS), 0, s, a, f, t);
}

// the crop kinds take a's CropPlanArgs part: their kernels' arguments are what they were
void yfv2_launch_crop_plan(const CropTensorPlanArgs& a, bool tensor, bool yuv, const void* frames, void* table, hipStream_t s) {
  if (!tensor) !yuv ? launch_crop_plan<CropBgr>(a, frames, table, s) : launch_crop_plan<CropYuv>(a, frames, table, s);
  else !yuv ? launch_crop_plan<TensorBgr>(a, frames, table, s) : launch_crop_plan<TensorYuv>(a, frames, table, s);
}
