// yfv2_anchors.hip - anchor k-means (the reference's genanchors.py:67-102 kmeans with IOU :17-32 and avg_IOU :34-40) as two
// short launches per pass, all arithmetic float64.  Built with -ffp-contract=off: every product, sum and quotient rounds on its
// own, as numpy's scalar float64 operations do - the assignment is an argmin, so a fused multiply-add could move a point.
//
// DETERMINISM RULE.  Every output bit is a function of (X, initial centroids, k) only.  Points are cut into fixed chunks of
// YFV2_KM_CH = 1024 (a compile-time constant - not the grid, not the CU count); every floating-point sum is taken by ONE
// tree, whose shape depends only on the position of a value in its list:
//     list v[0 .. n), padded with +0.0 to a multiple of 256
//     lane value  t (0..255):  ((v[t] + v[t + 256]) + v[t + 512]) + ...           ascending, sequential
//     wave value  w (0..3):    the 64 lane values 64 w .. 64 w + 63 folded in halves: a[l] += a[l + 32], then + 16, 8, 4, 2, 1
//     result:                  ((wave 0 + wave 1) + wave 2) + wave 3
// The assign launch applies it to the 1024 values of a chunk (a point that is not assigned to the cluster, or lies beyond N,
// contributes +0.0, which changes no bit of a non-negative sum); the finalise launch applies it to the list of chunk partials
// in chunk order.  No floating-point atomic anywhere; counts are integers.  tests/anchors_model.py is the numpy
// restatement of this tree that the GPU results are compared with bit for bit.
#include <float.h>

#include "yfv2_device.h"

namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_PER = YFV2_KM_CH / KM_THREADS;   // points per lane
constexpr int KM_MAXK = YFV2_KM_MAXK;

typedef double f64x2u __attribute__((ext_vector_type(2), aligned(8)));   // a (w, h) pair at any 8-byte address: one 16-byte load

// (the fold of 64 lane values described above is wave_fold, yfv2_device.h)

// 1 - IoU of two boxes that share a corner, evaluated through the reference's four cases in its order of tests, each with its
// own formula (genanchors.py:23-30): the box inside the centroid, the two ways of crossing, the centroid inside the box.
// Returns the similarity; the caller forms 1 - s.
__device__ __forceinline__ double km_similarity(double w, double h, double cw, double ch) {
  if (cw >= w && ch >= h) return w * h / (cw * ch);
  if (cw >= w && ch <= h) return w * ch / (w * h + (cw - w) * ch);
  if (cw <= w && ch >= h) return cw * h / (w * h + cw * (ch - h));
  return (cw * ch) / (w * h);
}

// ---- pass, first launch: assign every point of a chunk, write the chunk's partial sums
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(KmArgs a, int first) {
  if (*a.done != 0) return;   // wave-uniform: an earlier pass of this group has ended the loop
  __shared__ double s_c[2 * KM_MAXK];
  __shared__ double s_sum[2 * KM_MAXK + 1][4];
  __shared__ int s_cnt[KM_MAXK][4];
  __shared__ int s_flag[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k;
  if (tid < 2 * k) s_c[tid] = a.centroids[tid];
  __syncthreads();

  const int64_t base = (int64_t)blockIdx.x * YFV2_KM_CH + tid;
  double w[KM_PER], h[KM_PER], best_s[KM_PER];
  int asg[KM_PER];
  int flags = 0;
#pragma unroll
  for (int i = 0; i < KM_PER; ++i) {
    const int64_t p = base + (int64_t)i * KM_THREADS;
    w[i] = 0.0; h[i] = 0.0; best_s[i] = 0.0; asg[i] = -1;
    if (p < a.N) {
      const f64x2u x = *reinterpret_cast<const f64x2u*>(a.wh + 2 * p);
      w[i] = x[0]; h[i] = x[1];
      int best = 0;
      double best_d = 0.0, max_s = 0.0;
      for (int j = 0; j < k; ++j) {
        const double s = km_similarity(w[i], h[i], s_c[2 * j], s_c[2 * j + 1]);
        const double d = 1.0 - s;
        if (j == 0 || d < best_d) { best_d = d; best = j; }   // the first minimum (np.argmin)
        if (j == 0 || s > max_s) max_s = s;                   // max(IOU(...)) of avg_IOU
      }
      const int prev = first ? -1 : a.assign[p];
      if (prev != best) flags |= 1;
      a.assign[p] = best;
      if (first && !(w[i] > 0.0 && w[i] <= DBL_MAX && h[i] > 0.0 && h[i] <= DBL_MAX)) flags |= 2;
      asg[i] = best; best_s[i] = max_s;
    }
  }
  {
    double v = best_s[0];
#pragma unroll
    for (int i = 1; i < KM_PER; ++i) v += best_s[i];
    v = wave_fold(v);
    if (lane == 0) s_sum[2 * k][wave] = v;
  }
  for (int j = 0; j < k; ++j) {
    double sw = asg[0] == j ? w[0] : 0.0, sh = asg[0] == j ? h[0] : 0.0;
    int cnt = __popcll(__ballot(asg[0] == j));
#pragma unroll
    for (int i = 1; i < KM_PER; ++i) {
      sw += asg[i] == j ? w[i] : 0.0;
      sh += asg[i] == j ? h[i] : 0.0;
      cnt += __popcll(__ballot(asg[i] == j));
    }
    sw = wave_fold(sw);
    sh = wave_fold(sh);
    if (lane == 0) { s_sum[j][wave] = sw; s_sum[k + j][wave] = sh; s_cnt[j][wave] = cnt; }
  }
  {
    const int any = (__ballot(flags & 1) != 0 ? 1 : 0) | (__ballot(flags & 2) != 0 ? 2 : 0);
    if (lane == 0) s_flag[wave] = any;
  }
  __syncthreads();
  const int64_t nch = a.nchunks, c = blockIdx.x;
  if (tid < 2 * k + 1) a.part_sum[(int64_t)tid * nch + c] = ((s_sum[tid][0] + s_sum[tid][1]) + s_sum[tid][2]) + s_sum[tid][3];
  if (tid < k) a.part_cnt[(int64_t)tid * nch + c] = s_cnt[tid][0] + s_cnt[tid][1] + s_cnt[tid][2] + s_cnt[tid][3];
  if (tid == 0) a.part_flag[c] = s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3];
}

// ---- pass, second launch (one workgroup): add the chunk partials, decide, update the centroids or end the loop
__global__ __launch_bounds__(KM_THREADS) void km_final_kernel(KmArgs a, int pass, int last) {
  if (*a.done != 0) return;
  __shared__ double s_sum[2 * KM_MAXK + 1][4];
  __shared__ long long s_int[KM_MAXK + 2][4];   // counts of the k clusters, chunks with a changed point, chunks with bad input
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k;
  const int64_t nch = a.nchunks;
  for (int q = 0; q < 2 * k + 1; ++q) {
    const double* src = a.part_sum + (int64_t)q * nch;
    double v = 0.0;
    for (int64_t c = tid; c < nch; c += KM_THREADS) v += src[c];
    v = wave_fold(v);
    if (lane == 0) s_sum[q][wave] = v;
  }
  for (int q = 0; q < k + 2; ++q) {
    long long v = 0;
    if (q < k) {
      const int* src = a.part_cnt + (int64_t)q * nch;
      for (int64_t c = tid; c < nch; c += KM_THREADS) v += src[c];
    } else {
      const int bit = q == k ? 1 : 2;
      for (int64_t c = tid; c < nch; c += KM_THREADS) v += (a.part_flag[c] & bit) ? 1 : 0;
    }
    v = wave_fold(v);
    if (lane == 0) s_int[q][wave] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  auto total = [&](int q) { return ((s_sum[q][0] + s_sum[q][1]) + s_sum[q][2]) + s_sum[q][3]; };
  auto count = [&](int q) { return s_int[q][0] + s_int[q][1] + s_int[q][2] + s_int[q][3]; };
  const bool changed = count(k) != 0, bad = count(k + 1) != 0;
  *a.avg_iou = total(2 * k) / (double)a.N;   // of the centroids this pass assigned with: the ones returned if the loop ends here
  int empty = -1;
  for (int j = k - 1; j >= 0; --j)
    if (count(j) == 0) empty = j;
  const bool converged = !bad && !changed;
  if (bad || converged || empty >= 0 || last) {
    // the loop ends with this pass; the centroids stay what this pass read.  The word lives in host-mapped, coherent memory
    // (as the range guard's does): plain stores, read by the host after it has waited for the stream
    volatile int32_t* hw = a.host_word;
    hw[1] = pass + 1;
    hw[2] = converged ? 1 : 0;
    hw[3] = (bad || converged) ? -1 : empty;
    hw[4] = bad ? 1 : 0;
    hw[0] = 1;
    *a.done = 1;
    return;
  }
  for (int j = 0; j < k; ++j) {
    const double n = (double)count(j);
    a.centroids[2 * j] = total(j) / n;
    a.centroids[2 * j + 1] = total(k + j) / n;
  }
}

}  // namespace

void yfv2_launch_km_pass(const KmArgs& a, int pass, int last, hipStream_t s) {
  hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)a.nchunks), dim3(KM_THREADS), 0, s, a, pass == 0 ? 1 : 0);
  hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(KM_THREADS), 0, s, a, pass, last);
}
