// yfv2_tiles.hip - the last step of tiled detection (yfv2_merge_tiles / yfv2_detect_tiled_u8): the detections
// of a frame's tiles are moved into the frame, put into ONE conf-descending order and walked greedily.  Built with FP
// contraction off, like yfv2_post.hip: every fp32 operation below rounds on its own, as the numpy model of the rule does
// (tests/tiles_ref.py merge_model).
//
// The rule (include/yfv2.h states it for callers):
//   candidates of frame f   its tiles k0 <= k < k1 in ascending k, rows r < tile_count[k] of tile k; x += fp32(x0), y += fp32(y0)
//   order                   conf descending, stable over (k, r)
//   greedy walk             a candidate is dropped if an already kept one has an equal class float and a match with it whose
//                           double value is > thres; match = IoU (metric 0) or inter / min(area) (metric 1) in fp32, computed
//                           as torchvision's kernel computes IoU; a NaN match suppresses nothing; stop after max_out kept
//
// Two launches, no sort:
//   tile_rank_kernel    one workgroup per tile, one thread per row.  Every tile's rows already are conf-descending (what
//                       yfv2_detect writes), so a candidate's position in its frame's order is r + the sum over the frame's
//                       OTHER tiles of a binary search into that tile's conf list (<= 9 steps): ">= conf" in earlier tiles,
//                       "> conf" in later ones - exactly the stable order.  The conf lists of RK_STAGE tiles at a time are
//                       staged in LDS, so the searches are LDS reads with independent chains.  The thread then writes its
//                       candidate (box in frame coordinates, conf, class, origin, area) to that position of the ordered list
//                       in the handle's workspace: positions of a frame are a permutation, nothing is accumulated, nothing
//                       depends on which workgroup runs first.
//   tile_merge_kernel   one workgroup per frame walks the ordered list 64 candidates at a time, the way nms_kernel does:
//                       (a) 16 waves test the chunk's members against the kept set (wave q takes kept entries q, q + 16, ..;
//                       the kept boxes live in LDS and every read of them is a broadcast), (b) the same waves build per
//                       member the mask of EARLIER chunk members that match it, (c) wave 0 solves "kept = alive and no kept
//                       earlier member matches" by iterating ballots, appends the kept members to the LDS set and writes
//                       their output rows.  The next chunk's 64 records are loaded by wave 1 while the tests run.
//                       Up to 4096 kept boxes (6 floats each) = 96 KB of LDS.
// Rows that break the precondition (a tile whose confs are not descending, or not numbers) cannot address anything outside
// the workspace: every position stays below the frame's candidate count; the order is then simply not the stable sort.
#include <hip/hip_runtime.h>

#include "yfv2_device.h"

namespace {

constexpr int TILE_ROWS = 300;          // YFV2_MAX_DET: rows per tile in tile_dets / the tile workspace
constexpr int RK_THREADS = 320;         // 5 waves: thread r < 300 owns row r of the workgroup's tile
constexpr int RK_STAGE = 16;            // conf lists staged per round: 16 x 300 x 4 B = 19 KB of LDS

__device__ __forceinline__ int clamp_count(int c) { return c < 0 ? 0 : (c > TILE_ROWS ? TILE_ROWS : c); }

__global__ __launch_bounds__(RK_THREADS) void tile_rank_kernel(TileMergeArgs a) {
  __shared__ float sconf[RK_STAGE][TILE_ROWS];
  __shared__ int scount[RK_STAGE];
  const int k = (int)blockIdx.x, r = (int)threadIdx.x;
  const int x0 = a.table[4 * k + 0], y0 = a.table[4 * k + 1], k0 = a.table[4 * k + 2], k1 = a.table[4 * k + 3];
  const int nk = clamp_count(a.tile_count[k]);
  const bool live = r < nk;
  const float* row = a.tile_dets + ((size_t)k * TILE_ROWS + (size_t)(live ? r : 0)) * 6;
  const float conf = live ? row[4] : 0.0f;
  int pos = 0;
  for (int kb = k0; kb < k1; kb += RK_STAGE) {
    __syncthreads();                                       // the previous round's searches are done
    const int ns = min(RK_STAGE, k1 - kb);
    if (r < ns) scount[r] = clamp_count(a.tile_count[kb + r]);
    for (int t = 0; t < ns; ++t) {
      const int n = clamp_count(a.tile_count[kb + t]);     // (one address for the whole workgroup)
      if (r < n) sconf[t][r] = a.tile_dets[((size_t)(kb + t) * TILE_ROWS + r) * 6 + 4];
    }
    __syncthreads();
    if (live) {
      for (int t = 0; t < ns; ++t) {
        const int kk = kb + t;
        if (kk == k) { pos += r; continue; }               // its own tile: the rows before it
        const bool earlier = kk < k;                        // ties: a tile with a lower index comes first
        int lo = 0, len = scount[t];
        while (len > 0) {                                   // number of rows of tile kk that precede (conf, k, r)
          const int half = len >> 1;
          const float c = sconf[t][lo + half];
          const bool before = earlier ? c >= conf : c > conf;
          lo = before ? lo + half + 1 : lo;
          len = before ? len - half - 1 : half;
        }
        pos += lo;
      }
    }
  }
  if (!live) return;
  const float fx = (float)x0, fy = (float)y0;
  const float x1 = __fadd_rn(row[0], fx), y1 = __fadd_rn(row[1], fy), x2 = __fadd_rn(row[2], fx), y2 = __fadd_rn(row[3], fy);
  const float area = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
  const size_t o = (size_t)k0 * TILE_ROWS + (size_t)pos;   // pos < the frame's candidate count <= (k1 - k0) * 300
  reinterpret_cast<float4*>(a.geo)[o] = make_float4(x1, y1, x2, y2);
  reinterpret_cast<float4*>(a.meta)[o] = make_float4(conf, row[5], __int_as_float(k * TILE_ROWS + r), area);
}

constexpr int MG_THREADS = 1024;        // 16 waves, as nms_kernel: one workgroup per frame is latency-bound
constexpr int MG_NQ = MG_THREADS / 64;
constexpr int MG_PER = 64 / MG_NQ;      // earlier chunk members examined by one wave
constexpr int MG_MAX_OUT = 4096;        // the API's bound on max_out: 6 floats per kept row in LDS

__global__ __launch_bounds__(MG_THREADS) void tile_merge_kernel(TileMergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kept[];   // [6][max_out]: x1, y1, x2, y2, area, class of the kept boxes
  __shared__ float4 cgeo[2][64], cmeta[2][64];                   // the chunk being walked / the next one
  __shared__ unsigned long long pmask[MG_NQ][64];
  __shared__ unsigned char supp[64];
  __shared__ int n_total, n_keep;
  const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int M = a.max_out;
  float* const kx1 = kept; float* const ky1 = kx1 + M; float* const kx2 = ky1 + M; float* const ky2 = kx2 + M;
  float* const kar = ky2 + M; float* const kcl = kar + M;
  const int k0 = a.table[4 * a.T + 2 * f], k1 = a.table[4 * a.T + 2 * f + 1];
  if (tid == 0) { n_total = 0; n_keep = 0; }
  if (tid < 64) supp[tid] = 0;
  __syncthreads();
  int part = 0;
  for (int k = k0 + tid; k < k1; k += MG_THREADS) part += clamp_count(a.tile_count[k]);
  if (part) atomicAdd(&n_total, part);                           // (an integer sum: the same in any order)
  __syncthreads();
  const int n = n_total;
  const float4* const geo = reinterpret_cast<const float4*>(a.geo) + (size_t)k0 * TILE_ROWS;
  const float4* const meta = reinterpret_cast<const float4*>(a.meta) + (size_t)k0 * TILE_ROWS;
  if (tid < 64 && tid < n) { cgeo[0][tid] = geo[tid]; cmeta[0][tid] = meta[tid]; }
  __syncthreads();

  const double thr = a.thres;
  const bool thr_nonneg = thr >= 0.0;
  const int metric = a.metric;
  // (x1, y1, x2, y2, area) of an earlier box against candidate (g, area_j); classes were compared by the caller.  Boxes whose x
  // intervals do not meet have w = 0, inter = 0 and a match of 0 or NaN: not above any threshold >= 0, decided after two reads.
  auto match_above = [&](float ix1, float iy1, float ix2, float iy2, float iarea, const float4& g, float jarea) -> bool {
    const float xx1 = fmaxf(ix1, g.x), xx2 = fminf(ix2, g.z);
    if (thr_nonneg && !(xx2 > xx1)) return false;
    const float yy1 = fmaxf(iy1, g.y), yy2 = fminf(iy2, g.w);
    const float w = fmaxf(0.0f, __fsub_rn(xx2, xx1)), h = fmaxf(0.0f, __fsub_rn(yy2, yy1));
    const float inter = __fmul_rn(w, h);
    const float den = metric == 0 ? __fsub_rn(__fadd_rn(iarea, jarea), inter) : fminf(iarea, jarea);
    return (double)__fdiv_rn(inter, den) > thr;
  };

  const int j = tid & 63, q = tid >> 6;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int nk = n_keep;                                       // stable: written only between the barriers below
    if (nk >= M) break;
    const int buf = (c0 >> 6) & 1;
    const int m = min(64, n - c0);
    float4 ng = make_float4(0.f, 0.f, 0.f, 0.f), nm = ng;        // wave 1: the next chunk's records, in flight during the tests
    const bool fetch = q == 1 && c0 + 64 + j < n;
    if (fetch) { ng = geo[c0 + 64 + j]; nm = meta[c0 + 64 + j]; }
    unsigned long long bits = 0ull;
    if (j < m) {
      const float4 g = cgeo[buf][j], mt = cmeta[buf][j];
      const float cls = mt.y, area = mt.w;
      for (int kk = q; kk < nk; kk += MG_NQ) {                   // kept entry kk: one LDS address for the whole wave
        if (kcl[kk] == cls && match_above(kx1[kk], ky1[kk], kx2[kk], ky2[kk], kar[kk], g, area)) { supp[j] = 1; break; }
      }
#pragma unroll
      for (int c = 0; c < MG_PER; ++c) {
        const int i = MG_PER * q + c;
        if (i < j) {
          const float4 gi = cgeo[buf][i], mi = cmeta[buf][i];
          if (mi.y == cls && match_above(gi.x, gi.y, gi.z, gi.w, mi.w, g, area)) bits |= 1ull << i;
        }
      }
    }
    pmask[q][j] = bits;
    __syncthreads();
    if (tid < 64) {
      unsigned long long S = 0ull;
#pragma unroll
      for (int qq = 0; qq < MG_NQ; ++qq) S |= pmask[qq][tid];
      const bool alive = tid < m && !supp[tid];
      supp[tid] = 0;                                             // for the next chunk
      // K_j = alive_j & !(S_j & K): one solution; iterating from K = alive fixes members 0 .. t-1 after t rounds (nms_kernel)
      unsigned long long kmask = __ballot(alive);
      for (int it = 0; it < 64; ++it) {
        const unsigned long long k2 = __ballot(alive && !(S & kmask));
        if (k2 == kmask) break;
        kmask = k2;
      }
      if ((kmask >> tid) & 1ull) {
        const int pos = nk + __popcll(kmask & ((1ull << tid) - 1ull));
        if (pos < M) {
          const float4 g = cgeo[buf][tid], mt = cmeta[buf][tid];
          kx1[pos] = g.x; ky1[pos] = g.y; kx2[pos] = g.z; ky2[pos] = g.w; kar[pos] = mt.w; kcl[pos] = mt.y;
          float* d = a.dets + ((size_t)f * M + pos) * 6;
          d[0] = g.x; d[1] = g.y; d[2] = g.z; d[3] = g.w; d[4] = mt.x; d[5] = mt.y;
          if (a.src) a.src[(size_t)f * M + pos] = __float_as_int(mt.z);
        }
      }
      if (tid == 0) n_keep = min(M, nk + __popcll(kmask));
    }
    if (fetch) { cgeo[buf ^ 1][j] = ng; cmeta[buf ^ 1][j] = nm; }   // (that buffer's readers finished before the last barrier of the previous chunk)
    __syncthreads();
  }
  if (tid == 0) a.count[f] = n_keep;
}

}  // namespace

void yfv2_launch_tile_merge(const TileMergeArgs& a, hipStream_t s) {
  YFV2_LAUNCH(tile_rank_kernel, dim3((unsigned)a.T), dim3(RK_THREADS), 0, s, a);
  // the kept set of 4096 rows is 96 KB of dynamic LDS next to 12 KB of static: raise the function's limit to exactly that, once per device
  YFV2_LAUNCH_LDS(yfv2_device(), tile_merge_kernel, MG_MAX_OUT * 6 * (int)sizeof(float), dim3((unsigned)a.F), dim3(MG_THREADS), (size_t)a.max_out * 6 * sizeof(float), s, a);
}
