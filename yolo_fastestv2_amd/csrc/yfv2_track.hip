// yfv2_track.hip - identity across frames (yfv2_track_update): one workgroup per frame updates its stream's table
// of tracks from the frame's detection rows.  THE RULE is stated in include/yfv2.h and restated in tests/track_model.py; the IoU
// is ONE __host__ __device__ function (track_iou below: the kernel and yfv2_track_iou, the host entry point, both call it), and the
// unit is built with -ffp-contract=off so that both passes round every fp32 operation on its own.
//
// The greedy walk of the rule - edges by (v descending, row ascending, slot ascending), an edge taken when its row and its slot are
// both free - is sequential as written.  Its parallel form: the FIRST edge of that order among the edges that share a row or a slot
// with it is taken by the walk whatever else happens (nothing in front of it can claim its row or its slot), so every round
//   (a) every free row scans the free live slots: it names its best edge (highest v, lowest slot on ties: the scan ascends and
//       replaces on strictly greater only) and offers EVERY edge it has to that edge's slot by one 64-bit LDS atomicMax on
//       (bits(v) << 32) | ~row - a positive fp32 orders like its bits, ~row makes the lowest row win a tie;
//   (b) a row whose named slot's key is its own is the slot's best over ALL free rows and the slot is the row's best: the pair is
//       taken.  (A slot must hear from every row with an edge to it, not only from the rows that named it: a row that prefers
//       another slot and loses it comes back for this one IN FRONT of the row that named it.)
// until no free row has an edge.  Edges only disappear, so a row without an edge is done.  The round count is data-dependent: 2-4 on
// post-NMS rows, min(n, M) on a chain whose every edge has a heavier neighbour.  The result is the walk's, so it depends on nothing but
// the rows and the table; deaths, free slots, births and fresh rows are numbered by ballots and integer prefix sums in slot / row order.
//
// LDS (dynamic, 24 R + 48 M bytes: 144 KB at R = 4096, M = 1024): the row boxes (16 B), the row state (8 B: slot, bits(v) of the named
// edge; v = -1: matched), the table as arrays (40 B per slot) and the slot keys (8 B; high word -1: dead or matched, low word the
// row).  Slots are read as wave-uniform broadcasts, the way tile_merge_kernel reads its kept set; conf and cls of a row come from
// global memory where they are needed.
#include <algorithm>

#include "../../include/yfv2.h"
#include "yfv2_device.h"

// a, b: x1, y1, x2, y2.  Selects instead of fmaxf / fminf: the same values on finite inputs, and a zero extent is +0 on both passes.
__host__ __device__ inline float track_area(float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
  const float w = x2 - x1, h = y2 - y1;
  return w * h;
}
__host__ __device__ inline float track_iou(float ax1, float ay1, float ax2, float ay2, float aarea, float bx1, float by1, float bx2, float by2, float barea) {
#pragma clang fp contract(off)
  const float xx1 = ax1 > bx1 ? ax1 : bx1, yy1 = ay1 > by1 ? ay1 : by1;
  const float xx2 = ax2 < bx2 ? ax2 : bx2, yy2 = ay2 < by2 ? ay2 : by2;
  const float dw = xx2 - xx1, dh = yy2 - yy1;
  const float w = dw > 0.0f ? dw : 0.0f, h = dh > 0.0f ? dh : 0.0f;
  const float inter = w * h;
  const float sum = aarea + barea;
  const float den = sum - inter;
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(inter, den);
#else
  return inter / den;
#endif
}

namespace {

constexpr int TK_MAX_THREADS = 1024;
constexpr int TK_TAKEN = -1;            // a row's v word: matched or born; a slot key's high word: dead or matched

// the rank of this thread's flag among the workgroup's set flags, in thread order; every thread of the workgroup calls it
__device__ __forceinline__ int block_rank(bool f, int* s_cnt, int& total) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  const unsigned long long m = __ballot(f);
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = 0;
  total = 0;
  for (int w = 0; w < nw; ++w) {
    const int c = s_cnt[w];
    if (w < wave) before += c;
    total += c;
  }
  __syncthreads();                      // s_cnt is rewritten by the next call
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(TK_MAX_THREADS) void track_kernel(TrackArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_lds[];
  __shared__ int s_cnt[TK_MAX_THREADS / 64];
  __shared__ int s_deaths;
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x, lane = tid & 63;
  const int b = (int)blockIdx.x, R = a.R, M = a.M;
  float4* const rbox = reinterpret_cast<float4*>(tk_lds);
  float4* const sbox = rbox + R;
  int2* const rst = reinterpret_cast<int2*>(sbox + M);
  unsigned long long* const skey = reinterpret_cast<unsigned long long*>(rst + R);
  float* const sconf = reinterpret_cast<float*>(skey + M);
  float* const scls = sconf + M;
  int* const sid = reinterpret_cast<int*>(scls + M);
  int* const shits = sid + M;
  int* const smiss = shits + M;
  int* const sage = smiss + M;

  int32_t* const head = a.state + (size_t)a.stream_of[b] * (size_t)(TRACK_HEADER + TRACK_SLOT * M);
  int32_t* const slots = head + TRACK_HEADER;
  const int n = min(max(a.count[b], 0), R);
  const float* const rows = a.dets + (size_t)b * R * 6;
  const int issued = head[0];

  if (tid == 0) s_deaths = 0;
  for (int s = tid; s < M; s += nt) {
    const int32_t* w = slots + TRACK_SLOT * s;
    sbox[s] = make_float4(i2f(w[0]), i2f(w[1]), i2f(w[2]), i2f(w[3]));
    sconf[s] = i2f(w[4]); scls[s] = i2f(w[5]);
    sid[s] = w[6]; shits[s] = w[7]; smiss[s] = w[8]; sage[s] = w[9];
    skey[s] = w[6] == 0 ? ~0ull : 0ull;
  }
  for (int r = tid; r < n; r += nt) {
    const float* row = rows + 6 * r;
    const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
    bool valid = x2 > x1 && y2 > y1;
#pragma unroll
    for (int i = 0; i < 6; ++i) valid = valid && fabsf(row[i]) <= 3.402823466e38f;     // NaN or an infinity fails
    rbox[r] = make_float4(x1, y1, x2, y2);
    rst[r] = valid ? make_int2(-1, 1) : make_int2(-2, 0);   // v word: 0 = done, unmatched; 1 = to be scanned (no IoU's bits)
  }
  __syncthreads();

  // ---- steps 2 and 3: the rounds
  const double thres = a.thres;
  const bool aware = a.class_aware != 0;
  for (;;) {
    int any = 0;
    for (int r = tid; r < n; r += nt) {
      const int2 q = rst[r];
      if (q.y == 0 || q.y == TK_TAKEN) continue;
      const float4 g = rbox[r];
      const float garea = track_area(g.x, g.y, g.z, g.w);
      const float gcls = rows[6 * r + 5];
      const unsigned long long low = (unsigned)~r;
      int best = -1, bv = 0;
      for (int s = 0; s < M; ++s) {                          // one LDS address for the whole wave
        if ((int)(skey[s] >> 32) == TK_TAKEN) continue;      // dead or matched: stable during the scan, whatever the atomics do
        if (aware && !(scls[s] == gcls)) continue;
        const float4 t = sbox[s];
        const float v = track_iou(t.x, t.y, t.z, t.w, track_area(t.x, t.y, t.z, t.w), g.x, g.y, g.z, g.w, garea);
        if ((double)v > thres) {                             // v > 0: its bits order like its value; NaN fails
          const int vb = f2i(v);
          atomicMax(&skey[s], ((unsigned long long)(unsigned)vb << 32) | low);
          if (vb > bv) { bv = vb; best = s; }
        }
      }
      rst[r] = make_int2(best, bv);                          // no edge: (-1, 0), done
      any |= best >= 0;
    }
    if (!__syncthreads_or(any)) break;
    for (int r = tid; r < n; r += nt) {
      const int2 q = rst[r];
      if (q.y == 0 || q.y == TK_TAKEN) continue;
      if (skey[q.x] == (((unsigned long long)(unsigned)q.y << 32) | (unsigned)~r)) rst[r].y = TK_TAKEN - 1;   // mutual: marked, taken below
    }
    __syncthreads();
    for (int r = tid; r < n; r += nt) {
      const int2 q = rst[r];
      if (q.y != TK_TAKEN - 1) continue;
      skey[q.x] = ((unsigned long long)(unsigned)TK_TAKEN << 32) | (unsigned)r;
      rst[r].y = TK_TAKEN;
    }
    __syncthreads();
    for (int s = tid; s < M; s += nt)
      if ((int)(skey[s] >> 32) != TK_TAKEN) skey[s] = 0ull;  // the next round's offers start from nothing
    __syncthreads();
  }

  // ---- steps 4 and 5: matched slots take their row, the others miss and may die
  for (int s0 = 0; s0 < M; s0 += nt) {
    const int s = s0 + tid;
    bool died = false;
    if (s < M && sid[s] != 0) {
      const unsigned long long k = skey[s];
      if ((int)(k >> 32) == TK_TAKEN) {
        const int r = (int)(unsigned)k;
        sbox[s] = rbox[r];
        sconf[s] = rows[6 * r + 4]; scls[s] = rows[6 * r + 5];
        shits[s] += 1; smiss[s] = 0; sage[s] += 1;
      } else {
        const int m = smiss[s] + 1;
        smiss[s] = m; sage[s] += 1;
        if (m > a.max_misses) {
          died = true;
          sbox[s] = make_float4(0.f, 0.f, 0.f, 0.f);
          sconf[s] = 0.f; scls[s] = 0.f; sid[s] = 0; shits[s] = 0; smiss[s] = 0; sage[s] = 0;
        }
      }
    }
    const unsigned long long dm = __ballot(died);
    if (lane == 0 && dm) atomicAdd(&s_deaths, __popcll(dm));   // an integer sum: the same in any order
  }
  __syncthreads();

  // ---- step 6: the free slots in ascending order (the keys' LDS is free now), then the births in row order
  int* const freel = reinterpret_cast<int*>(skey);
  int nfree = 0;
  for (int s0 = 0; s0 < M; s0 += nt) {
    const int s = s0 + tid;
    const bool fr = s < M && sid[s] == 0;
    int total;
    const int k = nfree + block_rank(fr, s_cnt, total);
    if (fr) freel[k] = s;
    nfree += total;
  }
  __syncthreads();
  int nb = 0;
  for (int r0 = 0; r0 < n; r0 += nt) {
    const int r = r0 + tid;
    bool want = false;
    float conf = 0.f;
    if (r < n) {
      const int2 q = rst[r];
      conf = rows[6 * r + 4];
      want = q.x == -1 && q.y == 0 && conf >= a.init_conf;
    }
    int total;
    const int k = nb + block_rank(want, s_cnt, total);
    if (want && k < nfree) {
      const int s = freel[k];
      sbox[s] = rbox[r];
      sconf[s] = conf; scls[s] = rows[6 * r + 5];
      sid[s] = issued + 1 + k; shits[s] = 1; smiss[s] = 0; sage[s] = 1;
      rst[r] = make_int2(s, TK_TAKEN);
    }
    nb += total;
  }
  const int born = min(nb, nfree);
  __syncthreads();

  // ---- steps 7 and 8: the rows' outputs, the fresh rows in row order
  const bool emit = a.fresh_dets != nullptr;
  int nfresh = 0;
  for (int r0 = 0; r0 < R; r0 += nt) {
    const int r = r0 + tid;
    int id = 0, hits = 0;
    if (r < n) {
      const int2 q = rst[r];
      if (q.y == TK_TAKEN) { id = sid[q.x]; hits = shits[q.x]; }
    }
    if (r < R) {
      a.track_id[(size_t)b * R + r] = id;
      if (a.track_hits) a.track_hits[(size_t)b * R + r] = hits;
    }
    if (emit) {
      const bool fresh = hits == a.confirm_hits;             // hits >= 1 on an assigned row, 0 elsewhere; confirm_hits >= 1
      int total;
      const int j = nfresh + block_rank(fresh, s_cnt, total);
      if (fresh) {
        const float* row = rows + 6 * r;
        float* o = a.fresh_dets + ((size_t)b * R + j) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) o[i] = row[i];
        a.fresh_src[(size_t)b * R + j] = r;
      }
      nfresh += total;
    }
  }

  // ---- the table and the header go back
  for (int s = tid; s < M; s += nt) {
    int32_t* w = slots + TRACK_SLOT * s;
    const float4 t = sbox[s];
    w[0] = f2i(t.x); w[1] = f2i(t.y); w[2] = f2i(t.z); w[3] = f2i(t.w);
    w[4] = f2i(sconf[s]); w[5] = f2i(scls[s]);
    w[6] = sid[s]; w[7] = shits[s]; w[8] = smiss[s]; w[9] = sage[s];
  }
  if (tid == 0) {
    head[0] = issued + born;
    head[1] = M - nfree + born;
    head[2] += 1;
    head[3] += born;
    head[4] += s_deaths;
    head[5] += nb - born;
    if (emit) a.fresh_count[b] = nfresh;
  }
}

}  // namespace

void yfv2_launch_track(const TrackArgs& a, int frames, hipStream_t s) {
  const int threads = std::min(TK_MAX_THREADS, std::max(64, (a.R + 63) / 64 * 64));
  const size_t lds = (size_t)24 * a.R + (size_t)48 * a.M;
  YFV2_LAUNCH_LDS(yfv2_device(), track_kernel, 24 * TRACK_MAX_R + 48 * TRACK_MAX_M, dim3((unsigned)frames), dim3((unsigned)threads), lds, s, a);
}

extern "C" int yfv2_track_iou(const float a[4], const float b[4], float* v) {
  if (!a || !b || !v) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_iou: null pointer");
  *v = track_iou(a[0], a[1], a[2], a[3], track_area(a[0], a[1], a[2], a[3]), b[0], b[1], b[2], b[3], track_area(b[0], b[1], b[2], b[3]));
  return YFV2_OK;
}
