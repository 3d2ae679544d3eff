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
//
// The motion form (yfv2_track_update_motion) is the SAME kernel, track_kernel<true>: a slot is 32 words, its last 20
// the four constant-velocity filters of cx, cy, w, h.  They stay in global memory: the thread that owns a slot predicts them where
// the plain form reads the slot's box (and writes them back), sbox holds the PREDICTED corners, and the words are touched again only
// by the owner when the slot is matched (update) or dies (zeroed), and by the row's thread when a row is born into it.  A blind slot
// (a predicted word not finite, predicted w or h not > 0) gets NaN corners: track_iou then gives NaN, which is no edge - no flag,
// no LDS.  Words 0..3 (the last matched row) are written where they change, since sbox no longer holds them.  The filter is ONE
// __host__ __device__ function (track_filter_step: the kernel, yfv2_track_filter_step and yfv2_track_birth call it).
//
// The two-pass form (yfv2_track_update_two_pass) is the SAME kernel again, track_kernel<MOTION, true>, of either
// layout: the rounds are one routine, the body of a loop that runs once or twice.  A row's class - HIGH, LOW, OUT - comes from its
// conf in global memory, the way its cls does: no LDS.  The first run scans the HIGH rows with match_thres; a LOW row waits as (TK_LOW, 0),
// which every loop of the rounds skips.  Between the runs the unmatched HIGH rows are done as they stand, the LOW rows become "to be
// scanned", and a live unmatched slot that tracked_only bars gets the key TK_BARRED: the scan skips it like a taken one, the
// round's reset leaves it, and steps 4 / 5 see a slot that is not TK_TAKEN - unmatched.  The second run scans with match_thres_low.
// A matched row's pass is its class again (a HIGH row matches in the first run or is born, a LOW row matches in the second run or
// not at all), so track_pass and header word 6 need no state: a compare, and a ballot's count.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

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

// ---- the motion form's arithmetic: one constant-velocity Kalman filter per coordinate, x, v and the 2 x 2 covariance p00, p01, p11
struct TrackFilter { float x, v, p00, p01, p11; };

__host__ __device__ inline float track_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
// Which NaN an invalid operation makes differs between processors (the sign bit); what the rule stores or writes out is ONE quiet NaN.
__host__ __device__ inline float track_canon(float v) { return v != v ? __builtin_bit_cast(float, 0x7fc00000) : v; }
// one time step (predict, scale lp) and / or one measurement z (update, scale lu) of one filter: include/yfv2.h, operation by operation
__host__ __device__ __forceinline__ TrackFilter track_filter_step(TrackFilter f, bool predict, bool update, float z, float lp, float lu, const TrackMotion& m) {
#pragma clang fp contract(off)
  if (predict) {
    const float tp = m.std_pos * lp, tv = m.std_vel * lp;
    f.x = f.x + f.v;
    f.p00 = (((f.p00 + f.p01) + f.p01) + f.p11) + tp * tp;
    f.p01 = f.p01 + f.p11;
    f.p11 = f.p11 + tv * tv;
  }
  if (update) {
    const float tm = m.std_meas * lu;
    const float s = f.p00 + tm * tm;
    const float k0 = track_div(f.p00, s), k1 = track_div(f.p01, s), y = z - f.x;
    const float p00 = f.p00, p01 = f.p01;
    f.x = f.x + k0 * y;
    f.v = f.v + k1 * y;
    f.p00 = p00 - k0 * p00;
    f.p01 = p01 - k0 * p01;
    f.p11 = f.p11 - k1 * p01;
  }
  f.x = track_canon(f.x); f.v = track_canon(f.v); f.p00 = track_canon(f.p00); f.p01 = track_canon(f.p01); f.p11 = track_canon(f.p11);
  return f;
}
// a row's measurement cx, cy, w, h; a filter state's corners
__host__ __device__ __forceinline__ void track_measure(float x1, float y1, float x2, float y2, float z[4]) {
#pragma clang fp contract(off)
  z[0] = (x1 + x2) * 0.5f; z[1] = (y1 + y2) * 0.5f; z[2] = x2 - x1; z[3] = y2 - y1;
}
__host__ __device__ __forceinline__ void track_corners(float cx, float cy, float w, float h, float c[4]) {
#pragma clang fp contract(off)
  const float hw = w * 0.5f, hh = h * 0.5f;
  c[0] = track_canon(cx - hw); c[1] = track_canon(cy - hh); c[2] = track_canon(cx + hw); c[3] = track_canon(cy + hh);
}
// the filters of a track born from a row: cx and w scale with the row's w, cy and h with its h
__host__ __device__ __forceinline__ void track_birth(const float z[4], const TrackMotion& m, TrackFilter f[4]) {
#pragma clang fp contract(off)
  const float sp2 = 2.0f * m.std_pos, sv10 = 10.0f * m.std_vel;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float l = z[2 + (c & 1)], tp = sp2 * l, tv = sv10 * l;
    f[c].x = z[c]; f[c].v = 0.0f; f[c].p00 = tp * tp; f[c].p01 = 0.0f; f[c].p11 = tv * tv;
  }
}
__host__ __device__ __forceinline__ bool track_finite(float v) { return (v < 0.0f ? -v : v) <= 3.402823466e38f; }   // NaN or an infinity fails

// ---- the appearance form's arithmetic (include/yfv2.h "appearance association"): dot16 is sixteen partial sums and a tree over them.
// track_dot16_part is partial sum j - what ONE lane of a 16-lane group computes in the kernel, and what the host entry points loop
// over; the tree is four DPP row steps in the kernel (group_dot16 below) and track_dot16_tree on the host: the same additions.
__host__ __device__ __forceinline__ float track_dot16_part(const float* a, const float* b, int D, int j) {
#pragma clang fp contract(off)
  float p = 0.0f;
  for (int i = j; i < D; i += 16) p = p + a[i] * b[i];
  return p;
}
inline float track_dot16_tree(float P[16]) {
#pragma clang fp contract(off)
  for (int stride = 8; stride >= 1; stride >>= 1)
    for (int j = 0; j < stride; ++j) P[j] = P[j] + P[j + stride];
  return P[0];
}
// The square root rounded to nearest on both passes: sqrtf.  On the device that is the compiler's correctly rounded fp32 square root
// (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn is NOT - without OCML_BASIC_ROUNDED_OPERATIONS the
// toolchain's header defines it as the native, approximate instruction, which is one ulp off on sqrt(0.82f).
__host__ __device__ __forceinline__ float track_sqrt(float v) { return sqrtf(v); }
// a vector's norm from dot16(e, e), and whether it gives the row an appearance (an update a new feature): finite and > 0
__host__ __device__ __forceinline__ bool track_norm_ok(float n) { return n > 0.0f && track_finite(n); }
// the cosine of a row of norm n_r with a unit feature, from dot16(e, f); one quiet NaN, like the filter's results
__host__ __device__ __forceinline__ float track_cosine(float dot, float n_r) { return track_canon(track_div(dot, n_r)); }
// the value of a first-pass edge: the cosine c where both sides have an appearance (has), the boxes are close enough and c passes
// its own threshold and is the larger, else the IoU v.  by_app: the value is c
__host__ __device__ __forceinline__ float track_fuse(float v, float c, bool has, double prox, double app, bool& by_app) {
  by_app = has && (double)v > prox && track_finite(c) && (double)c > app && c > v;
  return by_app ? c : v;
}
// one element of a feature: of a first embedding, and of the moving average before it is normalised
__host__ __device__ __forceinline__ float track_feat_first(float e, float n_r) { return track_div(e, n_r); }
__host__ __device__ __forceinline__ float track_feat_blend(float f, float e, float n_r, float alpha, float beta) {
#pragma clang fp contract(off)
  return alpha * f + beta * track_div(e, n_r);
}

namespace {

constexpr int TK_MAX_THREADS = 1024;
constexpr int TK_TAKEN = -1;            // a row's v word: matched or born; a slot key's high word: dead or matched
constexpr int TK_BARRED = -2;           // (two-pass) a slot key's high word: live, unmatched, not offered to the second pass
constexpr int TK_LOW = -3;              // (two-pass) a row's slot word while the first pass runs: a LOW row, v word 0

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

// ---- the motion form's slot words 10..29, by the thread that owns them (w: the slot's first word)
__device__ __forceinline__ void filters_load(const int32_t* w, TrackFilter f[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int32_t* q = w + TRACK_FILTER + 5 * c;
    f[c].x = i2f(q[0]); f[c].v = i2f(q[1]); f[c].p00 = i2f(q[2]); f[c].p01 = i2f(q[3]); f[c].p11 = i2f(q[4]);
  }
}
__device__ __forceinline__ void filters_store(int32_t* w, const TrackFilter f[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int32_t* q = w + TRACK_FILTER + 5 * c;
    q[0] = f2i(f[c].x); q[1] = f2i(f[c].v); q[2] = f2i(f[c].p00); q[3] = f2i(f[c].p01); q[4] = f2i(f[c].p11);
  }
}
__device__ __forceinline__ float4 filters_corners(const TrackFilter f[4]) {
  float c[4];
  track_corners(f[0].x, f[1].x, f[2].x, f[3].x, c);
  return make_float4(c[0], c[1], c[2], c[3]);
}
__device__ __forceinline__ void box_store(int32_t* w, float4 g) { w[0] = f2i(g.x); w[1] = f2i(g.y); w[2] = f2i(g.z); w[3] = f2i(g.w); }
// step 0: a live slot's filters one frame on, written back; -> the predicted corners, NaN for a blind slot (no IoU with it is an edge)
__device__ __forceinline__ float4 slot_predict(int32_t* w, const TrackMotion& m) {
  if (w[6] == 0) return make_float4(0.f, 0.f, 0.f, 0.f);
  TrackFilter f[4];
  filters_load(w, f);
  const float lw = f[2].x, lh = f[3].x;
  bool seen = true;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    f[c] = track_filter_step(f[c], true, false, 0.0f, (c & 1) ? lh : lw, 0.0f, m);
    seen = seen && track_finite(f[c].x) && track_finite(f[c].v) && track_finite(f[c].p00) && track_finite(f[c].p01) && track_finite(f[c].p11);
  }
  filters_store(w, f);
  seen = seen && f[2].x > 0.0f && f[3].x > 0.0f;
  const float nan = __builtin_nanf("");
  return seen ? filters_corners(f) : make_float4(nan, nan, nan, nan);
}
// step 4: a matched slot's predicted filters take the row's measurement; -> the posterior corners
__device__ __forceinline__ float4 slot_update(int32_t* w, float4 g, const TrackMotion& m) {
  TrackFilter f[4];
  filters_load(w, f);
  float z[4];
  track_measure(g.x, g.y, g.z, g.w, z);
  const float lw = f[2].x, lh = f[3].x;
#pragma unroll
  for (int c = 0; c < 4; ++c) f[c] = track_filter_step(f[c], false, true, z[c], 0.0f, (c & 1) ? lh : lw, m);
  filters_store(w, f);
  return filters_corners(f);
}
// step 6: a row born into a free slot; -> the born state's corners
__device__ __forceinline__ float4 slot_birth(int32_t* w, float4 g, const TrackMotion& m) {
  TrackFilter f[4];
  float z[4];
  track_measure(g.x, g.y, g.z, g.w, z);
  track_birth(z, m, f);
  filters_store(w, f);
  return filters_corners(f);
}
__device__ __forceinline__ void row_box_store(float* track_box, size_t row, float4 c) {
  if (!track_box) return;
  float* o = track_box + row * 4;
  o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w;
}

// ---- the appearance form: a 16-lane group (a DPP row; lane j of it holds partial sum j) per pair, per slot or per row
// lane l <- lane l + N of its row: the tree step P[j] = P[j] + P[j + N] for j < N (the lanes above N hold values nothing reads)
template <int N>
__device__ __forceinline__ float row_down(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x100 + N, 0xf, 0xf, true));
}
__device__ __forceinline__ float group_tree(float p) {      // -> dot16's result in the group's lane 0
#pragma clang fp contract(off)
  p = p + row_down<8>(p);
  p = p + row_down<4>(p);
  p = p + row_down<2>(p);
  p = p + row_down<1>(p);
  return p;
}
__device__ __forceinline__ float group_dot16(const float* a, const float* b, int D, int j) { return group_tree(track_dot16_part(a, b, D, j)); }
__device__ __forceinline__ int* app_counter() {              // static LDS of the appearance kernels only: the others never name it
  __shared__ int s_app;
  return &s_app;
}
// The cosines of the wave's gated pairs of ONE slot (feature f): `gated` is the ballot of the lanes whose row passed the cheap tests,
// lane l's row is row_base + l.  Four pairs per step, one per 16-lane group; a gated lane gets its own c = dot16(e, f) / n_r.
__device__ __forceinline__ float wave_cosines(unsigned long long gated, const float* emb_rows, int row_base, const float* f, int D, float n_r, int lane) {
  const int grp = lane >> 4, j = lane & 15;
  float c = 0.0f;
  while (gated) {
    int src[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      src[k] = gated ? __builtin_ctzll(gated) : -1;
      gated &= gated - 1ull;
    }
    const int mine = grp == 0 ? src[0] : grp == 1 ? src[1] : grp == 2 ? src[2] : src[3];
    float dot = 0.0f;
    if (mine >= 0) dot = group_dot16(emb_rows + (size_t)(row_base + mine) * D, f, D, j);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dot), 16 * k));
      if (lane == src[k]) c = track_cosine(d, n_r);
    }
  }
  return c;
}

// MOTION: the slots are TRACK_SLOT_MOTION words and carry filters (above); TWO: the rounds run twice, over the HIGH rows and over
// the LOW rows (TrackTwoArgs; a plain table leaves its motion part unused); APP: first-pass edges may take the cosine of the row's
// embedding with the track's feature, and the features are kept (TrackAppArgs); everything else is the one kernel
template <bool MOTION, bool TWO, bool APP>
using track_args_t = std::conditional_t<APP, TrackAppArgs, std::conditional_t<TWO, TrackTwoArgs, std::conditional_t<MOTION, TrackMotionArgs, TrackArgs>>>;

template <bool MOTION, bool TWO, bool APP = false>
__global__ __launch_bounds__(TK_MAX_THREADS) void track_kernel(track_args_t<MOTION, TWO, APP> a) {
  constexpr int SLOT = MOTION ? TRACK_SLOT_MOTION : TRACK_SLOT;
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

  int32_t* const head = a.state + (size_t)a.stream_of[b] * (size_t)(TRACK_HEADER + SLOT * M);
  int32_t* const slots = head + TRACK_HEADER;
  const int n = min(max(a.count[b], 0), R);
  const float* const rows = a.dets + (size_t)b * R * 6;
  const int issued = head[0];
  // (appearance) a row's norm, 0 = no appearance, and a slot's n_feat, after the other forms' arrays; the stream's features; a
  // thread's place in its 16-lane group and the number of groups
  float* rnorm = nullptr;
  int* sfeat = nullptr;
  int32_t* feat = nullptr;
  const float* emb = nullptr;
  int D = 0, FS = 0, gj = 0, ng = 0;
  if constexpr (APP) {
    rnorm = reinterpret_cast<float*>(sage + M);
    sfeat = reinterpret_cast<int*>(rnorm + R);
    D = a.D; FS = TRACK_FEAT_HEAD + D; gj = tid & 15; ng = nt >> 4;
    feat = a.feat + (size_t)a.stream_of[b] * (size_t)M * (size_t)FS;
    emb = a.emb + (size_t)b * R * D;
  }

  if (tid == 0) s_deaths = 0;
  if constexpr (APP) {
    if (tid == 0) *app_counter() = 0;
  }
  for (int s = tid; s < M; s += nt) {
    int32_t* w = slots + SLOT * s;
    if constexpr (MOTION) sbox[s] = slot_predict(w, a.motion);
    else sbox[s] = make_float4(i2f(w[0]), i2f(w[1]), i2f(w[2]), i2f(w[3]));
    sconf[s] = i2f(w[4]); scls[s] = i2f(w[5]);
    sid[s] = w[6]; shits[s] = w[7]; smiss[s] = w[8]; sage[s] = w[9];
    skey[s] = w[6] == 0 ? ~0ull : 0ull;
    if constexpr (APP) sfeat[s] = feat[(size_t)s * FS];
  }
  if constexpr (APP) {                                        // the rows' norms, once per frame: a group per row
    for (int r = tid >> 4; r < n; r += ng) {
      const float* e = emb + (size_t)r * D;
      const float nr = track_sqrt(group_dot16(e, e, D, gj));
      if (gj == 0) rnorm[r] = track_norm_ok(nr) ? nr : 0.0f;
    }
  }
  for (int r = tid; r < n; r += nt) {
    const float* row = rows + 6 * r;
    const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
    bool valid = x2 > x1 && y2 > y1;
#pragma unroll
    for (int i = 0; i < 6; ++i) valid = valid && fabsf(row[i]) <= 3.402823466e38f;     // NaN or an infinity fails
    if constexpr (MOTION) {                                  // ... and so does a measurement that overflows
      float z[4];
      track_measure(x1, y1, x2, y2, z);
      valid = valid && track_finite(z[0]) && track_finite(z[1]) && track_finite(z[2]) && track_finite(z[3]);
    }
    rbox[r] = make_float4(x1, y1, x2, y2);
    if constexpr (TWO) {                                     // an OUT row is an invalid row; a LOW row waits for the second pass
      const float conf = row[4];
      rst[r] = !valid || !(conf >= a.low_conf) ? make_int2(-2, 0) : conf >= a.high_conf ? make_int2(-1, 1) : make_int2(TK_LOW, 0);
    } else {
      rst[r] = valid ? make_int2(-1, 1) : make_int2(-2, 0);   // v word: 0 = done, unmatched; 1 = to be scanned (no IoU's bits)
    }
  }
  __syncthreads();

  // ---- steps 2 and 3: the rounds - ONE routine: the rows whose v word says "to be scanned" against the slots whose key is free,
  // until no such row has an edge.  The two-pass form runs it twice: over the HIGH rows with match_thres, then (step 3b) over the LOW
  // rows and the slots still unmatched with match_thres_low; a key's high word may then also be TK_BARRED, which the scan skips like
  // TK_TAKEN and which, unlike a free key, the round's reset leaves alone.
  const bool aware = a.class_aware != 0;
  for (int pass = 0; pass < (TWO ? 2 : 1); ++pass) {
    double thres = a.thres;
    if constexpr (TWO) {
      if (pass == 1) {                                       // the first pass is complete: its unmatched HIGH rows are done as they stand
        for (int r = tid; r < n; r += nt)
          if (rst[r].x == TK_LOW) rst[r] = make_int2(-1, 1);
        if (a.tracked_only != 0)
          for (int s = tid; s < M; s += nt)                  // smiss is still the frame's first word: steps 4 and 5 come later
            if ((int)(skey[s] >> 32) != TK_TAKEN && smiss[s] != 0) skey[s] = (unsigned long long)(unsigned)TK_BARRED << 32;
        __syncthreads();
        thres = a.thres_low;
      }
    }
    for (;;) {
      int any = 0;
      if constexpr (APP) {
        // The same scan with every lane of a wave in the slot loop, so that the wave can work on its gated pairs together: a lane
        // whose row is done (or beyond n) scans with act = false and offers nothing.  In the first pass a slot with a feature makes
        // the lanes whose row has an appearance, the slot's class and an IoU above prox_thres vote; their cosines are computed four
        // pairs per step by wave_cosines, and the edge's value is track_fuse's.
        for (int r0 = 0; r0 < n; r0 += nt) {
          const int r = r0 + tid;
          const int2 q = r < n ? rst[r] : make_int2(-1, 0);
          const bool act = r < n && !(q.y == 0 || q.y == TK_TAKEN);
          if (__ballot(act) == 0ull) continue;
          const float4 g = act ? rbox[r] : make_float4(0.f, 0.f, 0.f, 0.f);
          const float garea = track_area(g.x, g.y, g.z, g.w);
          const float gcls = act ? rows[6 * r + 5] : 0.0f;
          const float nr = act && pass == 0 ? rnorm[r] : 0.0f;
          const unsigned long long low = (unsigned)~r;
          int best = -1, bv = 0;
          for (int s = 0; s < M; ++s) {
            if ((int)(skey[s] >> 32) < 0) continue;
            const bool open = act && !(aware && !(scls[s] == gcls));
            const float4 t = sbox[s];
            float v = track_iou(t.x, t.y, t.z, t.w, track_area(t.x, t.y, t.z, t.w), g.x, g.y, g.z, g.w, garea);
            if (pass == 0 && sfeat[s] > 0) {
              const bool gate = open && nr > 0.0f && (double)v > a.prox;
              const unsigned long long gated = __ballot(gate);
              if (gated != 0ull) {
                const float c = wave_cosines(gated, emb, r0 + tid - lane, reinterpret_cast<const float*>(feat + (size_t)s * FS + TRACK_FEAT_HEAD), D, nr, lane);
                bool by_app;
                v = track_fuse(v, c, gate, a.prox, a.app, by_app);
              }
            }
            if (open && (double)v > thres) {
              const int vb = f2i(v);
              atomicMax(&skey[s], ((unsigned long long)(unsigned)vb << 32) | low);
              if (vb > bv) { bv = vb; best = s; }
            }
          }
          if (act) rst[r] = make_int2(best, bv);
          any |= best >= 0;
        }
      } else
      for (int r = tid; r < n; r += nt) {
        const int2 q = rst[r];
        if (q.y == 0 || q.y == TK_TAKEN) continue;
        const float4 g = rbox[r];
        const float garea = track_area(g.x, g.y, g.z, g.w);
        const float gcls = rows[6 * r + 5];
        const unsigned long long low = (unsigned)~r;
        int best = -1, bv = 0;
        for (int s = 0; s < M; ++s) {                          // one LDS address for the whole wave
          if constexpr (TWO) {
            if ((int)(skey[s] >> 32) < 0) continue;          // ... or barred: every other high word is 0 or a positive fp32's bits
          } else {
            if ((int)(skey[s] >> 32) == TK_TAKEN) continue;  // dead or matched: stable during the scan, whatever the atomics do
          }
          if (aware && !(scls[s] == gcls)) continue;
          const float4 t = sbox[s];
          const float v = track_iou(t.x, t.y, t.z, t.w, track_area(t.x, t.y, t.z, t.w), g.x, g.y, g.z, g.w, garea);
          if ((double)v > thres) {                           // v > 0: its bits order like its value; NaN fails
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
      for (int s = tid; s < M; s += nt) {                      // the next round's offers start from nothing
        if constexpr (TWO) {
          if ((int)(skey[s] >> 32) >= 0) skey[s] = 0ull;
        } else {
          if ((int)(skey[s] >> 32) != TK_TAKEN) skey[s] = 0ull;
        }
      }
      __syncthreads();
    }
  }

  // ---- (appearance) steps 4 and 5 of the features, a group per live slot, while sbox, smiss and the keys are still the frame's:
  // the pair's cosine against the feature as it was, whether the walk took the pair at that cosine (header word 7), then the
  // feature's update; a slot that step 5 is about to kill loses its feature.  Lane j reads and writes elements 16 i + j only.
  if constexpr (APP) {
    for (int s = tid >> 4; s < M; s += ng) {
      if (sid[s] == 0) continue;
      int32_t* fw = feat + (size_t)s * FS;
      float* f = reinterpret_cast<float*>(fw + TRACK_FEAT_HEAD);
      const unsigned long long k = skey[s];
      if ((int)(k >> 32) == TK_TAKEN) {
        const int r = (int)(unsigned)k;
        const float nr = rnorm[r];
        const int nf = sfeat[s];
        const float* e = emb + (size_t)r * D;
        float c = 0.0f;
        if (nr > 0.0f && nf > 0) {
          c = track_cosine(group_dot16(e, f, D, gj), nr);
          if (gj == 0) {
            bool first = true, by_app;
            if constexpr (TWO) first = rows[6 * r + 4] >= a.high_conf;
            const float4 t = sbox[s], g = rbox[r];
            const float v = track_iou(t.x, t.y, t.z, t.w, track_area(t.x, t.y, t.z, t.w), g.x, g.y, g.z, g.w, track_area(g.x, g.y, g.z, g.w));
            track_fuse(v, c, first, a.prox, a.app, by_app);
            if (by_app) atomicAdd(app_counter(), 1);           // an integer sum: the same in any order
          }
        }
        if (gj == 0 && a.track_cos) a.track_cos[(size_t)b * R + r] = c;
        if (nr > 0.0f) {
          if (nf == 0) {
            for (int i = gj; i < D; i += 16) f[i] = track_feat_first(e[i], nr);
            if (gj == 0) fw[0] = 1;
          } else {
            float p = 0.0f;
            for (int i = gj; i < D; i += 16) {
              const float gv = track_feat_blend(f[i], e[i], nr, a.alpha, a.beta);
              p = __fadd_rn(p, __fmul_rn(gv, gv));
            }
            const float m = __shfl(track_sqrt(group_tree(p)), lane & ~15);
            if (track_norm_ok(m)) {
              for (int i = gj; i < D; i += 16) f[i] = track_div(track_feat_blend(f[i], e[i], nr, a.alpha, a.beta), m);
              if (gj == 0) fw[0] = nf + 1;
            }
          }
        }
      } else if (smiss[s] + 1 > a.max_misses) {
        for (int i = gj; i < FS; i += 16) fw[i] = 0;
      }
    }
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
        if constexpr (MOTION) {
          int32_t* w = slots + SLOT * s;
          box_store(w, rbox[r]);
          row_box_store(a.track_box, (size_t)b * R + r, slot_update(w, rbox[r], a.motion));
        } else {
          sbox[s] = rbox[r];
        }
        sconf[s] = rows[6 * r + 4]; scls[s] = rows[6 * r + 5];
        shits[s] += 1; smiss[s] = 0; sage[s] += 1;
      } else {
        const int m = smiss[s] + 1;
        smiss[s] = m; sage[s] += 1;
        if (m > a.max_misses) {
          died = true;
          if constexpr (MOTION) {
            int32_t* w = slots + SLOT * s;
            box_store(w, make_float4(0.f, 0.f, 0.f, 0.f));
#pragma unroll
            for (int i = TRACK_FILTER; i < TRACK_FILTER + 20; ++i) w[i] = 0;
          } else {
            sbox[s] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
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
      if constexpr (TWO) want = want && conf >= a.high_conf;   // an unmatched LOW row ends as (-1, 0) too: it never starts a track
    }
    int total;
    const int k = nb + block_rank(want, s_cnt, total);
    if (want && k < nfree) {
      const int s = freel[k];
      if constexpr (MOTION) {
        int32_t* w = slots + SLOT * s;
        box_store(w, rbox[r]);
        row_box_store(a.track_box, (size_t)b * R + r, slot_birth(w, rbox[r], a.motion));
      } else {
        sbox[s] = rbox[r];
      }
      sconf[s] = conf; scls[s] = rows[6 * r + 5];
      sid[s] = issued + 1 + k; shits[s] = 1; smiss[s] = 0; sage[s] = 1;
      rst[r] = make_int2(s, TK_TAKEN);
    }
    nb += total;
  }
  const int born = min(nb, nfree);
  __syncthreads();
  if constexpr (APP) {                                        // step 6 of the features, a group per born row (its slot's hits are 1)
    for (int r = tid >> 4; r < n; r += ng) {
      const int2 q = rst[r];
      if (q.y != TK_TAKEN || shits[q.x] != 1) continue;
      int32_t* fw = feat + (size_t)q.x * FS;
      const float nr = rnorm[r];
      if (nr > 0.0f) {
        const float* e = emb + (size_t)r * D;
        float* f = reinterpret_cast<float*>(fw + TRACK_FEAT_HEAD);
        for (int i = gj; i < D; i += 16) f[i] = track_feat_first(e[i], nr);
        if (gj < TRACK_FEAT_HEAD) fw[gj] = gj == 0 ? 1 : 0;
      } else {
        for (int i = gj; i < FS; i += 16) fw[i] = 0;
      }
    }
  }

  // ---- steps 7 and 8: the rows' outputs, the fresh rows in row order
  const bool emit = a.fresh_dets != nullptr;
  int nfresh = 0, nsecond = 0;
  for (int r0 = 0; r0 < R; r0 += nt) {
    const int r = r0 + tid;
    int id = 0, hits = 0;
    if (r < n) {
      const int2 q = rst[r];
      if (q.y == TK_TAKEN) { id = sid[q.x]; hits = shits[q.x]; }
    }
    if constexpr (TWO) {                                     // an assigned row's pass is its class: HIGH matched first or was born
      const int pass = id == 0 ? 0 : rows[6 * r + 4] >= a.high_conf ? 1 : 2;
      if (r < R && a.track_pass) a.track_pass[(size_t)b * R + r] = pass;
      int total;
      block_rank(pass == 2, s_cnt, total);
      nsecond += total;
    }
    if (r < R) {
      a.track_id[(size_t)b * R + r] = id;
      if (a.track_hits) a.track_hits[(size_t)b * R + r] = hits;
      if constexpr (MOTION)
        if (id == 0) row_box_store(a.track_box, (size_t)b * R + r, make_float4(0.f, 0.f, 0.f, 0.f));   // an assigned row's was written with its filter
      if constexpr (APP)
        if (a.track_cos && hits < 2) a.track_cos[(size_t)b * R + r] = 0.0f;                            // a matched row's was written with its feature
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
    int32_t* w = slots + SLOT * s;
    if constexpr (!MOTION) {
      const float4 t = sbox[s];
      w[0] = f2i(t.x); w[1] = f2i(t.y); w[2] = f2i(t.z); w[3] = f2i(t.w);
    }
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
    if constexpr (TWO) head[6] += nsecond;
    if constexpr (APP) head[7] += *app_counter();              // written before the barrier that follows the features' step 4
    if (emit) a.fresh_count[b] = nfresh;
  }
}

}  // namespace

// Dynamic LDS: 24 R + 48 M bytes, and 28 R + 52 M in the appearance form (yfv2_track_lds_bytes, yfv2_internal.h), whose entry point
// refuses an (R, M) above TRACK_APP_LDS_MAX - the other forms' largest, R = 4096 and M = 1024, is 144 KB.
template <bool MOTION, bool TWO, bool APP = false>
static void launch_track(const track_args_t<MOTION, TWO, APP>& a, int frames, hipStream_t s) {
  const int threads = std::min(TK_MAX_THREADS, std::max(64, (a.R + 63) / 64 * 64));
  const size_t lds = yfv2_track_lds_bytes(APP, a.R, a.M);
  constexpr int limit = APP ? (int)TRACK_APP_LDS_MAX : (int)yfv2_track_lds_bytes(false, TRACK_MAX_R, TRACK_MAX_M);
  YFV2_LAUNCH_LDS(yfv2_device(), (track_kernel<MOTION, TWO, APP>), limit, dim3((unsigned)frames), dim3((unsigned)threads), lds, s, a);
}
// a binds to each instantiation's own argument type (a base of TrackAppArgs): a kernel is passed that part and nothing else
void yfv2_launch_track(const TrackAppArgs& a, TrackForm form, int frames, hipStream_t s) {
  switch (form.motion | form.two_pass << 1 | form.appearance << 2) {
    case 0: return launch_track<false, false>(a, frames, s);
    case 1: return launch_track<true, false>(a, frames, s);
    case 2: return launch_track<false, true>(a, frames, s);
    case 3: return launch_track<true, true>(a, frames, s);
    case 4: return launch_track<false, false, true>(a, frames, s);
    case 5: return launch_track<true, false, true>(a, frames, s);
    case 6: return launch_track<false, true, true>(a, frames, s);
    case 7: return launch_track<true, true, true>(a, frames, s);
  }
}

extern "C" int yfv2_track_iou(const float a[4], const float b[4], float* v) {
  if (!a || !b || !v) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_iou: null pointer");
  *v = track_iou(a[0], a[1], a[2], a[3], track_area(a[0], a[1], a[2], a[3]), b[0], b[1], b[2], b[3], track_area(b[0], b[1], b[2], b[3]));
  return YFV2_OK;
}

// ---- the appearance form's arithmetic for the host (tests pin it to the model without a device): the partial sums, the tree and
// the element functions are the ones the kernel calls
static float host_dot16(const float* a, const float* b, int D) {
  float P[16];
  for (int j = 0; j < 16; ++j) P[j] = track_dot16_part(a, b, D, j);
  return track_dot16_tree(P);
}

extern "C" int yfv2_track_cosine(const float* e, const float* f, int32_t D, float* norm, float* cos) {
  if (!e || !f || !norm || !cos) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_cosine: null pointer");
  if (!yfv2_track_dim_ok(D)) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_cosine: D must be a multiple of 16 in 16..2048");
  const float n = track_canon(track_sqrt(host_dot16(e, e, D)));
  *norm = n;
  *cos = track_cosine(host_dot16(e, f, D), n);
  return YFV2_OK;
}

extern "C" int yfv2_track_feature_step(const float* f_in, int32_t n_feat_in, const float* e, int32_t D, float alpha, float* f_out, int32_t* n_feat_out) {
  if (!f_in || !e || !f_out || !n_feat_out) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_feature_step: null pointer");
  if (!yfv2_track_dim_ok(D)) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_feature_step: D must be a multiple of 16 in 16..2048");
  if (n_feat_in < 0) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_feature_step: n_feat_in < 0");
  if (!std::isfinite(alpha) || alpha < 0.0f || alpha > 1.0f) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_feature_step: alpha must be in [0, 1]");
  const float beta = 1.0f - alpha;
  const float nr = track_sqrt(host_dot16(e, e, D));
  std::vector<float> g(f_in, f_in + D);
  int32_t nf = n_feat_in;
  if (track_norm_ok(nr)) {
    if (nf == 0) {
      for (int i = 0; i < D; ++i) g[i] = track_feat_first(e[i], nr);
      nf = 1;
    } else {
      for (int i = 0; i < D; ++i) g[i] = track_feat_blend(f_in[i], e[i], nr, alpha, beta);
      const float m = track_sqrt(host_dot16(g.data(), g.data(), D));
      if (track_norm_ok(m)) {
        for (int i = 0; i < D; ++i) g[i] = track_div(g[i], m);
        nf += 1;
      } else {
        std::copy(f_in, f_in + D, g.begin());
      }
    }
  }
  std::copy(g.begin(), g.end(), f_out);
  *n_feat_out = nf;
  return YFV2_OK;
}

// ---- the motion form's arithmetic for the host (tests pin it to the model without a device)
extern "C" int yfv2_track_filter_step(const float in[5], const float* z, float scale_predict, float scale_update, const yfv2_track_motion* motion, float out[5]) {
  if (!in || !out || !motion) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_filter_step: null pointer");
  if (!yfv2_track_motion_ok(motion->std_pos, motion->std_vel, motion->std_meas))
    return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_filter_step: std_pos, std_vel and std_meas must be finite and > 0");
  const TrackMotion m{motion->std_pos, motion->std_vel, motion->std_meas};
  const TrackFilter f = track_filter_step(TrackFilter{in[0], in[1], in[2], in[3], in[4]}, true, z != nullptr, z ? *z : 0.0f, scale_predict, scale_update, m);
  out[0] = f.x; out[1] = f.v; out[2] = f.p00; out[3] = f.p01; out[4] = f.p11;
  return YFV2_OK;
}

extern "C" int yfv2_track_birth(const float row_box[4], const yfv2_track_motion* motion, float out[20]) {
  if (!row_box || !out || !motion) return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_birth: null pointer");
  if (!yfv2_track_motion_ok(motion->std_pos, motion->std_vel, motion->std_meas))
    return yfv2_ctx_fail(nullptr, YFV2_ERR_ARG, "yfv2_track_birth: std_pos, std_vel and std_meas must be finite and > 0");
  const TrackMotion m{motion->std_pos, motion->std_vel, motion->std_meas};
  float z[4];
  TrackFilter f[4];
  track_measure(row_box[0], row_box[1], row_box[2], row_box[3], z);
  track_birth(z, m, f);
  for (int c = 0; c < 4; ++c) {
    float* o = out + 5 * c;
    o[0] = f[c].x; o[1] = f[c].v; o[2] = f[c].p00; o[3] = f[c].p01; o[4] = f[c].p11;
  }
  return YFV2_OK;
}
