// yfv2_ap.hip - average precision per class (the reference's utils/utils.py:110-134 compute_ap and :136-192 ap_per_class) on the
// device: a stable key-value radix sort that ranks the detections, then one walk per class over its ranked segment.  Built with
// -ffp-contract=off: every quotient, difference, product and sum rounds on its own, as numpy's float64 operations do.
//
// RANK.  Detections are ordered by class, inside a class by confidence descending, equal confidences (+0 == -0) by ascending input
// index: np.argsort(-conf, kind="stable").  A least-significant-digit radix sort delivers exactly that: four 8-bit passes over the
// order-preserving 32-bit image of -conf (zero canonicalised), then one 8-bit pass over the class (255 = a prediction of no
// target class); every pass is stable, so ties keep their input order.  Payload: the input index with tp in the top bit.
// Per pass: ap_hist_kernel (digit counts of each tile of YFV2_AP_TILE detections), ap_scan_kernel (one workgroup per digit: exclusive
// scan along the digit's row of the table, row total), ap_scatter_kernel (digit bases from the 256 totals, then a stable scatter:
// wave w of a workgroup owns the w-th quarter of the tile, ranks its 64 detections of a round by ballot and popcount and
// advances its own per-digit cursor; the cursors of the four waves start in wave order).  The last pass's row totals are the classes'
// segments.
//
// CURVE.  ap_curve_kernel, one workgroup per class, walks the segment in chunks of YFV2_AP_CH = 1024 positions from the back:
//     tpc_i  = inclusive integer count of tp                      prec_i = double(tpc_i) / double(i + 1)
//     rec_i  = double(tpc_i) / (double(n_gt) + 1e-16)             env_i  = max(prec_j, j >= i)
//     term_i = tp_i ? (rec_i - rec_{i-1}) * env_i : +0.0          (rec_{i-1} = double(tpc_i - 1) / (...) where tp_i = 1)
// The integer scan and the max scan are exact under any association.  The SUM is one fixed tree (DESIGN.md 4.10's rule): lane t of
// the 256 adds the chunk's terms t, t + 256, t + 512, t + 768 in that order, each wave folds its 64 lane values in halves, the four
// wave values are added in ascending order; the chunk sums are added in ascending chunk order.  Its shape depends only on a term's
// position inside its class's segment - not on the grid, the device or the run.  No floating-point atomic anywhere; counts use
// integer atomics.  tests/ap_model.py is the numpy restatement the device is compared with bit for bit.
//
// K THRESHOLDS (yfv2_ap_per_class_multi).  The rank does not look at tp, so targets, keys and the five passes run once; then
// ap_permute_kernel brings the callers' masks (bit k = tp at threshold k) into rank order and ap_curve_kernel<true> runs on a
// (class, k) grid, reading bit k of the permuted word where ap_curve_kernel<false> reads bit 31 of the payload.  It is ONE body: the
// template parameter selects where the bit comes from and which result block and chunk-sum set are written, nothing else, so
// slice k is what the single-threshold call computes from tp = bit k.  n_gt and the bad-input word exist once, in block 0.
#include "../../include/yfv2.h"
#include "yfv2_device.h"

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_WAVE_ITEMS = YFV2_AP_TILE / 4;    // detections per wave of a sort workgroup
constexpr int AP_ROUNDS = AP_WAVE_ITEMS / 64;      // ... in rounds of one per lane
constexpr int AP_ROWS = YFV2_AP_CH / AP_THREADS;   // terms per lane of a chunk
static_assert(YFV2_AP_TILE % 256 == 0 && YFV2_AP_CH % AP_THREADS == 0, "tile and chunk are whole rounds");

// ---- input checks and the 256-bin histogram of the target classes
__global__ __launch_bounds__(AP_THREADS) void ap_targets_kernel(ApArgs a) {
  __shared__ unsigned s_hist[256];
  const int tid = threadIdx.x;
  s_hist[tid] = 0;
  __syncthreads();
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * AP_THREADS + tid; i < a.T; i += (int64_t)gridDim.x * AP_THREADS) {
    const float c = a.target_cls[i];
    if (c >= 0.0f && c <= 254.0f && (float)(int)c == c) atomicAdd(&s_hist[(int)c], 1u);
    else bad = true;   // a NaN fails the first comparison; the value is never used as an index
  }
  if (bad) atomicOr(&a.head->bad, 1);
  __syncthreads();
  if (s_hist[tid] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&a.head->n_gt[tid]), (unsigned long long)s_hist[tid]);
}

// ---- keys and payloads
__global__ __launch_bounds__(AP_THREADS) void ap_prep_kernel(ApArgs a) {
  const int64_t i = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
  if (i >= a.N) return;
  const float c = a.conf[i];
  const unsigned cb = __builtin_bit_cast(unsigned, c);
  if ((cb << 1) >= 0xff000000u) atomicOr(&a.head->bad, 1);          // exponent all ones: NaN or infinity
  const unsigned u = (cb << 1) == 0 ? 0u : cb ^ 0x80000000u;         // the bits of -conf; +0 and -0 are one key
  a.key[0][i] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);          // ascending as unsigned = ascending -conf = descending conf
  a.val[0][i] = (unsigned)i | (a.tp != nullptr && a.tp[i] != 0 ? 0x80000000u : 0u);
}

// digit of a detection in pass 0..3 (a byte of the key) or 4 (its class; 255: a class no target has)
__device__ __forceinline__ int ap_digit(const ApArgs& a, int pass, unsigned key, unsigned val, const unsigned char* s_present) {
  if (pass < 4) return (int)((key >> (8 * pass)) & 255u);
  const float c = a.pred_cls[val & 0x7fffffffu];
  if (c >= 0.0f && c <= 254.0f) {
    const int ci = (int)c;
    if ((float)ci == c && s_present[ci]) return ci;
  }
  return 255;
}

__device__ __forceinline__ void ap_load_present(const ApArgs& a, int pass, unsigned char* s_present) {
  const int tid = threadIdx.x;
  s_present[tid] = (pass == 4 && tid < 255 && a.head->n_gt[tid] > 0) ? 1 : 0;
}

// ---- pass, first launch: digit counts of every tile
__global__ __launch_bounds__(AP_THREADS) void ap_hist_kernel(ApArgs a, int pass) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned char s_present[256];
  const int tid = threadIdx.x;
  s_hist[tid] = 0;
  ap_load_present(a, pass, s_present);
  __syncthreads();
  const unsigned* key = a.key[pass & 1];
  const unsigned* val = a.val[pass & 1];
  const int64_t base = (int64_t)blockIdx.x * YFV2_AP_TILE + tid;
#pragma unroll
  for (int r = 0; r < YFV2_AP_TILE / AP_THREADS; ++r) {
    const int64_t p = base + (int64_t)r * AP_THREADS;
    if (p < a.N) atomicAdd(&s_hist[ap_digit(a, pass, pass < 4 ? key[p] : 0u, pass < 4 ? 0u : val[p], s_present)], 1u);   // 4 B per row either way
  }
  __syncthreads();
  a.hist[(size_t)tid * (size_t)a.nblk + blockIdx.x] = s_hist[tid];
}

// ---- pass, second launch (one workgroup per digit): exclusive scan along the digit's row, the row total
__global__ __launch_bounds__(AP_THREADS) void ap_scan_kernel(ApArgs a) {
  __shared__ unsigned s_w[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* row = a.hist + (size_t)blockIdx.x * (size_t)a.nblk;
  unsigned carry = 0;
  for (int base = 0; base < a.nblk; base += AP_THREADS) {
    const int i = base + tid;
    const unsigned x = i < a.nblk ? row[i] : 0u;
    unsigned inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned y = __shfl_up(inc, off, 64);
      if (lane >= off) inc += y;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned t = s_w[w];
      if (w < wave) before += t;
      total += t;
    }
    if (i < a.nblk) row[i] = before + inc - x;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) a.tot[blockIdx.x] = carry;
}

// ---- pass, third launch: the stable scatter
__global__ __launch_bounds__(AP_THREADS) void ap_scatter_kernel(ApArgs a, int pass) {
  __shared__ unsigned s_tot[256];
  __shared__ unsigned s_cur[4][256];   // per wave and digit: first the wave's count, then its cursor
  __shared__ unsigned char s_present[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_tot[tid] = a.tot[tid];
#pragma unroll
  for (int w = 0; w < 4; ++w) s_cur[w][tid] = 0;
  ap_load_present(a, pass, s_present);
  __syncthreads();
  const int src = pass & 1, dst = src ^ 1;
  const unsigned* key = a.key[src];
  const unsigned* val = a.val[src];
  const int64_t base = (int64_t)blockIdx.x * YFV2_AP_TILE + (int64_t)wave * AP_WAVE_ITEMS + lane;
  unsigned k[AP_ROUNDS], v[AP_ROUNDS];
  int d[AP_ROUNDS];
#pragma unroll
  for (int r = 0; r < AP_ROUNDS; ++r) {
    const int64_t p = base + (int64_t)r * 64;
    k[r] = 0; v[r] = 0; d[r] = -1;
    if (p < a.N) {
      if (pass < 4) k[r] = key[p];
      v[r] = val[p];
      d[r] = ap_digit(a, pass, k[r], v[r], s_present);
      atomicAdd(&s_cur[wave][d[r]], 1u);
    }
  }
  __syncthreads();
  {
    // thread = digit: where this tile's detections of the digit start (digits below it, then earlier tiles), then wave by wave
    unsigned off = a.hist[(size_t)tid * (size_t)a.nblk + blockIdx.x];
    for (int j = 0; j < 256; ++j) {
      const unsigned t = s_tot[j];
      if (j < tid) off += t;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned c = s_cur[w][tid];
      s_cur[w][tid] = off;
      off += c;
    }
  }
  __syncthreads();
  unsigned* kout = a.key[dst];
  unsigned* vout = a.val[dst];
#pragma unroll
  for (int r = 0; r < AP_ROUNDS; ++r) {
    const bool valid = d[r] >= 0;
    unsigned long long same = __ballot(valid);   // the lanes of this round whose digit equals mine
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool set = ((d[r] >> bit) & 1) != 0;
      const unsigned long long b = __ballot(valid && set);
      same &= set ? b : ~b;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    if (valid) {
      const size_t q = (size_t)s_cur[wave][d[r]] + (size_t)rank;   // < N by construction of the scanned table
      if (pass < 3) kout[q] = k[r];                                 // the class pass needs no key
      vout[q] = v[r];
    }
    __syncthreads();
    if (valid && rank == 0) s_cur[wave][d[r]] += (unsigned)__popcll(same);
    __syncthreads();
  }
}


// ---- K thresholds: the callers' masks in rank order, bits at and above K cleared
__global__ __launch_bounds__(AP_THREADS) void ap_permute_kernel(ApArgs a) {
  const int64_t q = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
  if (q >= a.N) return;
  const unsigned keep = a.K >= 32 ? ~0u : (1u << a.K) - 1u;
  a.pmask[q] = a.tpmask[a.val[1][q] & 0x7fffffffu] & keep;
}

// ---- one workgroup per class (MULTI: per class and threshold blockIdx.y): its ranked segment from the back, chunk by chunk
template <bool MULTI>
__global__ __launch_bounds__(AP_THREADS) void ap_curve_kernel(ApArgs a) {
  __shared__ unsigned s_tot[256];
  __shared__ int s_cnt[4 * AP_ROWS];
  __shared__ double s_max[4 * AP_ROWS];
  __shared__ double s_sum[4];
  __shared__ long long s_tp[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x;
  const int k = MULTI ? (int)blockIdx.y : 0;
  ApHead* head = a.head + k;
  const long long n_gt = a.head->n_gt[c];
  if (n_gt == 0) return;   // uniform: the class is absent, its outputs stay 0
  s_tot[tid] = a.N > 0 ? a.tot[tid] : 0u;
  __syncthreads();
  int64_t start = 0;
  for (int j = 0; j < c; ++j) start += s_tot[j];
  const int64_t n_p = s_tot[c];
  if (tid == 0) head->n_pred[c] = n_p;
  if (n_p == 0) return;    // uniform: p = r = ap = 0
  const unsigned* v = (MULTI ? a.pmask : a.val[1]) + start;
  const int sh = MULTI ? k : 31;   // where tp sits in a word of v

  long long total = 0;
  for (int64_t i = tid; i < n_p; i += AP_THREADS) total += (v[i] >> sh) & 1u;
  total = wave_fold(total);
  if (lane == 0) s_tp[wave] = total;
  __syncthreads();
  total = s_tp[0] + s_tp[1] + s_tp[2] + s_tp[3];

  const double den = (double)n_gt + 1e-16;
  const int64_t nch = (n_p + YFV2_AP_CH - 1) / YFV2_AP_CH;
  double* part = a.part + (int64_t)k * a.part_stride + (start / YFV2_AP_CH + c);
  const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  long long after = total;    // true positives up to the end of the current chunk
  double carry_env = 0.0;     // max of prec over every later chunk (prec >= 0: 0 is neutral)
  for (int64_t ch = nch - 1; ch >= 0; --ch) {
    const int64_t base = ch * YFV2_AP_CH + tid;
    bool valid[AP_ROWS];
    unsigned bit[AP_ROWS];
    unsigned long long m[AP_ROWS];
#pragma unroll
    for (int r = 0; r < AP_ROWS; ++r) {
      const int64_t pos = base + (int64_t)r * AP_THREADS;
      valid[r] = pos < n_p;
      bit[r] = valid[r] ? (v[pos] >> sh) & 1u : 0u;
      m[r] = __ballot(bit[r] != 0);
      if (lane == 0) s_cnt[r * 4 + wave] = __popcll(m[r]);
    }
    __syncthreads();
    int chunk_tp = 0;
#pragma unroll
    for (int j = 0; j < 4 * AP_ROWS; ++j) chunk_tp += s_cnt[j];
    const long long before = after - chunk_tp;
    long long tpc[AP_ROWS];
    double sfx[AP_ROWS];
#pragma unroll
    for (int r = 0; r < AP_ROWS; ++r) {
      const int kk = r * 4 + wave;
      int pre = 0;
#pragma unroll
      for (int j = 0; j < 4 * AP_ROWS; ++j) pre += j < kk ? s_cnt[j] : 0;
      tpc[r] = before + pre + __popcll(m[r] & le);
      const int64_t pos = base + (int64_t)r * AP_THREADS;
      double x = valid[r] ? (double)tpc[r] / (double)(pos + 1) : 0.0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_down(x, off, 64);
        if (lane + off < 64) x = fmax(x, o);
      }
      sfx[r] = x;   // max of prec over this lane and the later lanes of its wave's row
      if (lane == 0) s_max[kk] = x;
    }
    __syncthreads();
    double term[AP_ROWS];
    double chunk_max = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * AP_ROWS; ++j) chunk_max = fmax(chunk_max, s_max[j]);
#pragma unroll
    for (int r = 0; r < AP_ROWS; ++r) {
      const int kk = r * 4 + wave;
      double env = fmax(sfx[r], carry_env);
#pragma unroll
      for (int j = 0; j < 4 * AP_ROWS; ++j) env = j > kk ? fmax(env, s_max[j]) : env;
      term[r] = bit[r] ? ((double)tpc[r] / den - (double)(tpc[r] - 1) / den) * env : 0.0;
    }
    double t = term[0];
#pragma unroll
    for (int r = 1; r < AP_ROWS; ++r) t += term[r];
    t = wave_fold(t);
    if (lane == 0) s_sum[wave] = t;
    carry_env = fmax(carry_env, chunk_max);
    after = before;
    __syncthreads();
    if (tid == 0) part[ch] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
  }
  if (tid != 0) return;
  double ap = part[0];     // thread 0 wrote every chunk sum itself
#pragma unroll 8
  for (int64_t ch = 1; ch < nch; ++ch) ap += part[ch];
  head->ap[c] = ap;
  head->p[c] = (double)total / (double)n_p;
  head->r[c] = (double)total / den;
}

constexpr size_t ap_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

constexpr size_t ap_part_doubles(size_t n) { return ap_align((n / YFV2_AP_CH + 512) * sizeof(double)) / sizeof(double); }

// layout: [head x max(K, 1)][row totals 256][table 256 x nblk][chunk sums (N / 1024 + 512) x max(K, 1)][key 0][key 1][payload 0][payload 1]
// and, for K >= 1, [permuted mask].  K = 0 is the single-threshold form and asks for what it always did; K = 1 asks for 4 N bytes more.
size_t yfv2_ap_ws_bytes(int64_t N, int K) {
  const size_t n = (size_t)N, nblk = (n + YFV2_AP_TILE - 1) / YFV2_AP_TILE, sets = K > 1 ? (size_t)K : 1;
  return ap_align(sets * sizeof(ApHead)) + ap_align(256 * sizeof(uint32_t)) + ap_align(256 * nblk * sizeof(uint32_t)) +
         sets * ap_part_doubles(n) * sizeof(double) + (K > 0 ? 5 : 4) * ap_align(n * sizeof(uint32_t));
}

void yfv2_ap_carve(ApArgs& a, char* ws) {
  const size_t n = (size_t)a.N, nblk = (n + YFV2_AP_TILE - 1) / YFV2_AP_TILE, sets = a.K > 1 ? (size_t)a.K : 1;
  a.nblk = (int)nblk;
  a.head = reinterpret_cast<ApHead*>(ws); ws += ap_align(sets * sizeof(ApHead));
  a.tot = reinterpret_cast<uint32_t*>(ws); ws += ap_align(256 * sizeof(uint32_t));
  a.hist = reinterpret_cast<uint32_t*>(ws); ws += ap_align(256 * nblk * sizeof(uint32_t));
  a.part = reinterpret_cast<double*>(ws); a.part_stride = (int64_t)ap_part_doubles(n); ws += sets * ap_part_doubles(n) * sizeof(double);
  for (int i = 0; i < 2; ++i) { a.key[i] = reinterpret_cast<uint32_t*>(ws); ws += ap_align(n * sizeof(uint32_t)); }
  for (int i = 0; i < 2; ++i) { a.val[i] = reinterpret_cast<uint32_t*>(ws); ws += ap_align(n * sizeof(uint32_t)); }
  a.pmask = a.K > 0 ? reinterpret_cast<uint32_t*>(ws) : nullptr;
}

void yfv2_launch_ap(const ApArgs& a, hipStream_t s) {
  (void)hipMemsetAsync(a.head, 0, (a.K > 1 ? (size_t)a.K : 1) * sizeof(ApHead), s);
  if (a.T > 0) {
    const int64_t blocks = (a.T + AP_THREADS * 8 - 1) / (AP_THREADS * 8);
    hipLaunchKernelGGL(ap_targets_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(AP_THREADS), 0, s, a);
  }
  if (a.N > 0) {
    hipLaunchKernelGGL(ap_prep_kernel, dim3((unsigned)((a.N + AP_THREADS - 1) / AP_THREADS)), dim3(AP_THREADS), 0, s, a);
    for (int pass = 0; pass < 5; ++pass) {
      hipLaunchKernelGGL(ap_hist_kernel, dim3((unsigned)a.nblk), dim3(AP_THREADS), 0, s, a, pass);
      hipLaunchKernelGGL(ap_scan_kernel, dim3(256), dim3(AP_THREADS), 0, s, a);
      hipLaunchKernelGGL(ap_scatter_kernel, dim3((unsigned)a.nblk), dim3(AP_THREADS), 0, s, a, pass);
    }
  }
  if (a.K > 0) {
    if (a.N > 0) hipLaunchKernelGGL(ap_permute_kernel, dim3((unsigned)((a.N + AP_THREADS - 1) / AP_THREADS)), dim3(AP_THREADS), 0, s, a);
    hipLaunchKernelGGL(ap_curve_kernel<true>, dim3(255, (unsigned)a.K), dim3(AP_THREADS), 0, s, a);
  } else {
    hipLaunchKernelGGL(ap_curve_kernel<false>, dim3(255), dim3(AP_THREADS), 0, s, a);
  }
}

void yfv2_ap_finish(const ApHead& head, yfv2_ap_result* out) {
  int present = 0;
  double sp = 0.0, sr = 0.0, sa = 0.0, sf = 0.0;
  for (int c = 0; c < 256; ++c) {
    out->n_gt[c] = head.n_gt[c]; out->n_pred[c] = head.n_pred[c];
    out->p[c] = head.p[c]; out->r[c] = head.r[c]; out->ap[c] = head.ap[c];
    if (c == 255 || head.n_gt[c] == 0) continue;
    ++present;
    const double p = head.p[c], r = head.r[c];
    sp += p; sr += r; sa += head.ap[c];
    sf += 2 * p * r / (p + r + 1e-16);          // utils.py:190
  }
  out->classes_present = present;
  out->bad_input = head.bad ? 1 : 0;
  const double n = (double)present;              // 0 / 0 = NaN for an empty target list: np.mean([])
  out->mean_p = sp / n; out->mean_r = sr / n; out->mean_ap = sa / n; out->mean_f1 = sf / n;
}

void yfv2_ap_finish_multi(ApHead* heads, int K, yfv2_ap_result* out) {
  for (int k = 0; k < K; ++k) {
    if (k > 0) {
      for (int c = 0; c < 256; ++c) heads[k].n_gt[c] = heads[0].n_gt[c];
      heads[k].bad = heads[0].bad;
    }
    yfv2_ap_finish(heads[k], out + k);
  }
}
