// yfv2_pack.hip - the host-side weight packer (yfv2_pack.h): BatchNorm folding and the packed image of every kernel.
// Host only: no kernel, no HIP runtime call.  Every packing rule is stated once, in the helpers at the top; the layout
// comment above an image_* function is the specification of that kernel's image (the host-model tests decode the images
// from these comments alone).
#include "yfv2_pack.h"

#include <cmath>

#include "yfv2_internal.h"

namespace {

// ---------------------------------------------------------------------------
// number formats and scaling
// ---------------------------------------------------------------------------
float rn_f16(float v) { return (float)(_Float16)v; }
unsigned f16_bits(float v) { const _Float16 h = (_Float16)v; unsigned short u; std::memcpy(&u, &h, 2); return u; }
unsigned bf16_trunc_bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u >> 16; }
float bf16_trunc(float v) { unsigned u; std::memcpy(&u, &v, 4); u &= 0xffff0000u; float r; std::memcpy(&r, &u, 4); return r; }
int pow2_for(float mx) {   // sw with mx * 2^sw in (2^13, 2^14]
  if (!(mx > 0.f) || !std::isfinite(mx)) return 0;
  int sw = 14 - (int)std::ceil(std::log2(mx));
  return sw > 24 ? 24 : (sw < -14 ? -14 : sw);
}
template <class Fn>
float max_abs(int M, int K, Fn el) {   // max |el(r, c)| over M x K
  float mx = 0.f;
  for (int r = 0; r < M; ++r)
    for (int c = 0; c < K; ++c) mx = std::fmax(mx, std::fabs(el(r, c)));
  return mx;
}
float max_abs(const float* w, int n) { return max_abs(1, n, [&](int, int i) { return w[i]; }); }

// The two-term fp16 split: v = h1 + h2 to 2^-24 with h1 = RN16(v), h2 = RN16(v - h1) (v - h1 is exact in fp32).  One dword
// of an operand = term `term` of two neighbouring values, low half first.
unsigned f16_term_pair(float v0, float v1, int term) {
  const float v[2] = {v0, v1};
  unsigned packed = 0;
  for (int e = 0; e < 2; ++e) {
    const float h1 = rn_f16(v[e]);
    packed |= f16_bits(term == 0 ? h1 : v[e] - h1) << (16 * e);
  }
  return packed;
}

// A operands of v_mfma_f32_16x16x32_f16 as two fp16 terms: [tile][chunk][term 2][64 lanes][4 dwords].  Lane 16 g + i holds
// row 16 tile + i and the eight K slots q = 8 chunk .. 8 chunk + 7 of its group g, two per dword; el(row, g, q) is the value
// (already carrying its power of two) that belongs there.  The images differ only in what a (g, q) means.
template <class Fn>
void push_f16_terms(std::vector<float>& im, int tiles, int chunks, Fn el) {
  for (int t = 0; t < tiles; ++t)
    for (int c = 0; c < chunks; ++c)
      for (int term = 0; term < 2; ++term)
        for (int l = 0; l < 64; ++l)
          for (int d = 0; d < 4; ++d) {
            const int r = 16 * t + (l & 15), g = l >> 4, q = 8 * c + 2 * d;
            WeightPacker::push_bits(im, f16_term_pair(el(r, g, q), el(r, g, q + 1), term));
          }
}
// K slot q of lane group g on a plain row-major matrix: column 16 (q / 4) + 4 g + q % 4.  A chunk (8 slots) is a PAIR of
// 16-column chunks of the fp32 fragment order: dwords 0, 1 = columns 4g..4g+3 of the pair's first chunk, 2, 3 = of its second.
int k_col(int g, int q) { return 16 * (q >> 2) + 4 * g + (q & 3); }
// an M x K matrix el(row, column) in that order, MT row tiles x KP chunk pairs, zero outside M x K
template <class Fn>
void push_f16_matrix(std::vector<float>& im, int M, int K, int MT, int KP, Fn el) {
  push_f16_terms(im, MT, KP, [&](int r, int g, int q) { const int c = k_col(g, q); return (r < M && c < K) ? el(r, c) : 0.f; });
}

// fragment-major fp32 filter: frag (mt, s), lane l -> el(16mt + (l&15), 16s + 4(l>>4) .. +3)
template <class Fn>
void push_frag_fn(std::vector<float>& im, int MT, int KC, Fn el) {
  for (int mt = 0; mt < MT; ++mt)
    for (int s = 0; s < KC; ++s)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 4; ++j) im.push_back(el(16 * mt + (l & 15), 16 * s + 4 * (l >> 4) + j));
}
void push_frag(std::vector<float>& im, const float* w, int M, int K, int MT, int KC) {   // W [M][K], zero outside M x K
  push_frag_fn(im, MT, KC, [&](int r, int c) { return (r < M && c < K) ? w[(size_t)r * K + c] : 0.f; });
}
void push_rows(std::vector<float>& im, const float* w, int nrows, int C, int KS) {  // [nrows][C] -> [nrows][KS]
  for (int r = 0; r < nrows; ++r)
    for (int c = 0; c < KS; ++c) im.push_back(c < C ? w[(size_t)r * C + c] : 0.f);
}
void push_vec(std::vector<float>& im, const float* v, int n, int padded) {
  for (int i = 0; i < padded; ++i) im.push_back((v && i < n) ? v[i] : 0.f);
}

// The BN shift of a depthwise conv goes through the pointwise conv behind it (both linear): the pointwise conv's bias for
// output row `wrow` is shift + scale * (W . depthwise shift), the dot product in double.
float bias_through_pw(const float* wrow, int K, float scale, float shift, const float* dw_shift) {
  double acc = 0;
  for (int k = 0; k < K; ++k) acc += (double)wrow[k] * dw_shift[k];
  return shift + scale * (float)acc;
}

// Depthwise 3x3 taps (BN scale folded, times 2^shift_pow2) in the lane order of the f16 streaming kernels (yfv2_stage2h.hip):
// [9 S / 4][64], S = K slots a lane owns (8 of which some are empty at 24 channels, C / 4 at 48 and 96).  Lane (l, g),
// register q' holds tap f = 4q' + (l & 3) = cs * 9 + dy * 3 + dx of the lane's channel slot cs = channel k_col(g, cs); zero
// where that is no channel.  wd = [9][C], scd = [C].
void push_lane_taps(std::vector<float>& im, const float* wd, const float* scd, int C, int shift_pow2) {
  const int S = C == 24 ? 8 : C / 4;
  for (int q = 0; q < 9 * S / 4; ++q)
    for (int l = 0; l < 64; ++l) {
      const int f = 4 * q + (l & 3), cs = f / 9, tt = f % 9, n = k_col(l >> 4, cs);
      im.push_back(n < C ? std::ldexp(wd[(size_t)tt * C + n] * scd[n], shift_pow2) : 0.f);
    }
}

// block_s1chain6_kernel: a 48x48 filter x 2^sw as two fp16 terms (w1 = RN16, w2 = RN16 of the rest), [mt (3)][three 16-byte
// operands][64 lanes][4 dwords]: {w1 chunk 0, w1 chunk 1}, {w2 chunk 0, w2 chunk 1}, {w1 chunk 2, w2 chunk 2}; a lane's two
// dwords of a chunk = K positions 4g..4g+3.  Returns sw.
int push_chain6_filter(std::vector<float>& im, const float* w /* [48][48] */) {
  const int sw = pow2_for(max_abs(w, 48 * 48));
  auto term = [&](int r, int c, int t) {               // packed (value c, value c + 1) of row r, fp16 term t
    return f16_term_pair(std::ldexp(w[(size_t)r * 48 + c], sw), std::ldexp(w[(size_t)r * 48 + c + 1], sw), t);
  };
  for (int mt = 0; mt < 3; ++mt)
    for (int op = 0; op < 3; ++op)
      for (int l = 0; l < 64; ++l)
        for (int d = 0; d < 4; ++d) {
          const int r = 16 * mt + (l & 15), kq = 4 * (l >> 4) + 2 * (d & 1);
          if (op < 2) WeightPacker::push_bits(im, term(r, 16 * (d >> 1) + kq, op));   // the pair: dwords 0, 1 = chunk 0, dwords 2, 3 = chunk 1
          else WeightPacker::push_bits(im, term(r, 32 + kq, d >> 1));                 // chunk 2: dwords 0, 1 = first term, 2, 3 = second
        }
  return sw;
}

// block_s2w_kernel's W1 pre-split for bf16x6: an fp32 weight is the exact sum of three truncated bf16 terms (hi, mid, lo).
// Per (tile of 16 output channels mt, PAIR of 16-channel chunks sp, term) one 16-byte lane quad: {term(w0),term(w1)}
// {term(w2),term(w3)} of chunk 2sp, then the same of chunk 2sp+1 - the A operand of one v_mfma_f32_16x16x32_bf16 whose 32
// k-slots are the two chunks.
void push_frag_split3(std::vector<float>& im, const float* w, int M, int K, int MT, int KC) {
  for (int mt = 0; mt < MT; ++mt)
    for (int sp = 0; sp < KC / 2; ++sp)
      for (int term = 0; term < 3; ++term)
        for (int l = 0; l < 64; ++l)
          for (int d = 0; d < 4; ++d) {
            const int r = 16 * mt + (l & 15), c = k_col(l >> 4, 8 * sp + 2 * d);
            unsigned packed = 0;
            for (int e = 0; e < 2; ++e) {
              float v = (r < M && c + e < K) ? w[(size_t)r * K + c + e] : 0.f;
              for (int t = 0; t < term; ++t) v = v - bf16_trunc(v);   // exact in fp32
              packed |= bf16_trunc_bits(v) << (16 * e);
            }
            WeightPacker::push_bits(im, packed);
          }
}

// towerh_kernel's A operands: [tile][chunk 5][64 lanes][4 dwords of fp16 pairs: term 1, term 1, term 2, term 2] of the
// lane's FOUR columns 16 s + 4 g .. + 3 (one 16-column chunk per operand); el(row, col) already scaled
template <class Fn>
void push_a16(std::vector<float>& im, Fn el, int MT) {
  for (int mt = 0; mt < MT; ++mt)
    for (int s = 0; s < 5; ++s)
      for (int l = 0; l < 64; ++l) {
        float v[4];
        for (int e = 0; e < 4; ++e) v[e] = el(16 * mt + (l & 15), 16 * s + 4 * (l >> 4) + e);
        for (int d = 0; d < 4; ++d) WeightPacker::push_bits(im, f16_term_pair(v[2 * (d & 1)], v[2 * (d & 1) + 1], d >> 1));
      }
}

// ---- stage 2 in lane-per-pixel form (yfv2_stage2.hip)
// pointwise 24->24 in the 4x4x1 broadcast form [10][64]: register q, lane 4j+i holds entry (m, k) of
// output position 4m+i, (m*25 + k) = 16q + j; k = 24 is the bias column.  row(n) / col(k) give the
// filter row / column of output position n / input position k.
template <class RowFn, class ColFn, class BiasFn>
void push_pw24_bcast(std::vector<float>& im, RowFn row, ColFn col, BiasFn bias, const float* w, const float* scale) {
  const size_t base = im.size();
  im.resize(base + 640, 0.f);
  for (int m = 0; m < 6; ++m)
    for (int i = 0; i < 4; ++i) {
      const int r = row(4 * m + i);
      for (int k = 0; k < 25; ++k) {
        const int idx = m * 25 + k;
        im[base + (idx >> 4) * 64 + 4 * (idx & 15) + i] = k < 24 ? w[(size_t)r * 24 + col(k)] * scale[r] : bias(r);
      }
    }
}
// depthwise 3x3 taps of 24 channels, BN scale folded: [54][64], lane&3 = k of register q holds tap 4q+k, flat index c*9 + dy*3 + dx
void push_taps_quad(std::vector<float>& im, const float* wd, const float* scd) {
  const size_t base = im.size();
  im.resize(base + 54 * 64, 0.f);
  for (int c = 0; c < 24; ++c)
    for (int t = 0; t < 9; ++t) {
      const int f = c * 9 + t;
      for (int quad = 0; quad < 16; ++quad) im[base + (f >> 2) * 64 + 4 * quad + (f & 3)] = wd[(size_t)t * 24 + c] * scd[c];
    }
}

// ---- s1h_kernel / s2h_kernel (yfv2_stage2h.hip): lane (l, g = lane >> 4) owns channel POSITIONS npos(g, j), j = 0..7: 4g + j
// for j < 4 (channel tile 0), 16 + 4g + (j - 4) for j >= 4 and g < 2 (tile 1), none otherwise - as K slots of the B operand
// and as rows 4g..4g+3 of the D tiles alike.
int s1h_npos(int g, int j) { return j < 4 ? 4 * g + j : (g < 2 ? 16 + 4 * g + (j - 4) : -1); }
// a 24 x 24 filter el(row position, K position) -> [tile 2][term 2][64][4 dwords] of fp16 pairs
template <class Fn>
void push_h3_filter(std::vector<float>& im, Fn el) {
  push_f16_terms(im, 2, 1, [&](int r, int g, int j) { const int n = s1h_npos(g, j); return (n >= 0 && r < 24) ? el(r, n) : 0.f; });
}
// per-lane table [4][64] of a value per pair the lane owns: pair 2g + k for k < 2, 8 + 2g + (k - 2) for k >= 2 and g < 2, else
// the NONE mark (the pairs of positions s1h_npos(g, 2k), + 1)
const int LANE_NONE = (int)0x80000000;
template <class Fn>
void push_lane_pairs(std::vector<float>& im, Fn value) {
  for (int k = 0; k < 4; ++k)
    for (int l = 0; l < 64; ++l) {
      const int g = l >> 4, kk = k < 2 ? 2 * g + k : (g < 2 ? 8 + 2 * g + (k - 2) : -1);
      WeightPacker::push_bits(im, kk < 0 ? LANE_NONE : value(kk));
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// weights: reference state_dict -> one blob of kernel-ready parameters
// ---------------------------------------------------------------------------
// element count of every floating-point state_dict entry of the architecture (model/detector.py:8-19 and the modules it builds:
// shufflenetv2.py:19-46,66-100, fpn.py:5-49) for this configuration
std::map<std::string, int64_t> expected_numels(const yfv2_config& cfg) {
  std::map<std::string, int64_t> m;
  auto conv = [&](const std::string& n, int co, int ci_per_group, int k) { m[n + ".weight"] = (int64_t)co * ci_per_group * k * k; };
  auto bn = [&](const std::string& n, int c) { for (const char* leaf : {".weight", ".bias", ".running_mean", ".running_var"}) m[n + leaf] = c; };
  conv("backbone.first_conv.0", 24, 3, 3); bn("backbone.first_conv.1", 24);
  const int repeats[3] = {4, 8, 4}, chans[4] = {24, 48, 96, 192};
  int cin = 24;
  for (int si = 0; si < 3; ++si) {
    const int cout = chans[si + 1], mid = cout / 2;
    for (int i = 0; i < repeats[si]; ++i) {
      const std::string p = "backbone.stage" + std::to_string(si + 2) + "." + std::to_string(i);
      const int inp = i == 0 ? cin : cin / 2;
      conv(p + ".branch_main.0", mid, inp, 1); bn(p + ".branch_main.1", mid);
      conv(p + ".branch_main.3", mid, 1, 3); bn(p + ".branch_main.4", mid);
      conv(p + ".branch_main.5", cout - inp, mid, 1); bn(p + ".branch_main.6", cout - inp);
      if (i == 0) {
        conv(p + ".branch_proj.0", inp, 1, 3); bn(p + ".branch_proj.1", inp);
        conv(p + ".branch_proj.2", inp, inp, 1); bn(p + ".branch_proj.3", inp);
      }
      cin = cout;
    }
  }
  conv("fpn.conv1x1_2.0", 72, 288, 1); bn("fpn.conv1x1_2.1", 72);
  conv("fpn.conv1x1_3.0", 72, 192, 1); bn("fpn.conv1x1_3.1", 72);
  for (const char* head : {"cls_head_2", "reg_head_2", "reg_head_3", "cls_head_3"}) {
    const std::string p = std::string("fpn.") + head + ".block";
    conv(p + ".0", 72, 1, 5); bn(p + ".1", 72); conv(p + ".3", 72, 72, 1); bn(p + ".4", 72);
    conv(p + ".5", 72, 1, 5); bn(p + ".6", 72); conv(p + ".8", 72, 72, 1); bn(p + ".9", 72);
  }
  const int A = cfg.anchor_num;
  const std::pair<const char*, int> outs[3] = {{"output_reg_layers", 4 * A}, {"output_obj_layers", A}, {"output_cls_layers", cfg.classes}};
  for (const auto& o : outs) { m[std::string(o.first) + ".weight"] = (int64_t)o.second * 72; m[std::string(o.first) + ".bias"] = o.second; }
  return m;
}
bool WeightPacker::index(const yfv2_config& cfg, const yfv2_tensor_desc* tensors, int32_t n) {
  for (int i = 0; i < n; ++i)
    if (tensors[i].name) byname[tensors[i].name] = &tensors[i];
  for (const auto& [name, numel] : expected_numels(cfg)) {
    auto it = byname.find(name);
    if (it == byname.end() || it->second->data == nullptr) missing = "missing tensor '" + name + "'";
    else if (it->second->numel != numel)
      missing = "tensor '" + name + "' has " + std::to_string(it->second->numel) + " elements, expected " + std::to_string(numel);
    if (!missing.empty()) return false;
  }
  return true;
}
// eval-mode BatchNorm2d -> y = x*scale + shift  (ATen: alpha = gamma*invstd, beta = bias - mean*alpha)
void WeightPacker::bn(const std::string& name, int c, Folded* f) {
  const float* g = get(name + ".weight");
  const float* b = get(name + ".bias");
  const float* m = get(name + ".running_mean");
  const float* v = get(name + ".running_var");
  f->scale = reserve(c);
  f->shift = reserve(c);
  for (int i = 0; i < c; ++i) {
    const float invstd = 1.0f / std::sqrt(v[i] + 1e-5f);
    const float alpha = g[i] * invstd;
    blob[f->scale + i] = alpha;
    blob[f->shift + i] = b[i] - m[i] * alpha;
  }
}
// pointwise conv weight (co, ci, 1, 1) is already the [M][K] row-major A operand
void WeightPacker::pw(const std::string& conv, const std::string& bnname, int co, int ci, Folded* f) {
  const float* w = get(conv + ".weight");
  f->w = reserve((size_t)co * ci);
  std::memcpy(&blob[f->w], w, sizeof(float) * co * ci);
  bn(bnname, co, f);
}
// depthwise weight (C,1,k,k) -> [k*k][C] so that a channel quad is one 16-byte load
void WeightPacker::dw(const std::string& conv, const std::string& bnname, int c, int k, Folded* f) {
  const float* w = get(conv + ".weight");
  f->w = reserve((size_t)c * k * k);
  for (int ch = 0; ch < c; ++ch)
    for (int t = 0; t < k * k; ++t) blob[f->w + (size_t)t * c + ch] = w[(size_t)ch * k * k + t];
  bn(bnname, c, f);
}
// stem weight (24,3,3,3) -> [27 taps][24 co]
void WeightPacker::stem(const std::string& conv, const std::string& bnname, Folded* f) {
  const float* w = get(conv + ".weight");
  f->w = reserve(24 * 27);
  for (int co = 0; co < 24; ++co)
    for (int t = 0; t < 27; ++t) blob[f->w + (size_t)t * 24 + co] = w[co * 27 + t];
  bn(bnname, 24, f);
}
// biased output convs: rows of several (co_i, 72) matrices stacked; scale = 1, shift = bias
void WeightPacker::heads(const std::vector<std::pair<std::string, int>>& parts, int ci, Folded* f) {
  int total = 0;
  for (auto& p : parts) total += p.second;
  f->w = reserve((size_t)total * ci);
  f->scale = reserve(total);
  f->shift = reserve(total);
  int row = 0;
  for (auto& p : parts) {
    const float* w = get(p.first + ".weight");
    const float* b = get(p.first + ".bias");
    std::memcpy(&blob[f->w + (size_t)row * ci], w, sizeof(float) * p.second * ci);
    for (int i = 0; i < p.second; ++i) {
      blob[f->scale + row + i] = 1.0f;
      blob[f->shift + row + i] = b[i];
    }
    row += p.second;
  }
}
// rows [r0, r0 + n) of one biased output conv (the class head of a model with more classes than one launch's 96 rows)
void WeightPacker::heads_range(const std::string& name, int r0, int n, int ci, Folded* f) {
  const float* w = get(name + ".weight");
  const float* b = get(name + ".bias");
  f->w = reserve((size_t)n * ci); f->scale = reserve(n); f->shift = reserve(n);
  std::memcpy(&blob[f->w], w + (size_t)r0 * ci, sizeof(float) * n * ci);
  for (int i = 0; i < n; ++i) { blob[f->scale + i] = 1.0f; blob[f->shift + i] = b[r0 + i]; }
}
// columns [c0, c0 + n) of a folded conv's filter as a conv of its own (same BN scale / shift)
Folded WeightPacker::pw_columns(const Folded& f, int co, int ci, int c0, int n) {
  Folded g = f;
  g.w = reserve((size_t)co * n);
  for (int r = 0; r < co; ++r)
    for (int k = 0; k < n; ++k) blob[g.w + (size_t)r * n + k] = blob[f.w + (size_t)r * ci + c0 + k];
  return g;
}
// copies with the INPUT channels re-ordered: position k takes logical channel label[k]
Folded WeightPacker::permuted_pw_inputs(const Folded& f, int co, int ci, const int* label) {
  Folded g = f;
  g.w = reserve((size_t)co * ci);
  for (int r = 0; r < co; ++r)
    for (int k = 0; k < ci; ++k) blob[g.w + (size_t)r * ci + k] = blob[f.w + (size_t)r * ci + label[k]];
  return g;
}
// copy with the OUTPUT channels re-ordered: row r (and its BN scale / shift) takes logical output channel label[r]
Folded WeightPacker::permuted_pw_outputs(const Folded& f, int co, int ci, const int* label) {
  Folded g;
  g.w = reserve((size_t)co * ci); g.scale = reserve(co); g.shift = reserve(co);
  for (int r = 0; r < co; ++r) {
    for (int k = 0; k < ci; ++k) blob[g.w + (size_t)r * ci + k] = blob[f.w + (size_t)label[r] * ci + k];
    blob[g.scale + r] = blob[f.scale + label[r]];
    blob[g.shift + r] = blob[f.shift + label[r]];
  }
  return g;
}
Folded WeightPacker::permuted_dw_channels(const Folded& f, int c, int kk, const int* label) {
  Folded g;
  g.w = reserve((size_t)c * kk); g.scale = reserve(c); g.shift = reserve(c);
  for (int k = 0; k < c; ++k) {
    for (int t = 0; t < kk; ++t) blob[g.w + (size_t)t * c + k] = blob[f.w + (size_t)t * c + label[k]];
    blob[g.scale + k] = blob[f.scale + label[k]];
    blob[g.shift + k] = blob[f.shift + label[k]];
  }
  return g;
}

// ---------------------------------------------------------------------------
// images
// ---------------------------------------------------------------------------
// stem_px_kernel: filter registers in the 4x4x1 broadcast form [11][64]: register q, lane 4j+i holds
// scale[co] * W[co = 4m+i][k] for (m*27 + k) = 16q + j, k = ky*9 + ci*3 + kx; then shift[24]
// in_scale: 1 for fp32 input in [0,1]; 1/255 for the uint8 entry points (test.py:38's float()/255 folded into the filter)
size_t WeightPacker::image_stem(const Folded& f, float in_scale) {
  std::vector<float> im(11 * 64 + 24, 0.f);
  const float* w = &blob[f.w];  // [27 taps t = ci*9 + ky*3 + kx][24 co]
  for (int idx = 0; idx < 162; ++idx)
    for (int i = 0; i < 4; ++i) {
      const int co = 4 * (idx / 27) + i, k = idx % 27, ky = k / 9, ci = (k % 9) / 3, kx = k % 3;
      im[(idx >> 4) * 64 + 4 * (idx & 15) + i] = w[(ci * 9 + ky * 3 + kx) * 24 + co] * blob[f.scale + co] * in_scale;
    }
  for (int co = 0; co < 24; ++co) im[11 * 64 + co] = blob[f.shift + co];
  return put(im);
}
// stem_h3_kernel (yfv2_stem16.hip): the BN-folded filter times 2^sw as TWO fp16 terms (w = h1 + h2 to 2^-24, round to
// nearest) in the A-operand order of v_mfma_f32_16x16x32_f16: [channel tile 2][term 2][lane 64][dword 4], lane = 16 g + r
// holds output channel 16 t + r, K slots 8 g .. 8 g + 7, two halves per dword (low half = even slot).  Slot -> tap:
//   g < 3 (input channel g): (ky,kx) = (0,1) (0,2) (1,1) (1,2) (0,0) (1,0) (2,0) (2,1);   g = 3: slots 2, 3, 7 = tap (2,2)
//   of input channels 0, 1, 2, the rest zero.       Then shift * 2^(sw+8) [32 channels, zero beyond 24] and 2^-(sw+8).
size_t WeightPacker::image_stem16(const Folded& f) {
  const float* w = &blob[f.w];   // [27 taps t = ci*9 + ky*3 + kx][24 co]
  auto folded = [&](int co, int ci, int ky, int kx) { return w[(ci * 9 + ky * 3 + kx) * 24 + co] * blob[f.scale + co]; };
  const int sw = pow2_for(max_abs(24, 27, [&](int co, int t) { return w[t * 24 + co] * blob[f.scale + co]; }));
  const float up = std::ldexp(1.0f, sw);
  static const int TAP[8][2] = {{0, 1}, {0, 2}, {1, 1}, {1, 2}, {0, 0}, {1, 0}, {2, 0}, {2, 1}};
  std::vector<float> im;
  push_f16_terms(im, 2, 1, [&](int co, int g, int j) -> float {
    if (co >= 24) return 0.f;
    if (g < 3) return folded(co, g, TAP[j][0], TAP[j][1]) * up;
    if (j == 2) return folded(co, 0, 2, 2) * up;
    if (j == 3) return folded(co, 1, 2, 2) * up;
    if (j == 7) return folded(co, 2, 2, 2) * up;
    return 0.f;
  });
  // the kernel scales the image by 2^8 before splitting it (yfv2_stem16.hip): accumulators carry 2^(sw+8)
  for (int co = 0; co < 32; ++co) im.push_back(co < 24 ? std::ldexp(blob[f.shift + co], sw + 8) : 0.f);
  im.push_back(std::ldexp(1.0f, -(sw + 8)));
  while (im.size() % 4) im.push_back(0.f);
  // stem_h3u_kernel (uint8 pixels 0..255 as they are, one exact fp16 term): accumulators carry 2^sw 255
  for (int co = 0; co < 32; ++co) im.push_back(co < 24 ? (float)(std::ldexp((double)blob[f.shift + co], sw) * 255.0) : 0.f);
  im.push_back((float)(std::ldexp(1.0, -sw) / 255.0));
  while (im.size() % 4) im.push_back(0.f);
  return put(im);
}
// pw_kernel: filter fragments [MT][K/16][64 lanes][4] (+ an 8-channel tail [MT][64 lanes][2]), scale[MT*16], shift[MT*16]
size_t WeightPacker::image_pw(const Folded& f, int M, int K, int MT, bool presplit) {
  std::vector<float> im;
  build_pw(im, f, M, K, MT, presplit);
  return put(im);
}
// PW_DUAL: two convs on the same input as ONE image of 2 MT output tiles - fragments of the first, fragments of the second (each filter
// with its own power-of-two scale), then scale[2 MT 16], shift[2 MT 16]
size_t WeightPacker::image_pw_dual(const Folded& f0, const Folded& f1, int M, int K, int MT) {
  std::vector<float> i0, i1, im;
  build_pw(i0, f0, M, K, MT, true);
  build_pw(i1, f1, M, K, MT, true);
  const size_t fr = i0.size() - 2 * (size_t)MT * 16, r = (size_t)MT * 16;
  im.insert(im.end(), i0.begin(), i0.begin() + fr);
  im.insert(im.end(), i1.begin(), i1.begin() + fr);
  im.insert(im.end(), i0.begin() + fr, i0.begin() + fr + r);
  im.insert(im.end(), i1.begin() + fr, i1.begin() + fr + r);
  im.insert(im.end(), i0.begin() + fr + r, i0.end());
  im.insert(im.end(), i1.begin() + fr + r, i1.end());
  return put(im);
}
void WeightPacker::build_pw(std::vector<float>& im, const Folded& f, int M, int K, int MT, bool presplit) {
  const int rows = MT * 16, K16 = K / 16;
  const float* w = &blob[f.w];
  int sw = 0;
  if (presplit) {
    // pw_kernel<.., PRE>: the filter x 2^sw as two fp16 terms, [mt][chunk pair][term][64 lanes][4 dwords]: dwords 0,1 = K
    // positions 4g..4g+3 of the pair's first chunk, 2,3 = of its second (one A operand of v_mfma_f32_16x16x32_f16)
    sw = pow2_for(max_abs(w, M * K));
    push_f16_matrix(im, M, K, MT, K16 / 2, [&](int r, int c) { return std::ldexp(w[(size_t)r * K + c], sw); });
  } else {
    push_frag(im, w, M, K, MT, K16);
  }
  if (K % 16)
    for (int mt = 0; mt < MT; ++mt)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 2; ++j) {
          const int r = 16 * mt + (l & 15), c = 16 * K16 + 2 * (l >> 4) + j;
          im.push_back((r < M && c < K) ? w[(size_t)r * K + c] : 0.f);
        }
  if (presplit) for (int i = 0; i < rows; ++i) im.push_back(i < M ? std::ldexp(blob[f.scale + i], -(sw + 4)) : 0.f);   // the accumulators carry 2^(sw+4): undone exactly inside the BN scale
  else push_vec(im, &blob[f.scale], M, rows);
  push_vec(im, &blob[f.shift], M, rows);
}
// block_s1chain6_kernel, one block: W1 | W2 (push_chain6_filter) | dw taps [9][48] | sc1 sh1 scd shd sc2 sh2 [48]
void WeightPacker::append_s1_bf6(std::vector<float>& im, const Folded& f1, const Folded& fd, const Folded& f2) {
  const int sw1 = push_chain6_filter(im, &blob[f1.w]);
  const int sw2 = push_chain6_filter(im, &blob[f2.w]);
  push_rows(im, &blob[fd.w], 9, 48, 48);
  for (const Folded* f : {&f1, &fd, &f2}) {
    const int un = f == &f1 ? sw1 + 4 : (f == &f2 ? sw2 + 4 : 0);   // the pointwise accumulators carry 2^(sw+4): undone exactly inside the BN scale
    for (int i = 0; i < 48; ++i) im.push_back(std::ldexp(blob[f->scale + i], -un));
    push_vec(im, &blob[f->shift], 48, 48);
  }
}
// ---- a chain of stride-1 blocks with the whole activation resident in LDS (block_s1pool_kernel, yfv2_block.hip): natural
// channel order, so the only host work is cutting every block's filters into the three 32-channel passes the kernel runs:
// per pass W1 rows 32 t .. +31 (fragment-major [2][6][64][4]) | W2 columns 32 t .. +31 ([6][2][64][4]) | depthwise taps
// [9][32] | sc1 sh1 scd shd [32] | sc2 sh2 [96].  pre (block_s1pool_kernel<.., PRE>: fp16x3): W1 / W2 x 2^sw as two fp16
// terms per chunk pair ([2][3][2][64][4] | [6][1][2][64][4]), one power of two per filter; sc1 / sc2 carry the exact 2^-(sw+4)
size_t WeightPacker::image_s1pool(const std::vector<Folded>& f1s, const std::vector<Folded>& fds, const std::vector<Folded>& f2s, int c2, bool pre, bool* ok) {
  std::vector<float> im;
  for (size_t k = 0; k < f1s.size(); ++k) {
    const Folded &f1 = f1s[k], &fd = fds[k], &f2 = f2s[k];
    const float* w1 = &blob[f1.w]; const float* w2 = &blob[f2.w]; const float* wd = &blob[fd.w];
    const int sw1 = pre ? pow2_for(max_abs(w1, c2 * c2)) : 0, sw2 = pre ? pow2_for(max_abs(w2, c2 * c2)) : 0;
    const int un1 = pre ? sw1 + 4 : 0, un2 = pre ? sw2 + 4 : 0;
    for (int t = 0; t < 3; ++t) {
      const size_t start = im.size();
      auto e1 = [&](int r, int c) { return w1[(size_t)(32 * t + r) * c2 + c]; };    // W1 rows 32 t .. +31, K = 96
      auto e2 = [&](int r, int c) { return w2[(size_t)r * c2 + 32 * t + c]; };      // W2 columns 32 t .. +31
      if (pre) {
        push_f16_matrix(im, 32, c2, 2, 3, [&](int r, int c) { return std::ldexp(e1(r, c), sw1); });
        push_f16_matrix(im, c2, 32, 6, 1, [&](int r, int c) { return std::ldexp(e2(r, c), sw2); });
      } else {
        push_frag_fn(im, 2, 6, e1);
        push_frag_fn(im, 6, 2, e2);
      }
      for (int tap = 0; tap < 9; ++tap)
        for (int ch = 0; ch < 32; ++ch) im.push_back(wd[(size_t)tap * c2 + 32 * t + ch]);
      for (const size_t* v : {&f1.scale, &f1.shift, &fd.scale, &fd.shift})
        for (int ch = 0; ch < 32; ++ch) im.push_back(v == &f1.scale ? std::ldexp(blob[*v + 32 * t + ch], -un1) : blob[*v + 32 * t + ch]);
      for (int ch = 0; ch < c2; ++ch) im.push_back(std::ldexp(blob[f2.scale + ch], -un2));
      for (int ch = 0; ch < c2; ++ch) im.push_back(blob[f2.shift + ch]);
      if ((int)(im.size() - start) != yfv2_s1pool_image_floats(pre)) *ok = false;
    }
  }
  return put(im);
}
// block_s2_kernel<CIN>: W1 | W2 | Wproj | main dw taps | proj dw taps | sc1 sh1 scd shd sc2 sh2 scpd shpd scpp shpp
// block_s2w_kernel (cin = 96, w1_split3): the same image with W1 pre-split for bf16x6 (push_frag_split3)
size_t WeightPacker::image_s2(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, int cin, bool w1_split3) {
  const int KC = (cin + 15) / 16, KS = 16 * KC;
  std::vector<float> im;
  if (w1_split3) push_frag_split3(im, &blob[f1.w], cin, cin, KC, KC);
  else push_frag(im, &blob[f1.w], cin, cin, KC, KC);
  push_frag(im, &blob[f2.w], cin, cin, KC, KC);
  push_frag(im, &blob[fpp.w], cin, cin, KC, KC);
  push_rows(im, &blob[fd.w], 9, cin, KS);
  push_rows(im, &blob[fpd.w], 9, cin, KS);
  for (const Folded* f : {&f1, &fd, &f2, &fpd, &fpp}) { push_vec(im, &blob[f->scale], cin, KS); push_vec(im, &blob[f->shift], cin, KS); }
  return put(im);
}
// tower kernels: pw [80][84] | output conv [mh16][84] | dw taps [25][80] | scd shd scp shp bias [5][96]
size_t WeightPacker::image_tower(const Folded& fd, const Folded& fp, const Folded* fh, int mh) {
  std::vector<float> im;
  push_frag(im, &blob[fp.w], 72, 72, 5, 5);
  const int mh_tiles = fh ? ((mh + 15) / 16 <= 1 ? 1 : 6) : 0;  // kernels are instantiated for 1 or 6 output tiles
  if (fh) push_frag(im, &blob[fh->w], mh, 72, mh_tiles, 5);
  push_rows(im, &blob[fd.w], 25, 72, 80);
  push_vec(im, &blob[fd.scale], 72, 96); push_vec(im, &blob[fd.shift], 72, 96);
  push_vec(im, &blob[fp.scale], 72, 96); push_vec(im, &blob[fp.shift], 72, 96);
  push_vec(im, fh ? &blob[fh->shift] : nullptr, mh, 96);
  return put(im);
}
// towerh_kernel (yfv2_towerh.hip): WP [5][5][64][4 dwords of fp16 pairs: term 1, term 1, term 2, term 2] | CS [4][96] |
// WH [mh tiles][5][64][4] | TAPS [5][4][27][4] + 16
size_t WeightPacker::image_towerh(const Folded& fd, const Folded& fp, const Folded* fh, int mh, int mh_tiles) {
  std::vector<float> im;
  const float* wpw = &blob[fp.w];
  const int sw = pow2_for(max_abs(wpw, 72 * 72));
  push_a16(im, [&](int r, int c) { return (r < 72 && c < 72) ? std::ldexp(wpw[(size_t)r * 72 + c], sw) : 0.f; }, 5);
  // A half that ends in an output conv: pointwise conv, its BatchNorm and the biased output conv are three linear maps in a row
  // (fpn.py:16-17,23-24 - no activation behind the block's last BN; detector.py:25-31), so the kernels apply their PRODUCT to the
  // depthwise result: M = Wh diag(scale) Wp (mh x 72), bias = Wh shift + b, both formed here in double and rounded once - closer
  // to the exact value than the reference's own two fp32 steps.  (The 72 x 72 filter above stays in the image: a launch has one
  // LDS layout for all its jobs, and the halves WITHOUT an output conv use it.)
  std::vector<float> mw, mb;
  int swh = 0;
  if (fh) {
    mw.assign((size_t)mh * 72, 0.f); mb.assign((size_t)mh, 0.f);
    for (int o = 0; o < mh; ++o) {
      double bacc = blob[fh->shift + o];
      for (int k = 0; k < 72; ++k) bacc += (double)blob[fh->w + (size_t)o * 72 + k] * (double)blob[fp.shift + k];
      mb[o] = (float)bacc;
      for (int c = 0; c < 72; ++c) {
        double acc = 0.0;
        for (int k = 0; k < 72; ++k) acc += (double)blob[fh->w + (size_t)o * 72 + k] * (double)blob[fp.scale + k] * (double)wpw[(size_t)k * 72 + c];
        mw[(size_t)o * 72 + c] = (float)acc;
      }
    }
    swh = pow2_for(max_abs(mw.data(), mh * 72));
  }
  for (int c = 0; c < 96; ++c) im.push_back(c < 72 ? std::ldexp(blob[fp.scale + c], -(sw + 4)) : 0.f);
  push_vec(im, &blob[fp.shift], 72, 96);
  push_vec(im, fh ? mb.data() : nullptr, mh, 96);
  for (int c = 0; c < 96; ++c) im.push_back(c == 0 ? std::ldexp(1.0f, -(swh + 4)) : 0.f);
  push_a16(im, [&](int r, int c) { return (fh && r < mh && c < 72) ? std::ldexp(mw[(size_t)r * 72 + c], swh) : 0.f; }, mh_tiles);   // zero tiles where a job has no (or a narrower) output conv: one LDS layout per launch
  auto tap = [&](int t, int ch) {   // depthwise record of a channel: taps 0..24, then BN scale and shift x 2^4 (exact)
    return (ch >= 72 || t > 26) ? 0.f : t < 25 ? blob[fd.w + (size_t)t * 72 + ch] : 16.0f * (t == 25 ? blob[fd.scale + ch] : blob[fd.shift + ch]);
  };
  for (int s = 0; s < 5; ++s)
    for (int q = 0; q < 4; ++q)
      for (int t = 0; t < 27; ++t)
        for (int e = 0; e < 4; ++e) im.push_back(tap(t, 16 * s + 4 * q + e));
  for (int i = 0; i < 16; ++i) im.push_back(0.f);   // the scalar-cache warm-up reads whole 64-byte lines
  // towerp_kernel's table (round 6): the same numbers per channel PAIR, one 256-byte record per (chunk, pair) = what a wave's
  // depthwise unit pulls into 54 SGPRs: floats 2 t + e = tap t of channel 16 s + 2 pair + e, 50 + e = BN scale x 16, 52 + e = BN shift x 16
  for (int s = 0; s < 5; ++s)
    for (int pr = 0; pr < 8; ++pr)
      for (int i = 0; i < 64; ++i) im.push_back(tap(i >> 1, 16 * s + 2 * pr + (i & 1)));
  return put(im);
}
// s1px_kernel image: w1q | w2q | depthwise taps [54][64] (lane&3 = k holds scaled tap 4q+k, flat index c*9 + dy*3 + dx).
// order[n] = which branch-input channel sits at input position n = which branch-output channel goes to output position n
size_t WeightPacker::image_s1px(const Folded& f1, const Folded& fd, const Folded& f2, const int (&order)[24]) {
  std::vector<float> im;
  const float* w1 = &blob[f1.w]; const float* w2 = &blob[f2.w];
  const float* sc1 = &blob[f1.scale]; const float* sh1 = &blob[f1.shift];
  const float* sc2 = &blob[f2.scale]; const float* sh2 = &blob[f2.shift];
  push_pw24_bcast(im, [](int n) { return n; }, [&](int k) { return order[k]; }, [&](int r) { return sh1[r]; }, w1, sc1);
  push_pw24_bcast(im, [&](int n) { return order[n]; }, [](int k) { return k; },
                  [&](int r) { return bias_through_pw(w2 + (size_t)r * 24, 24, sc2[r], sh2[r], &blob[fd.shift]); }, w2, sc2);
  push_taps_quad(im, &blob[fd.w], &blob[fd.scale]);
  return put(im);
}
// s1h_kernel (yfv2_stage2h.hip): the same block with both pointwise convs as two-term fp16 operands in the A-operand order of
// v_mfma_f32_16x16x32_f16 (push_h3_filter; channel positions: s1h_npos).  Position n = pair n / 2, element n & 1 of the 12
// branch pairs; order[] as image_s1px.  W1 | W2 | taps [18][64] | shift1 [32] | bias2 [32] | 2^-(sw2+4), zeros up to 3272 |
// per-lane byte offsets of the lane's four pairs, read from [4][64] | written to [4][64]
size_t WeightPacker::image_s1h(const Folded& f1, const Folded& fd, const Folded& f2, const int (&order)[24], const int (&src_off)[12], const int (&dst_off)[12]) {
  const float* w1 = &blob[f1.w]; const float* w2 = &blob[f2.w];
  const float* sc1 = &blob[f1.scale]; const float* sh1 = &blob[f1.shift];
  const float* sc2 = &blob[f2.scale]; const float* sh2 = &blob[f2.shift];
  auto e1 = [&](int r, int n) { return w1[(size_t)r * 24 + order[n]] * sc1[r]; };                 // pw1: natural output channel r, input position n
  auto e2 = [&](int r, int n) { return w2[(size_t)order[r] * 24 + n] * sc2[order[r]]; };          // pw2: output position r, natural input channel n
  const int sw1 = pow2_for(max_abs(24, 24, e1)), sw2 = pow2_for(max_abs(24, 24, e2));
  std::vector<float> im;
  push_h3_filter(im, [&](int r, int n) { return std::ldexp(e1(r, n), sw1); });
  push_h3_filter(im, [&](int r, int n) { return std::ldexp(e2(r, n), sw2); });
  push_lane_taps(im, &blob[fd.w], &blob[fd.scale], 24, -sw1);   // they see relu(pw1) * 2^(sw1+4) and must hand pw2 its input times 2^4: BN scale * 2^-sw1
  for (int n = 0; n < 32; ++n) im.push_back(n < 24 ? std::ldexp(sh1[n], sw1 + 4) : 0.f);
  for (int n = 0; n < 32; ++n) {
    const int r = n < 24 ? order[n] : 0;
    im.push_back(n < 24 ? std::ldexp(bias_through_pw(w2 + (size_t)r * 24, 24, sc2[r], sh2[r], &blob[fd.shift]), sw2 + 4) : 0.f);
  }
  im.push_back(std::ldexp(1.0f, -(sw2 + 4)));
  while (im.size() < 3272) im.push_back(0.f);
  push_lane_pairs(im, [&](int kk) { return src_off[kk]; });
  push_lane_pairs(im, [&](int kk) { return dst_off[kk]; });
  return put(im);
}
// s2px_kernel role images.  pos[n] = branch-local output channel at output position n of the role's last pointwise conv
size_t WeightPacker::image_s2px_proj(const Folded& fpd, const Folded& fpp, const int (&pos)[24]) {
  std::vector<float> im;
  const float* w = &blob[fpp.w]; const float* sc = &blob[fpp.scale]; const float* sh = &blob[fpp.shift];
  push_pw24_bcast(im, [&](int n) { return pos[n]; }, [](int k) { return k; },
                  [&](int r) { return bias_through_pw(w + (size_t)r * 24, 24, sc[r], sh[r], &blob[fpd.shift]); }, w, sc);
  push_taps_quad(im, &blob[fpd.w], &blob[fpd.scale]);
  return put(im);
}
size_t WeightPacker::image_s2px_main(const Folded& f1, const Folded& fd, const Folded& f2, const int (&pos)[24]) {
  std::vector<float> im;
  const float* w2 = &blob[f2.w]; const float* sc2 = &blob[f2.scale]; const float* sh2 = &blob[f2.shift];
  const float* sh1 = &blob[f1.shift];
  push_pw24_bcast(im, [](int n) { return n; }, [](int k) { return k; }, [&](int r) { return sh1[r]; }, &blob[f1.w], &blob[f1.scale]);
  push_pw24_bcast(im, [&](int n) { return pos[n]; }, [](int k) { return k; },
                  [&](int r) { return bias_through_pw(w2 + (size_t)r * 24, 24, sc2[r], sh2[r], &blob[fd.shift]); }, w2, sc2);
  push_taps_quad(im, &blob[fd.w], &blob[fd.scale]);
  return put(im);
}
// s2h_kernel (yfv2_stage2h.hip): stage2.0 with both branches in one wave.  Input positions = natural channels (the stem's
// pair planes); output position r of a branch = its channel pos[r] (pos[][] of PlanBuilder::s2px_block: 0..15 = the branch's
// eight whole pairs, 16..23 = its halves of the eight pairs that mix a proj and a main channel).
// W1 | Wproj | W2 (push_h3_filter) | main taps | proj taps [18][64] | shift1 | bias proj | bias 2 [32] | 2^-(swp+4), 2^-(sw2+4),
// zeros up to 5480 | per-lane byte offsets: loads [4][64] | stores [8][64]
size_t WeightPacker::image_s2h(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, const int (&pos)[2][24],
                               const int (&st2_off)[2][8], const int (&st1_off)[2][8], int IH, int IW) {
  const float* w1 = &blob[f1.w]; const float* w2 = &blob[f2.w]; const float* wq = &blob[fpp.w];
  const float* sc1 = &blob[f1.scale]; const float* sc2 = &blob[f2.scale]; const float* scq = &blob[fpp.scale];
  auto e1 = [&](int r, int n) { return w1[(size_t)r * 24 + n] * sc1[r]; };
  auto ep = [&](int r, int n) { return wq[(size_t)pos[0][r] * 24 + n] * scq[pos[0][r]]; };
  auto e2 = [&](int r, int n) { return w2[(size_t)pos[1][r] * 24 + n] * sc2[pos[1][r]]; };
  const int sw1 = pow2_for(max_abs(24, 24, e1)), swp = pow2_for(max_abs(24, 24, ep)), sw2 = pow2_for(max_abs(24, 24, e2));
  std::vector<float> im;
  push_h3_filter(im, [&](int r, int n) { return std::ldexp(e1(r, n), sw1); });
  push_h3_filter(im, [&](int r, int n) { return std::ldexp(ep(r, n), swp); });
  push_h3_filter(im, [&](int r, int n) { return std::ldexp(e2(r, n), sw2); });
  push_lane_taps(im, &blob[fd.w], &blob[fd.scale], 24, -sw1);     // main: sees relu(pw1) * 2^(sw1+4), hands pw2 its input * 2^4
  push_lane_taps(im, &blob[fpd.w], &blob[fpd.scale], 24, 0);      // proj: sees the raw input * 2^4
  for (int n = 0; n < 32; ++n) im.push_back(n < 24 ? std::ldexp(blob[f1.shift + n], sw1 + 4) : 0.f);
  auto bias = [&](const float* w, const Folded& fp_, const Folded& fdw, int c) {
    return bias_through_pw(w + (size_t)c * 24, 24, blob[fp_.scale + c], blob[fp_.shift + c], &blob[fdw.shift]);
  };
  for (int n = 0; n < 32; ++n) im.push_back(n < 24 ? std::ldexp(bias(wq, fpp, fpd, pos[0][n]), swp + 4) : 0.f);
  for (int n = 0; n < 32; ++n) im.push_back(n < 24 ? std::ldexp(bias(w2, f2, fd, pos[1][n]), sw2 + 4) : 0.f);
  im.push_back(std::ldexp(1.0f, -(swp + 4)));
  im.push_back(std::ldexp(1.0f, -(sw2 + 4)));
  while (im.size() < 5480) im.push_back(0.f);
  push_lane_pairs(im, [&](int kk) { return kk * IH * IW * 8; });   // loads: the lane's four input pair planes
  for (int k = 0; k < 8; ++k)                      // stores: proj whole pairs (2), main whole pairs (2), mixed pairs (4)
    for (int l = 0; l < 64; ++l) {
      const int g = l >> 4;
      int v = LANE_NONE;
      if (k < 2) v = st2_off[0][2 * g + k];
      else if (k < 4) v = st2_off[1][2 * g + (k - 2)];
      else if (g < 2) v = st1_off[0][4 * g + (k - 4)];   // the pair's base: proj sits in element 0, main in element 1
      push_bits(im, v);
    }
  return put(im);
}
// s3h_kernel / s4h_kernel (yfv2_stage2h.hip): a stride-2 block of C = 48 / 96 input channels (stage3.0 48 -> 96, stage4.0
// 96 -> 192) in the same form.  Lane (l, g) owns positions k_col(g, q) = 16 (q / 4) + 4g + q % 4, q = 0 .. C / 4 - 1; as K
// slots: chunk q / 8, slot q % 8 (48 channels: the second chunk's slots 4..7 are zero).  Input positions = what the Folded
// objects passed in have as input columns / depthwise channels, outputs natural.
// W1 | Wproj | W2, each x 2^sw as two fp16 terms [C / 16][chunks][2][64][4] | main taps | proj taps (push_lane_taps) |
// shift1 * 2^(sw1+4) | bias proj * 2^(swp+4) | bias 2 * 2^(sw2+4) [C] | 2^-(swp+4), 2^-(sw2+4), 0, 0
void WeightPacker::build_s2_stream(std::vector<float>& im, const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, int C) {
  const Folded* fs[3] = {&f1, &fpp, &f2};
  int sw[3];
  for (int f = 0; f < 3; ++f) {
    const float* w = &blob[fs[f]->w]; const float* sc = &blob[fs[f]->scale];
    auto el = [&](int r, int n) { return w[(size_t)r * C + n] * sc[r]; };
    sw[f] = pow2_for(max_abs(C, C, el));
    push_f16_matrix(im, C, C, C / 16, (C + 31) / 32, [&](int r, int n) { return std::ldexp(el(r, n), sw[f]); });
  }
  push_lane_taps(im, &blob[fd.w], &blob[fd.scale], C, -sw[0]);      // main: sees relu(pw1) * 2^(sw1+4), hands pw2 its input * 2^4
  push_lane_taps(im, &blob[fpd.w], &blob[fpd.scale], C, 0);         // proj: sees the raw input * 2^4
  for (int n = 0; n < C; ++n) im.push_back(std::ldexp(blob[f1.shift + n], sw[0] + 4));
  auto bias = [&](const Folded& fp_, const Folded& fdw, int c) {
    return bias_through_pw(&blob[fp_.w + (size_t)c * C], C, blob[fp_.scale + c], blob[fp_.shift + c], &blob[fdw.shift]);
  };
  for (int n = 0; n < C; ++n) im.push_back(std::ldexp(bias(fpp, fpd, n), sw[1] + 4));
  for (int n = 0; n < C; ++n) im.push_back(std::ldexp(bias(f2, fd, n), sw[2] + 4));
  im.push_back(std::ldexp(1.0f, -(sw[1] + 4)));
  im.push_back(std::ldexp(1.0f, -(sw[2] + 4)));
  im.push_back(0.f); im.push_back(0.f);
}
// s3h_kernel: input positions = stage 2's pair-plane slots; behind the image [6][64] per-lane byte offsets of input pair
// 8t + 2g + h, k = 2t + h
size_t WeightPacker::image_s3h(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, unsigned pp_mask,
                               long long pp_bufstride, int IH, int IW) {
  std::vector<float> im;
  build_s2_stream(im, f1, fd, f2, fpd, fpp, 48);
  for (int k = 0; k < 6; ++k)
    for (int l = 0; l < 64; ++l) {
      const int pair = 8 * (k >> 1) + 2 * (l >> 4) + (k & 1);
      const long long off = (((pp_mask >> pair) & 1u) ? pp_bufstride * 4 : 0) + (long long)pair * IH * IW * 8;
      push_bits(im, (int)off);
    }
  return put(im);
}
// s4h_kernel: input positions = physical NHWC channel positions of stage 3's output
size_t WeightPacker::image_s4h(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp) {
  std::vector<float> im;
  build_s2_stream(im, f1, fd, f2, fpd, fpp, 96);
  return put(im);
}
