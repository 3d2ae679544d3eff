// yfv2_device.h - device-only helpers shared by the kernel translation units: vector types, lane moves (DPP), the fp16 two-term
// split, the bf16x6 split, the range guard, the post-process sigmoid / softmax, the wave fold and the cycle stamps.  ONE definition
// of each; included by the kernel units only (the host units - pack, plan, api* - include yfv2_internal.h and never parse this).
// What does NOT belong here: operand packing that only one kernel's MFMA layout explains (mfma_cross, pw_h3, f_conv_col, the chain's
// BOps) stays next to that kernel.
#pragma once
#include "yfv2_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x3u __attribute__((ext_vector_type(3), aligned(4)));   // three floats at any dword address (global_load/store_dwordx3)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 yfv2_h2 __attribute__((ext_vector_type(2)));
typedef _Float16 yfv2_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 yfv2_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 yfv2_bf16x8 __attribute__((ext_vector_type(8)));

// n / d for 0 <= n < 2^16 and 8 <= d <= 1024 through the float pipe (cvt, fma, cvt instead of the ~25-instruction
// integer division): (n + 0.5) / d is at least 0.5/d away from an integer, far more than the fp32 error of the product.
__device__ __forceinline__ int yfv2_fdiv(int n, float inv_d) { return (int)(((float)n + 0.5f) * inv_d); }

// ---- bit casts and lane moves
// NB: pass the value through a by-value parameter (f2i, row_shr1, ...): __builtin_bit_cast applied directly to a vector
// ELEMENT lvalue (bit_cast(int, q[3])) reads element 0 with this compiler (seen in tools/ubench/dpp.hip).
__device__ __forceinline__ int f2i(float v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ float i2f(int v) { return __builtin_bit_cast(float, v); }
// lane l <- lane l-1 inside its 16-lane row, 0 at l = 0 (DPP row_shr:1, zero fill: a conv's left padding)
__device__ __forceinline__ float row_shr1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
}
__device__ __forceinline__ unsigned row_shr1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); }
__device__ __forceinline__ float row_shl1(float v) {   // lane l <- lane l+1 inside its 16-lane row, 0 at l = 15
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x101, 0xf, 0xf, true));
}
// tap k (0..3) of the lane's quad: the depthwise taps live four to a register in the lanes of every quad
// (all quads identical), DPP quad_perm:[k,k,k,k] hands tap k to all lanes without touching SGPRs or LDS
template <int K>
__device__ __forceinline__ float quad_mul(float tap4, float v) {   // tap4[quad lane K] * v
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, tap4), K * 0x55, 0xf, 0xf, false)) * v;
}
// acc += tap4[quad lane K] * v as ONE v_fmac_f32_dpp (hipcc folds the DPP into v_mul but not into v_fmac: it
// emits v_mov 0 + v_mov_dpp + v_fmac).  Inline asm hides two gfx9 hazards from the compiler's hazard recognizer,
// both met in practice (wrong depthwise sums in one wave role only):
//   * the tap register may just have been written by a VALU op the compiler inserted (a v_accvgpr_read of a
//     spilled tap): "VALU writes VGPR -> DPP reads it" needs 2 wait states -> every asm block starts with s_nop 1;
//   * the asm WRITES acc with a VALU op, and a compiler-generated DPP (row_shr1/row_shl1 of a column sum) may
//     read it next -> dpp_src_ready() below.
// Groups of FMAs share one block (one s_nop).  KA.. are the quad lanes of the taps (immediates).
#define YFV2_QP(n) "quad_perm:[%" #n ",%" #n ",%" #n ",%" #n "] row_mask:0xf bank_mask:0xf\n\t"
template <int KA>
__device__ __forceinline__ void quad_fmac1(float& s, float ta, float v) {
  asm("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 " YFV2_QP(3) : "+v"(s) : "v"(ta), "v"(v), "n"(KA));
}
// s = ta*v0; q = tb*v1; s += tc*v1   (the FIRST vertical tap row of a stride-2 window: two v_mul_f32_dpp and one v_fmac_f32_dpp, the
// same three operations as quad_mul, quad_mul, quad_fmac1.  As compiler code the second product's tap broadcast can end up in another
// basic block than its multiply, where it stays a v_mov 0 + v_mov_dpp + v_mul: three instructions for one.)
template <int KA, int KB, int KC>
__device__ __forceinline__ void quad_mul2_fmac1(float& s, float& q, float ta, float tb, float tc, float v0, float v1) {
  asm("s_nop 1\n\tv_mul_f32_dpp %0, %2, %5 " YFV2_QP(7) "v_mul_f32_dpp %1, %3, %6 " YFV2_QP(8) "v_fmac_f32_dpp %0, %4, %6 " YFV2_QP(9)
      : "=&v"(s), "=&v"(q) : "v"(ta), "v"(tb), "v"(tc), "v"(v0), "v"(v1), "n"(KA), "n"(KB), "n"(KC));
}
// s += ta*v0; q += tb*v1; s += tc*v1   (one vertical tap row of a stride-2 window: dx = 1, 0, 2)
template <int KA, int KB, int KC>
__device__ __forceinline__ void quad_fmac3(float& s, float& q, float ta, float tb, float tc, float v0, float v1) {
  asm("s_nop 1\n\tv_fmac_f32_dpp %0, %2, %5 " YFV2_QP(7) "v_fmac_f32_dpp %1, %3, %6 " YFV2_QP(8) "v_fmac_f32_dpp %0, %4, %6 " YFV2_QP(9)
      : "+v"(s), "+v"(q) : "v"(ta), "v"(tb), "v"(tc), "v"(v0), "v"(v1), "n"(KA), "n"(KB), "n"(KC));
}
// a0 += t3*u + t6*w; a1 += t4*u + t7*w; a2 += t5*u + t8*w   (rows dy = 1, 2 of a stride-1 window, all three dx)
template <int K3, int K4, int K5, int K6, int K7, int K8>
__device__ __forceinline__ void quad_fmac6(float& a0, float& a1, float& a2, float t3, float t4, float t5, float t6, float t7, float t8,
                                           float u, float w) {
  asm("s_nop 1\n\tv_fmac_f32_dpp %0, %3, %9 " YFV2_QP(11) "v_fmac_f32_dpp %1, %4, %9 " YFV2_QP(12) "v_fmac_f32_dpp %2, %5, %9 " YFV2_QP(13)
      "v_fmac_f32_dpp %0, %6, %10 " YFV2_QP(14) "v_fmac_f32_dpp %1, %7, %10 " YFV2_QP(15) "v_fmac_f32_dpp %2, %8, %10 " YFV2_QP(16)
      : "+v"(a0), "+v"(a1), "+v"(a2)
      : "v"(t3), "v"(t4), "v"(t5), "v"(t6), "v"(t7), "v"(t8), "v"(u), "v"(w), "n"(K3), "n"(K4), "n"(K5), "n"(K6), "n"(K7), "n"(K8));
}
#undef YFV2_QP
// 2 wait states between an inline-asm VALU write of v and a DPP read of v (gfx9 "VALU writes VGPR -> DPP reads it")
__device__ __forceinline__ void dpp_src_ready(float& v) { asm volatile("s_nop 1" : "+v"(v)); }

// halves of two packed registers (v_perm_b32)
__device__ __forceinline__ unsigned pack_hi_hi(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }   // {a.hi, b.hi}
__device__ __forceinline__ unsigned pack_hi_lo(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x05040302u); }   // {a.hi, b.lo}
// bytes sel.b0 and sel.b2 of the eight bytes {hi, lo} -> two exact fp16 integers: u8 -> fp16 without a conversion
// instruction, 0x6400 | n is the fp16 number 1024 + n, one packed subtract gives n
__device__ __forceinline__ unsigned u8pair(unsigned hi, unsigned lo, unsigned sel) {
  const unsigned v = __builtin_amdgcn_perm(hi, lo, sel) | 0x64006400u;
  const yfv2_h2 h = __builtin_bit_cast(yfv2_h2, v) - (yfv2_h2){(_Float16)1024.0f, (_Float16)1024.0f};
  return __builtin_bit_cast(unsigned, h);
}

// ---- the fp16 two-term split of the fp16x3 arithmetic: THE definition, every kernel of the default plan uses it.
// Contract: h1 = RN16(v) (v_cvt_pk_f16_f32, round to nearest), r = v - fl32(h1) (exact in fp32), h2 = RN16(r).  h1 + h2 reproduces
// v to 2^-24 |v| while |v| < 65504 and h2 is a normal fp16, and to 2^-25 absolutely below that; beyond the range h1 = +-Inf and the
// products are NaN, which Yfv2Watch reports.  The caller applies the exact power-of-two pre-scale that moves fp16's absolute floor out
// of the way (x 2^4 activations, x 2^8 pixels, none where the producer's BN constants already carry it) and undoes it after the sum.
// The cross-plan bit-identity tests hold because every site is this one expression.
// pair form: {first terms of (v0, v1), second terms}; quad form: {first terms of (v0, v1), (v2, v3), second terms of (v0, v1), (v2, v3)}
__device__ __forceinline__ u32x2 split_f16x2(f32x2 v) {
  const yfv2_h2 t1 = __builtin_convertvector(v, yfv2_h2);                       // v_cvt_pk_f16_f32 (RN)
  const f32x2 r = v - __builtin_convertvector(t1, f32x2);                       // exact
  const yfv2_h2 t2 = __builtin_convertvector(r, yfv2_h2);
  return (u32x2){__builtin_bit_cast(unsigned, t1), __builtin_bit_cast(unsigned, t2)};
}
__device__ __forceinline__ u32x4 split_f16x2(f32x4 v) {
  const yfv2_h4 t1 = __builtin_convertvector(v, yfv2_h4);                       // v_cvt_pk_f16_f32 (RN)
  const f32x4 r = v - __builtin_convertvector(t1, f32x4);                       // exact
  const yfv2_h4 t2 = __builtin_convertvector(r, yfv2_h4);
  const u32x2 a = __builtin_bit_cast(u32x2, t1), b = __builtin_bit_cast(u32x2, t2);
  return (u32x4){a[0], a[1], b[0], b[1]};
}

// ---- the stem's row records (yfv2_stem16.hip's kernels and the stem part of front2_kernel, yfv2_stage2h.hip)
// one input row of the lane, both fp16 terms [k]: pairs (v0, v1), (v2, v3); m: HIGH half = the column left of v0 (filled by the kernel:
// the left lane's p23, or the lane's own other record)
struct Row16 { unsigned p01[2], p23[2], m[2]; };
struct Row8 { unsigned p01, p23, m; };   // uint8 input: a pixel is exactly ONE fp16 term
__device__ __forceinline__ void split_cols(const f32x4 v, Row16& o) {   // the image is split after an exact x 2^8 (undone with the filter's 2^-sw)
  const u32x2 a = split_f16x2((f32x2){v[0], v[1]} * 256.0f), b = split_f16x2((f32x2){v[2], v[3]} * 256.0f);
  o.p01[0] = a[0]; o.p01[1] = a[1];
  o.p23[0] = b[0]; o.p23[1] = b[1];
}
__device__ __forceinline__ void split_cols_u8(const u32x3 d, unsigned sel_a, unsigned sel_b, Row8& o) {
  o.p01 = u8pair(d[1], d[0], sel_a);
  o.p23 = u8pair(d[2], d[1], sel_b);
}

// ---- fp32 pointwise convs on the bf16 matrix cores ("bf16x6")
// gfx950's fp32 MFMA runs at the fp32 VECTOR rate (16x16x4: 32 cycles per 1024 MACs per SIMD); its bf16 MFMA is 16x
// faster (16x16x32: ~17 cycles per 8192 MACs).  An fp32 value is EXACTLY the sum of three bf16 terms (truncation: 8 + 8 + 8
// significant bits), so w * x = sum of nine bf16 x bf16 products, each exact in fp32; the six largest (everything above
// 2^-23 of |w x|, i.e. below one fp32 rounding of the product) are accumulated in fp32 by three MFMAs whose eight k-slots
// per lane group are the lane's 4 channels x 2 terms:
//     A {w.hi, w.hi} x B {x.hi, x.mid}      A {w.mid, w.mid} x B {x.hi, x.mid}      A {w.hi, w.lo} x B {x.lo, x.hi}
// Same fragment maps as v_mfma_f32_16x16x4_f32 (A lane l: row l&15; B lane l: pixel l&15; lane group l>>4 owns 4 channels of
// the 16-channel chunk; D lane l reg r: row 4(l>>4)+r, column l&15), so it drops into the existing loops: split the A
// fragment once per (tile of output channels, chunk), the B fragment once per (pixel tile, chunk), then mfma6().
// Measured (tools/ubench/bf16x6.hip, K = 192, 5 x 2 tiles): max error vs float64 7.1e-6 against 8.6e-6 for the fp32 MFMA on
// the same data; 30 MFMAs in ~520 cycles against 40 in 1280; the whole network's logits: 1.39e-5 vs 1.41e-5 from float64.
struct Bf3A { u32x4 hh, mm, hl; };   // {hi,hi}, {mid,mid}, {hi,lo}
struct Bf3B { u32x4 hm, lh; };       // {hi,mid}, {lo,hi}
__device__ __forceinline__ unsigned yfv2_pack_hi16(float a, float b) {   // high halves of a (low 16 bits) and b (high 16 bits): two truncated bf16
  return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, b), __builtin_bit_cast(unsigned, a), 0x07060302u);
}
__device__ __forceinline__ float yfv2_trunc_bf16(float a) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, a) & 0xffff0000u); }
__device__ __forceinline__ void yfv2_split3(f32x4 v, unsigned (&h)[2], unsigned (&m)[2], unsigned (&l)[2]) {
  float r1[4], r2[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { r1[c] = v[c] - yfv2_trunc_bf16(v[c]); r2[c] = r1[c] - yfv2_trunc_bf16(r1[c]); }   // exact subtractions
  h[0] = yfv2_pack_hi16(v[0], v[1]); h[1] = yfv2_pack_hi16(v[2], v[3]);
  m[0] = yfv2_pack_hi16(r1[0], r1[1]); m[1] = yfv2_pack_hi16(r1[2], r1[3]);
  l[0] = yfv2_pack_hi16(r2[0], r2[1]); l[1] = yfv2_pack_hi16(r2[2], r2[3]);
}
__device__ __forceinline__ Bf3A yfv2_split_a(f32x4 w) {
  unsigned h[2], m[2], l[2];
  yfv2_split3(w, h, m, l);
  return {(u32x4){h[0], h[1], h[0], h[1]}, (u32x4){m[0], m[1], m[0], m[1]}, (u32x4){h[0], h[1], l[0], l[1]}};
}
__device__ __forceinline__ Bf3B yfv2_split_b(f32x4 x) {
  unsigned h[2], m[2], l[2];
  yfv2_split3(x, h, m, l);
  return {(u32x4){h[0], h[1], m[0], m[1]}, (u32x4){l[0], l[1], h[0], h[1]}};
}
// one of the three MFMAs (k = 0: the small terms, 1: w.mid, 2: w.hi): call sites run k outermost over their independent
// accumulators so that no MFMA waits for the one before it
template <int k>
__device__ __forceinline__ f32x4 yfv2_mfma6_step(const Bf3A& a, const Bf3B& b, f32x4 acc) {
  if constexpr (k == 0) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(yfv2_bf16x8, a.hl), __builtin_bit_cast(yfv2_bf16x8, b.lh), acc, 0, 0, 0);
  else if constexpr (k == 1) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(yfv2_bf16x8, a.mm), __builtin_bit_cast(yfv2_bf16x8, b.hm), acc, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(yfv2_bf16x8, a.hh), __builtin_bit_cast(yfv2_bf16x8, b.hm), acc, 0, 0, 0);
}
// acc[mt][nt] += A[mt] x B[nt] for all tiles of a 16-channel chunk
template <int MT_, int NT_>
__device__ __forceinline__ void yfv2_mfma6_tiles(const Bf3A (&a)[MT_], const Bf3B (&b)[NT_], f32x4 (&acc)[MT_][NT_]) {
#pragma unroll
  for (int mt = 0; mt < MT_; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT_; ++nt) acc[mt][nt] = yfv2_mfma6_step<0>(a[mt], b[nt], acc[mt][nt]);
#pragma unroll
  for (int mt = 0; mt < MT_; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT_; ++nt) acc[mt][nt] = yfv2_mfma6_step<1>(a[mt], b[nt], acc[mt][nt]);
#pragma unroll
  for (int mt = 0; mt < MT_; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT_; ++nt) acc[mt][nt] = yfv2_mfma6_step<2>(a[mt], b[nt], acc[mt][nt]);
}

// ---- range guard of the fp16x3 arithmetic (include/yfv2.h yfv2_nonfinite)
// An operand beyond fp16's range (|activation| * 2^4 or |pixel| * 2^8 >= 65520) splits into (+Inf, -Inf); the three
// products of ANY filter entry with it are +-Inf or NaN and sum to NaN, for every output channel of that pixel - and the ReLU
// behind almost every pointwise conv (v_max_f32 / v_med3_f32 return the non-NaN operand) would turn that NaN into a clean,
// silent 0.  So every kernel of the fp16x3 plan looks at ONE accumulator element per lane of every pointwise product before
// its ReLU: a shift and an unsigned compare into a scalar register pair OR-ed into a sticky wave-uniform mask (no branch),
// and reports once at its end.  Non-finite INPUT values are caught by the same test.
struct Yfv2Watch {
  unsigned long long m = 0;
  // an integer test of the exponent field (all ones: NaN or Inf), two VALU instructions: the kernel files are compiled with
  // -fno-honor-nans (bare v_max for the ReLUs), under which `v != v` and the class intrinsics fold to false
  __device__ __forceinline__ void see(float v) {
    const unsigned b = __builtin_bit_cast(unsigned, v);
    m |= __builtin_amdgcn_ballot_w64((b << 1) >= 0xff000000u);
  }
  __device__ __forceinline__ void report(int* flag) const {
    // the rare path.  A plain store of the constant 1 (every writer stores the same value): the word lives in host-mapped,
    // coherent memory (yfv2_create), where a store needs no PCIe atomic - the host can then LOOK at it without waiting for
    // any stream (yfv2_nonfinite_peek)
    if (m != 0 && flag != nullptr) *reinterpret_cast<volatile int*>(flag) = 1;
  }
};

// ---- the device sigmoid and class softmax of the post-process (decode_kernel, yfv2_post.hip; export_maps_kernel, yfv2_deploy.hip).
// ONE definition: the two kernels must agree bit for bit.  Units that use them are built with -ffp-contract=off.
// fp32 sigmoid as ATen's CPU kernel evaluates it: 1 / (1 + exp(-x)), true division
__device__ __forceinline__ float sigmoid_f32(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }
// fp32 softmax over the `nc` class logits cls[c * hw + cc] of one grid cell, shared by 4 CONSECUTIVE, CONVERGED lanes: lane
// `part` (0..3) owns classes [part * per, min(nc, (part + 1) * per)), per = ceil(nc / 4), and gets their probabilities
// exp(x - max) / sum in ev[0 .. per) (slots beyond its slice: 0).  The sum is added slice by slice in class order, then
// (s0 + s1) + (s2 + s3) by two xor exchanges: the summation tree is part of the result.  The lane's logits are fetched with
// one batch of independent loads (fixed trip count, masked) instead of a load per loop turn.
template <int MAXPER>
__device__ __forceinline__ void yfv2_softmax_quad(const float* cls, int nc, int hw, int cc, int part, float (&ev)[MAXPER]) {
  const int per = (nc + 3) >> 2;
  const int c_lo = part * per, c_hi = min(nc, c_lo + per);
  float lv[MAXPER];
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) {
    const int c = c_lo + i;
    lv[i] = cls[(unsigned)((c < c_hi ? c : (c_lo < nc ? c_lo : 0)) * hw + cc)];   // masked slots re-read a valid class (fewer than 4 classes: quarters 1-3 are empty)
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAXPER; ++i)
    if (c_lo + i < c_hi) m = fmaxf(m, lv[i]);
  m = fmaxf(m, __shfl_xor(m, 1));
  m = fmaxf(m, __shfl_xor(m, 2));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) {
    ev[i] = 0.f;
    if (c_lo + i < c_hi) {
      ev[i] = expf(__fsub_rn(lv[i], m));
      sum = __fadd_rn(sum, ev[i]);
    }
  }
  sum = __fadd_rn(sum, __shfl_xor(sum, 1));
  sum = __fadd_rn(sum, __shfl_xor(sum, 2));
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) ev[i] = __fdiv_rn(ev[i], sum);  // class probabilities of this lane's slice
}

// ---- the fold of a wave's 64 lane values (k-means partial sums, AP chunk sums: the summation tree is part of their results).  Lane l
// adds the value of lane l ^ off; addition commutes bit for bit, so the two partners hold the same number after every step and lane 0
// ends with the tree over (l, l + off)
template <typename T>
__device__ __forceinline__ T wave_fold(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- cycle stamps of workgroup 0 into the launch's `a.trace` (debug; null: none).  YFV2_STAMP: thread 0 at phase boundaries, trace[i];
// YFV2_WSTAMP: lane 0 of every wave (YFV2_TRACE=1, tools/trace_waves.py), trace[64 + 32 * wave + i]
#define YFV2_STAMP(i) do { if (a.trace && blockIdx.x == 0 && threadIdx.x == 0) a.trace[i] = (long long)__builtin_readcyclecounter(); } while (0)
#define YFV2_WSTAMP(i) do { if (a.trace && blockIdx.x == 0 && (threadIdx.x & 63) == 0) a.trace[64 + 32 * (threadIdx.x >> 6) + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
