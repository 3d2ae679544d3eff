// yfv2_stem16.hip - the stem (conv3x3 s2 3->24 + BN + ReLU + maxpool3x3 s2, model/backbone/shufflenetv2.py:74-80,
// 102-104; behaviour only) as an implicit GEMM on the f16 matrix cores, fp32 accuracy kept by splitting every operand
// EXACTLY-to-2^-24 into two fp16 terms ("fp16x3"): round 3's replacement of yfv2_stem.hip's 4x4x1 fp32-MFMA kernel for
// fp32 input, and (stem_h3u_kernel, at the end of this file) for the uint8 entry points; the 4x4x1 kernel stays as the YFV2_BF6=0 plan.
//
// Why: gfx950's fp32 MFMA issues at the fp32 VECTOR rate and shares that datapath with the VALU (tools/ubench/shadow.hip),
// so the old kernel's time was MFMA + VALU summed (PMC: MFMA busy 55 %, issue-wait 40 %, 144 us = 0.49 of the HBM roofline
// on its 571 MB).  v_mfma_f32_16x16x32_f16 is 16x faster per MAC and runs beside the VALU.
//
// Arithmetic.  For a = fl32, h1 = RN16(a), h2 = RN16(a - fl32(h1)) (the subtraction is exact): |a - h1 - h2| <= 2^-24 |a|
// as long as |a| < 65504 and h2 is a normal fp16, and <= 2^-25 absolutely below that.  w x = w1 x1 + w1 x2 + w2 x1 + O(2^-22)
// w2 x2: three f16 x f16 products, each EXACT in fp32 (11 + 11 significant bits), accumulated in fp32 by the matrix core -
// the error per product is below the one rounding v_mfma_f32_4x4x1_f32 makes, measured in tests/test_stem16_host_model.py
// (numpy model of this arithmetic vs float64 and vs the fp32 conv).  The filter (BN scale folded) is split on the HOST and
// pre-scaled by a power of two 2^sw that puts its largest entry near 2^14 (exact; undone with the same power of two after
// pooling), so that the second terms of small weights stay normal numbers; the image is split in the kernel after an exact
// scaling by 2^8 (fp16's absolute floor 2^-25 then sits at 2^-33 of a pixel: below one fp32 ulp of every pixel value >=
// 1/255; unscaled, a dark image's second terms would be subnormal and the result 100x less accurate than the fp32 conv -
// tests/test_stem16_host_model.py).  Valid for |x| < 255.9: the reference feeds [0, 1] (test.py:38), raw 0..255 pixels fit too;
// larger magnitudes overflow fp16 (stated in include/yfv2.h; the uint8 entry points and YFV2_BF6=0 have no such bound).
// A carried row above the image / a band's first row: see the kernels.
//
// GEMM shape.  D[channel][pixel] += W[channel][k] X[k][pixel], 16 x 16 x 32 per instruction: 24 channels = two channel tiles
// (the second half empty), K = 27 taps in 32 slots, N = 16 pixels.  A wave = ONE strip of 16 lanes' worth of pooled columns
// (15 new + a halo lane, as in yfv2_stem.hip) walking down a band of pooled rows; lane = (p = lane & 15: pooled column
// px = 15 strip + p, g = lane >> 4: K group).  Per conv row the wave multiplies TWO pixel tiles - tile E: the even conv
// columns 2px, tile O: the odd ones 2px + 1 - so that the horizontal max-pool needs ONE neighbour access
// (max(O[p-1], E[p], O[p])) and every lane ends up with pooled values to store.
//
// K slots.  Lane group g < 3 carries input channel g: one ALIGNED 16-byte load per input row gives columns 4px .. 4px+3 =
// v0..v3, the column 4px-1 = vm1 is the left neighbour's v3 (DPP row_shr:1, zero fill = the image's left padding).  With
// X0, X1, X2 = input rows 2y-1, 2y, 2y+1 of conv row y the eight slots of a lane are
//     tile E:  X0.v0 X0.v1 | X1.v0 X1.v1 | X0.vm1 X1.vm1 | X2.vm1 X2.v0        taps (ky,kx): (0,1)(0,2) (1,1)(1,2) (0,0)(1,0) (2,0)(2,1)
//     tile O:  X0.v2 X0.v3 | X1.v2 X1.v3 | X0.v1  X1.v1  | X2.v1  X2.v2        (same taps, columns shifted by two)
// - the first two register pairs are the packed conversion of a loaded pair as it stands.  That is 8 of a channel's 9
// taps; the ninth, (2,2), of all three channels lives in lane group 3, which runs the SAME instructions on other data:
// its "X1" is (ch0, ch1) of columns 4px+1 | 4px+3 of row 2y+1 and its "X2" is ch2 of the same columns, which puts tap (2,2)
// of the three channels into slots 2, 3 and 7 of both tiles; the filter image is zero in its other slots.  Lane group 3
// loads nothing: those values sit in the registers of lanes (p, 0..2) and come over with six ds_bpermute_b32 per conv row.
// No LDS storage, no barriers; carried between conv rows: the split row 2y+1 (= the next row's 2y-1) and the pooled maxima.
//
// Measured (round 3, same-box A/Bs at B = 256): the 4x4x1 kernel 145-151 us; this arithmetic with one conv
// row of load lookahead 148 (the compute had moved off the critical path, the kernel was now bound by bytes in flight);
// two conv rows of lookahead (this form, 140 VGPRs, 3 waves per SIMD) 134; a MEMORY-ONLY build of the same loads and
// stores (no conversion, no MFMA) 120-128 - reads alone 92, writes alone 38-45: the launch is bound by its HBM access
// pattern (strips of 240 bytes per row and plane), not by arithmetic; every input value loaded once (lane group 3 by
// ds_bpermute instead of three extra L2-hit loads, row 2y-1 carried instead of re-read) 118-124.  4 waves per SIMD by
// register cap spills (258 us); by buffer stores with 32-bit offsets instead of 64-bit pointers (124 VGPRs, no spills): no
// change (131-133 against 128-132 us, same box) - bytes in flight are not what limits it; 4, 2 or 11 bands per image
// instead of 8: 126-131.
#include "yfv2_device.h"

namespace {
// Row16 / Row8, split_cols and the two-term split itself are yfv2_device.h's (front2_kernel, yfv2_stage2h.hip, shares them); here a
// row's left column comes from the left lane
__device__ __forceinline__ void split_row(const f32x4 v, Row16& o) {
  split_cols(v, o);
  o.m[0] = row_shr1(o.p23[0]);     // high half = the neighbour's v3 = this lane's column 4px-1
  o.m[1] = row_shr1(o.p23[1]);
}
}  // namespace

__global__ __launch_bounds__(64, 3) void stem_h3_kernel(StemArgs a) {
  const int H = a.H, W = a.W, PH = H >> 2, PW = W >> 2;
  const int strips = (PW - 1 + 14) / 15;
  const int bands = PH / a.R;                      // a.R divides PH
  const int wpi = strips * bands;                  // waves per image
  // workgroup ids are dealt round-robin to the 8 XCDs: give every XCD a contiguous range of waves, so that the waves of one
  // image (which share halo rows / columns and DRAM pages) sit behind one L2
  const int nwg = gridDim.x;
  const int wid = (nwg & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (nwg >> 3) + (int)(blockIdx.x >> 3);
  const int b = __builtin_amdgcn_readfirstlane(wid / wpi), wi = __builtin_amdgcn_readfirstlane(wid - b * wpi);
  const int strip = wi % strips, band = wi / strips;   // the strips of a band run side by side: their halo columns and partial lines meet in L2
  const int lane = threadIdx.x, p = lane & 15, g = lane >> 4;
  const int px = 15 * strip + p;
  const bool lvalid = px < PW;
  const int py0 = band * a.R;
  const bool st_ok = lvalid && (p > 0 || strip == 0);

  __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.x + (size_t)b * 3 * H * W * 4), 0, 3 * H * W * 4, 0x00020000);
  const int rowb = W * 4;
  constexpr int OOB = (int)0x80000000;
  // Every input value is loaded from memory ONCE: lane groups 0..2 load rows 2y and 2y+1 of their channel per conv row (row
  // 2y-1 is the previous conv row's 2y+1: its split form is carried), lane group 3 loads nothing - its three taps are
  // columns 4px+1 / 4px+3 of row 2y+1 of the three channels, which sit in the registers of lanes (p, 0..2): six
  // ds_bpermute_b32 per conv row.  (Loading them again instead - three more 16-byte loads per lane and row, all L2 hits -
  // cost 10 us of the launch's 120: measured with a memory-only build of this kernel.)
  const int chan_off = (lvalid && g < 3) ? g * H * rowb + 4 * px * 4 : OOB;
  const int src0 = (0 * 16 + p) * 4, src1 = (1 * 16 + p) * 4, src2 = (2 * 16 + p) * 4;   // ds_bpermute byte addresses of lanes (p, 0..2)

  // filter: [tile 2][term 2][64 lanes][4 dwords] fp16 pairs, then shift * 2^(sw+8) [32], then 2^-(sw+8)
  yfv2_h8 wa[2][2];
  {
    const u32x4* wimg = reinterpret_cast<const u32x4*>(a.img16);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int k = 0; k < 2; ++k) wa[t][k] = __builtin_bit_cast(yfv2_h8, wimg[(t * 2 + k) * 64 + lane]);
  }
  const float* cst = a.img16 + 2 * 2 * 64 * 4;
  const f32x4 sh0 = *reinterpret_cast<const f32x4*>(cst + 4 * g), sh1 = *reinterpret_cast<const f32x4*>(cst + 16 + 4 * g);
  const float unscale = cst[32];

  auto load_row = [&](int r) -> f32x4 {            // input row r of the lane's channel (zeros for lane group 3 / outside the image)
    const int off = (chan_off != OOB && r >= 0) ? chan_off + r * rowb : OOB;
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
  };
  auto load2 = [&](int y, f32x4 (&raw)[2]) { raw[0] = load_row(2 * y); raw[1] = load_row(2 * y + 1); };

  // conv row y from the carried row 2y-1 (x0) and the freshly loaded rows 2y, 2y+1 -> horizontally pooled raw values
  // hp[tile][4] = max(O[p-1], E[p], O[p]) (BN shift inside, pre-ReLU, x 2^(sw+8)); x0 <- the split row 2y+1
  Yfv2Watch watch;
  auto conv_row = [&](Row16& x0, const f32x4 (&raw)[2], f32x4 (&hp)[2]) {
    f32x4 r1 = raw[0], r2 = raw[1];
    {   // lane group 3: (ch0, ch1) of columns 4px+1 | 4px+3 into X1's v0 v1 | v2 v3, ch2 into X2's v0 | v2
      const int a1 = f2i(raw[1][1]), a3 = f2i(raw[1][3]);   // (by-value helper: bit_cast of a vector ELEMENT lvalue reads element 0 with this hipcc)
      const int e0 = __builtin_amdgcn_ds_bpermute(src0, a1), e1 = __builtin_amdgcn_ds_bpermute(src1, a1), e2 = __builtin_amdgcn_ds_bpermute(src2, a1);
      const int q0 = __builtin_amdgcn_ds_bpermute(src0, a3), q1 = __builtin_amdgcn_ds_bpermute(src1, a3), q2 = __builtin_amdgcn_ds_bpermute(src2, a3);
      if (g == 3) {
        r1 = (f32x4){i2f(e0), i2f(e1), i2f(q0), i2f(q1)};
        r2 = (f32x4){i2f(e2), 0.f, i2f(q2), 0.f};
      }
    }
    Row16 x1, x2;
    split_row(r1, x1); split_row(r2, x2);
    yfv2_h8 be[2], bo[2];                           // B operands of tile E / tile O, per term
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const u32x4 e = {x0.p01[k], x1.p01[k], pack_hi_hi(x0.m[k], x1.m[k]), pack_hi_lo(x2.m[k], x2.p01[k])};
      const u32x4 o = {x0.p23[k], x1.p23[k], pack_hi_hi(x0.p01[k], x1.p01[k]), pack_hi_lo(x2.p01[k], x2.p23[k])};
      be[k] = __builtin_bit_cast(yfv2_h8, e);
      bo[k] = __builtin_bit_cast(yfv2_h8, o);
    }
    x0 = x2;
    f32x4 ae[2] = {sh0, sh1}, ao[2] = {sh0, sh1};
    // w1 x2, w2 x1, w1 x1 - smallest terms first; the four accumulators of a product are independent
#pragma unroll
    for (int t = 0; t < 2; ++t) { ae[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], be[1], ae[t], 0, 0, 0); ao[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], bo[1], ao[t], 0, 0, 0); }
#pragma unroll
    for (int t = 0; t < 2; ++t) { ae[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][1], be[0], ae[t], 0, 0, 0); ao[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][1], bo[0], ao[t], 0, 0, 0); }
#pragma unroll
    for (int t = 0; t < 2; ++t) { ae[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], be[0], ae[t], 0, 0, 0); ao[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], bo[0], ao[t], 0, 0, 0); }
    watch.see(ae[0][0]); watch.see(ao[0][0]);   // every input column sits in an even or an odd window: a pixel beyond fp16's range makes both NaN
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e)     // 0 from the DPP at the image's left edge stands for the -inf padding: ReLU follows the pooling
        hp[t][e] = __builtin_fmaxf(__builtin_fmaxf(row_shr1(ao[t][e]), ae[t][e]), ao[t][e]);
  };

  // carried: hp of the odd conv row above the current pooled row (0 above the image: post-ReLU equivalent of the padding),
  // and the split form of the input row above the next conv row (zeros above the image = the conv's padding)
  f32x4 up[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  Row16 carry;
  // Two sets of row buffers: while a pooled row is computed from one set, the four loads of the NEXT pooled row fill the
  // other (bandwidth = bytes in flight / latency: one conv row of lookahead left the kernel at the old kernel's 4.3 TB/s)
  f32x4 re0[2], ro0[2], re1[2], ro1[2];
  if (py0 > 0) {
    f32x4 hb[2];
    const f32x4 top = load_row(4 * py0 - 3);       // row above conv row 2 py0 - 1
    load2(2 * py0 - 1, hb);
    load2(2 * py0, re0);
    load2(2 * py0 + 1, ro0);
    split_row(top, carry);
    conv_row(carry, hb, up);
  } else {
    load2(0, re0);
    load2(1, ro0);
    split_row((f32x4){0.f, 0.f, 0.f, 0.f}, carry);
  }
  // output [PH][PW][24]: a pixel's 96 bytes in one run, ONE 16-byte store per channel tile and lane group.  (Rounds 1-3 wrote 8-byte
  // pair-plane records, round 4's first half quad planes [6][PH][PW][4]: tools/ubench/stem_pattern.hip - this kernel's loads and
  // stores without its arithmetic - 139 / 123 / 118 us; stage2.0's loads cost the same from either layout.)
  float* __restrict__ ob = a.out + (((size_t)b * PH + py0) * PW + (st_ok ? px : 0)) * 24;
  const int ylast = (H >> 1) - 1;
  auto step = [&](int t, const f32x4 (&ce)[2], const f32x4 (&co)[2], f32x4 (&ne)[2], f32x4 (&no)[2]) {
    const int y = 2 * (py0 + t);
    load2(min(y + 2, ylast - 1), ne);              // next pooled row (past the image's end: a re-read that stays in range)
    load2(min(y + 3, ylast), no);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 h0[2], h1[2];
    conv_row(carry, ce, h0);
    conv_row(carry, co, h1);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m = __builtin_fmaxf(__builtin_fmaxf(up[tt][e], h0[tt][e]), h1[tt][e]);
        o[e] = __builtin_fmaxf(m, 0.f) * unscale;  // ReLU, then the exact power of two back
      }
      up[tt] = h1[tt];
      if (st_ok && (tt == 0 || g < 2)) *reinterpret_cast<f32x4*>(ob + 16 * tt + 4 * g) = o;   // channel tile 1 holds channels 16..23 in lane groups 0, 1
    }
    ob += (size_t)PW * 24;
  };
  int t = 0;
#pragma unroll 1
  for (; t + 1 < a.R; t += 2) {
    step(t, re0, ro0, re1, ro1);
    step(t + 1, re1, ro1, re0, ro0);
  }
  if (t < a.R) step(t, re0, ro0, re1, ro1);
  watch.report(a.nonfinite);
}

// ---- uint8 (B,H,W,3) input (yfv2_forward_u8 / yfv2_detect_u8: test.py:34-38's reshape / permute / float() / 255 folded into the loads).
// The same implicit GEMM with three simplifications: (1) a pixel 0..255 is EXACTLY one fp16 term, so a MAC is two products
// (w1 x, w2 x) instead of three; the 1/255 rides in the final unscale (2^-sw / 255, one rounding), the BN shift enters the
// accumulator as shift 2^sw 255; (2) HWC puts the three channels of a lane's four columns into ONE aligned 12-byte load, the
// same for the four lane groups of a pooled column: lane group g picks its channel's bytes with v_perm_b32 (selector per
// lane), and lane group 3 picks tap (2,2)'s six values out of its own load - no ds_bpermute; (3) u8 -> fp16 without a
// conversion instruction: 0x6400 | n is the fp16 number 1024 + n, one packed subtract gives n.  381 MB of input become 95.

namespace {
__device__ __forceinline__ void split_row_u8(const u32x3 d, unsigned sel_a, unsigned sel_b, Row8& o) {
  split_cols_u8(d, sel_a, sel_b, o);
  o.m = row_shr1(o.p23);
}
}  // namespace

__global__ __launch_bounds__(64, 4) void stem_h3u_kernel(StemArgs a) {
  const int H = a.H, W = a.W, PH = H >> 2, PW = W >> 2;
  const int strips = (PW - 1 + 14) / 15;
  const int bands = PH / a.R;
  const int wpi = strips * bands;
  const int nwg = gridDim.x;
  const int wid = (nwg & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (nwg >> 3) + (int)(blockIdx.x >> 3);
  const int b = __builtin_amdgcn_readfirstlane(wid / wpi), wi = __builtin_amdgcn_readfirstlane(wid - b * wpi);
  const int strip = wi % strips, band = wi / strips;
  const int lane = threadIdx.x, p = lane & 15, g = lane >> 4;
  const int px = 15 * strip + p;
  const bool lvalid = px < PW;
  const int py0 = band * a.R;
  const bool st_ok = lvalid && (p > 0 || strip == 0);

  __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.x + (size_t)b * 3 * H * W), 0, 3 * H * W, 0x00020000);
  const int rowb = W * 3;
  constexpr int OOB = (int)0x80000000;
  const int lane_off = lvalid ? 12 * px : OOB;      // columns 4px .. 4px+3, three channels each: 12 bytes, 4-byte aligned (W % 4 == 0)
  // byte selectors (v_perm_b32: indices 0..3 = the low source, 4..7 = the high one, 0x0c = zero).  Stream byte 3 c + ch is
  // channel ch of column 4px + c.  Pairs (v0, v1) come out of {d1, d0} (stream bytes 0..7), pairs (v2, v3) out of {d2, d1}
  // (stream bytes 4..11).  Lane group g < 3: channel g of columns 0..3, for X1 (row 2y) and X2 (row 2y+1) alike; lane group
  // 3: X1 = (ch0, ch1) of columns 1 | 3, X2 = (ch2, 0) of columns 1 | 3, both from row 2y+1 - tap (2,2) in slots 2, 3, 7.
  constexpr unsigned Z = 0x0c;
  const unsigned sel1a = g < 3 ? (unsigned)g | (Z << 8) | ((unsigned)(g + 3) << 16) | (Z << 24) : 3u | (Z << 8) | (4u << 16) | (Z << 24);
  const unsigned sel1b = g < 3 ? (unsigned)(g + 2) | (Z << 8) | ((unsigned)(g + 5) << 16) | (Z << 24) : 5u | (Z << 8) | (6u << 16) | (Z << 24);
  const unsigned sel2a = g < 3 ? sel1a : 5u | (Z << 8) | (Z << 16) | (Z << 24);
  const unsigned sel2b = g < 3 ? sel1b : 7u | (Z << 8) | (Z << 16) | (Z << 24);

  yfv2_h8 wa[2][2];
  {
    const u32x4* wimg = reinterpret_cast<const u32x4*>(a.img16);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int k = 0; k < 2; ++k) wa[t][k] = __builtin_bit_cast(yfv2_h8, wimg[(t * 2 + k) * 64 + lane]);
  }
  const float* cst = a.img16 + 2 * 2 * 64 * 4 + 36;   // the uint8 constants follow the fp32 ones: shift 2^sw 255 [32], 2^-sw / 255
  const f32x4 sh0 = *reinterpret_cast<const f32x4*>(cst + 4 * g), sh1 = *reinterpret_cast<const f32x4*>(cst + 16 + 4 * g);
  const float unscale = cst[32];

  auto load_row = [&](int r) -> u32x3 {
    const int off = (lane_off != OOB && r >= 0) ? lane_off + r * rowb : OOB;
    return __builtin_bit_cast(u32x3, __builtin_amdgcn_raw_buffer_load_b96(rsrc, off, 0, 0));
  };
  auto load2 = [&](int y, u32x3 (&raw)[2]) { raw[0] = load_row(2 * y); raw[1] = load_row(2 * y + 1); };

  auto conv_row = [&](Row8& x0, const u32x3 (&raw)[2], f32x4 (&hp)[2]) {
    const u32x3 s1 = g == 3 ? raw[1] : raw[0];
    Row8 x1, x2;
    split_row_u8(s1, sel1a, sel1b, x1);
    split_row_u8(raw[1], sel2a, sel2b, x2);
    const u32x4 e = {x0.p01, x1.p01, pack_hi_hi(x0.m, x1.m), pack_hi_lo(x2.m, x2.p01)};
    const u32x4 o = {x0.p23, x1.p23, pack_hi_hi(x0.p01, x1.p01), pack_hi_lo(x2.p01, x2.p23)};
    const yfv2_h8 be = __builtin_bit_cast(yfv2_h8, e), bo = __builtin_bit_cast(yfv2_h8, o);
    x0 = x2;
    f32x4 ae[2] = {sh0, sh1}, ao[2] = {sh0, sh1};
#pragma unroll
    for (int t = 0; t < 2; ++t) { ae[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][1], be, ae[t], 0, 0, 0); ao[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][1], bo, ao[t], 0, 0, 0); }
#pragma unroll
    for (int t = 0; t < 2; ++t) { ae[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], be, ae[t], 0, 0, 0); ao[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], bo, ao[t], 0, 0, 0); }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2)
        hp[t][e2] = __builtin_fmaxf(__builtin_fmaxf(row_shr1(ao[t][e2]), ae[t][e2]), ao[t][e2]);
  };

  f32x4 up[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  Row8 carry;
  u32x3 re0[2], ro0[2], re1[2], ro1[2];
  if (py0 > 0) {
    u32x3 hb[2];
    const u32x3 top = load_row(4 * py0 - 3);
    load2(2 * py0 - 1, hb);
    load2(2 * py0, re0);
    load2(2 * py0 + 1, ro0);
    split_row_u8(top, sel2a, sel2b, carry);        // a carried row is an X2
    conv_row(carry, hb, up);
  } else {
    load2(0, re0);
    load2(1, ro0);
    carry.p01 = carry.p23 = carry.m = 0u;
  }
  float* __restrict__ ob = a.out + (((size_t)b * PH + py0) * PW + (st_ok ? px : 0)) * 24;
  const int ylast = (H >> 1) - 1;
  auto step = [&](int t, const u32x3 (&ce)[2], const u32x3 (&co)[2], u32x3 (&ne)[2], u32x3 (&no)[2]) {
    const int y = 2 * (py0 + t);
    load2(min(y + 2, ylast - 1), ne);
    load2(min(y + 3, ylast), no);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 h0[2], h1[2];
    conv_row(carry, ce, h0);
    conv_row(carry, co, h1);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m = __builtin_fmaxf(__builtin_fmaxf(up[tt][e], h0[tt][e]), h1[tt][e]);
        o[e] = __builtin_fmaxf(m, 0.f) * unscale;
      }
      up[tt] = h1[tt];
      if (st_ok && (tt == 0 || g < 2)) *reinterpret_cast<f32x4*>(ob + 16 * tt + 4 * g) = o;
    }
    ob += (size_t)PW * 24;
  };
  int t = 0;
#pragma unroll 1
  for (; t + 1 < a.R; t += 2) {
    step(t, re0, ro0, re1, ro1);
    step(t + 1, re1, ro1, re0, ro0);
  }
  if (t < a.R) step(t, re0, ro0, re1, ro1);
}

void yfv2_launch_stem16(const StemArgs& a, hipStream_t s) {
  StemArgs b = a;
  const int PH = a.H / 4, PW = a.W / 4;
  int nb = 8;                                       // bands per image: R must divide PH
  while (nb > 1 && (PH % nb || PH / nb < 4)) nb >>= 1;
  b.R = PH / nb;
  const int strips = (PW - 1 + 14) / 15;
  const dim3 grid(a.B * strips * nb);
  if (a.u8_in) YFV2_LAUNCH(stem_h3u_kernel, grid, dim3(64), 0, s, b);
  else YFV2_LAUNCH(stem_h3_kernel, grid, dim3(64), 0, s, b);
}
