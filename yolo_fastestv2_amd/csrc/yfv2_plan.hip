// yfv2_plan.hip - the forward launch plan (yfv2_plan.h): PlanBuilder turns a configuration into the list of launches and
// decides which packed images enter the blob, in which order; plan_run enqueues the list.  Host only: no kernel.
// Reference dataflow followed by the plan (behaviour only): model/backbone/shufflenetv2.py:102-109, model/fpn.py:51-64,
// model/detector.py:21-47.
#include "yfv2_plan.h"

#include <algorithm>
#include <utility>

thread_local Yfv2LaunchProbe yfv2_launch_probe;   // (yfv2_internal.h: YFV2_LAUNCH)

namespace {

template <class K> K* kind_of(Step& s) { return std::get_if<K>(&s.kind); }
template <class K> const K* kind_of(const Step& s) { return std::get_if<K>(&s.kind); }
// a tower step that is still one half (what tower_half emits; merge_tower_launches joins them)
const TowerHalf* lone_half(const Step& s) {
  const TowerStep* t = kind_of<TowerStep>(s);
  return t && t->halves.size() == 1 ? &t->halves[0] : nullptr;
}
// the step is towerp_kernel's under the default arithmetic (yfv2_launch_towerh routes by the same predicate)
bool towerp_step(const TowerStep& k) { return k.halves[0].img16 && yfv2_towerp_map(k.halves[0].args.H, k.halves[0].args.W); }
double half_flops(const TowerHalf& t) { return 2.0 * t.args.H * t.args.W * (25.0 * 72 + 72.0 * 72 + (t.has_head ? 72.0 * t.args.mh : 0.0)); }
double half_bytes(const TowerHalf& t) { return 4.0 * t.args.H * t.args.W * (72.0 + (t.has_head ? t.args.mh : 72.0)); }

struct PlanBuilder {
  const yfv2_config& cfg;
  const PlanSwitches& sw;
  const Workspace& ws;
  WeightPacker& wp;
  Plan plan;
  bool ok = true;

  static PwStep& pw(Step& s) { return std::get<PwStep>(s.kind); }
  template <class K>
  Step& push(Step& s, K k) {
    s.kind = std::move(k);
    plan.steps.push_back(std::move(s));
    return plan.steps.back();
  }

  void add_stem(const Buf& out, bool pp_out) {
    Folded f;
    wp.stem("backbone.first_conv.0", "backbone.first_conv.1", &f);
    Step s;
    StemStep kd;
    kd.args.out = out.p;
    kd.args.H = cfg.height;
    kd.args.W = cfg.width;
    kd.args.R = 0;  // bands are chosen by the launcher
    kd.args.pp_out = pp_out ? 1 : 0;
    kd.img = wp.image_stem(f);
    kd.img_u8 = wp.image_stem(f, 1.0f / 255.0f);
    kd.img16 = wp.image_stem16(f);
    s.name = "stem conv3x3s2+bn+relu+maxpool3x3s2";
    const double ch = cfg.height / 2.0, cw = cfg.width / 2.0;
    s.flops = 2.0 * ch * cw * 27 * 24;
    s.bytes = 4.0 * (3.0 * cfg.height * cfg.width + (ch / 2) * (cw / 2) * 24);
    push(s, kd);
  }

  // generic pointwise launch; bn_name empty => Folded given by caller (heads)
  Step& add_pw(const std::string& name, int K, int mode, int M, int px, const float* in, int in_stride, int in_off,
               float* out, int out_stride, int out_off, bool relu, const Folded& f) {
    Step s;
    PwStep kd;
    kd.K = K; kd.mode = mode;
    kd.args.in = in; kd.args.in2 = nullptr; kd.args.out = out;
    kd.args.M = M;
    kd.args.in_stride = in_stride; kd.args.in_off = in_off;
    kd.args.out_stride = out_stride; kd.args.out_off = out_off;
    kd.args.relu = relu ? 1 : 0;
    kd.args.copy = nullptr; kd.args.copy_stride = 0; kd.args.copy_off = 0;
    kd.args.H = 0; kd.args.W = 0; kd.args.HW = px;
    kd.args.nchw0 = nullptr; kd.args.nchw1 = nullptr; kd.args.split = 0; kd.args.ctot0 = 0; kd.args.coff0 = 0;
    kd.px_per_img = px;
    kd.args.presplit = (sw.bf6 && yfv2_pw_presplit_supported(K, mode, M)) ? 1 : 0;
    kd.img = wp.image_pw(f, M, K, yfv2_pw_tiles(K, mode, M), kd.args.presplit != 0);
    s.name = name;
    s.flops = 2.0 * px * K * M;
    s.bytes = 4.0 * px * (K + M);
    return push(s, kd);
  }

  void add_dw(const std::string& name, int ksize, int stride, int C, int H, int W, const float* in, int in_stride,
              float* out, int out_stride, bool relu, const Folded& f) {
    Step s;
    DwStep kd;
    kd.ksize = ksize; kd.stride = stride;
    kd.args.in = in; kd.args.out = out;
    kd.args.H = H; kd.args.W = W; kd.args.C = C;
    kd.args.OH = H / stride; kd.args.OW = W / stride;
    kd.args.in_stride = in_stride; kd.args.in_off = 0;
    kd.args.out_stride = out_stride; kd.args.out_off = 0;
    kd.args.relu = relu ? 1 : 0;
    kd.w = f.w; kd.scale = f.scale; kd.shift = f.shift;
    s.name = name;
    s.flops = 2.0 * kd.args.OH * kd.args.OW * C * ksize * ksize;
    s.bytes = 4.0 * C * ((double)H * W + (double)kd.args.OH * kd.args.OW);
    push(s, kd);
  }

  // ShuffleV2Block stride 2 (shufflenetv2.py:19-44,52-55): out = cat(proj(x), main(x))
  // pp_label != nullptr: the input is stage 2's pair-plane layout (slot k holds logical channel pp_label[k],
  // pair p lives in buffer pp_buf[p]); only the fused kernel reads it
  // in_label != nullptr: the NHWC input holds logical channel in_label[k] at position k (stage 3 written by the chain kernel)
  void block_s2(const std::string& p, int cin, int H, int W, const Buf& x, const Buf& y, const int* pp_label = nullptr,
                const int* pp_buf = nullptr, long long pp_bufstride = 0, const int* in_label = nullptr) {
    Folded f;
    const int oh = H / 2, ow = W / 2, co = 2 * cin;
    const bool layer_plan = sw.plan.layer_by_layer != 0;
    const int rfused = (cin == 24 || cin == 48 || (cin == 96 && !pp_label && sw.bf6)) ? yfv2_block_s2_rows(cin, H, W) : 0;   // 96: block_s2w_kernel (its pw1 is bf16x6 only)
    if (!layer_plan && rfused > 0) {
      Folded f1, fd, f2, fpd, fpp;
      wp.dw(p + ".branch_proj.0", p + ".branch_proj.1", cin, 3, &fpd);
      wp.pw(p + ".branch_proj.2", p + ".branch_proj.3", cin, cin, &fpp);
      wp.pw(p + ".branch_main.0", p + ".branch_main.1", cin, cin, &f1);
      wp.dw(p + ".branch_main.3", p + ".branch_main.4", cin, 3, &fd);
      wp.pw(p + ".branch_main.5", p + ".branch_main.6", cin, cin, &f2);
      Step s;
      S2Step kd;
      kd.cin = cin;
      kd.args.in = x.p; kd.args.out = y.p;
      kd.args.H = H; kd.args.W = W; kd.args.R = rfused;
      if (pp_label && ok) {  // channel position k of the staged tile = slot k: re-order every per-input-channel parameter
        f1 = wp.permuted_pw_inputs(f1, cin, cin, pp_label);
        fpd = wp.permuted_dw_channels(fpd, cin, 9, pp_label);
        fpp = wp.permuted_pw_inputs(fpp, cin, cin, pp_label);
        kd.args.pp_in = 1;
        kd.args.pp_bufstride = pp_bufstride;
        kd.args.pp_imgstride = 2 * pp_bufstride;
        for (int q = 0; q < cin / 2; ++q) if (pp_buf[q]) kd.args.pp_mask |= 1u << q;
      } else if (in_label && ok) {
        f1 = wp.permuted_pw_inputs(f1, cin, cin, in_label);
        fpd = wp.permuted_dw_channels(fpd, cin, 9, in_label);
        fpp = wp.permuted_pw_inputs(fpp, cin, cin, in_label);
      }
      kd.img = cin == 96 ? wp.image_s2w(f1, fd, f2, fpd, fpp) : wp.image_s2(f1, fd, f2, fpd, fpp, cin);
      if (cin == 48 && pp_label && ok && sw.bf6 && yfv2_s3h_supported(H, W))   // the streaming form on the f16 matrix cores (yfv2_stage2h.hip)
        kd.img16 = wp.image_s3h(f1, fd, f2, fpd, fpp, kd.args.pp_mask, pp_bufstride, H, W);
      if (cin == 96 && !pp_label && ok && sw.bf6 && yfv2_s4h_supported(H, W))
        kd.img16 = wp.image_s4h(f1, fd, f2, fpd, fpp);
      s.name = p + " fused s2 block: proj(dw3x3s2+bn -> pw+bn+relu) | main(pw1+bn+relu -> dw3x3s2+bn -> pw2+bn+relu) | cat";
      s.flops = 2.0 * ((double)H * W * cin * cin + 2.0 * oh * ow * cin * cin + 2.0 * oh * ow * 9 * cin);
      s.bytes = 4.0 * ((double)H * W * cin + (double)oh * ow * co);
      push(s, kd);
      return;
    }
    wp.dw(p + ".branch_proj.0", p + ".branch_proj.1", cin, 3, &f);
    if (in_label && ok) f = wp.permuted_dw_channels(f, cin, 9, in_label);
    add_dw(p + ".proj.dw3x3s2+bn", 3, 2, cin, H, W, x.p, cin, ws.t3.p, cin, false, f);
    wp.pw(p + ".branch_proj.2", p + ".branch_proj.3", cin, cin, &f);
    if (in_label && ok) f = wp.permuted_pw_inputs(f, cin, cin, in_label);
    add_pw(p + ".proj.pw+bn+relu", cin, PW_PLAIN, cin, oh * ow, ws.t3.p, cin, 0, y.p, co, 0, true, f);
    wp.pw(p + ".branch_main.0", p + ".branch_main.1", cin, cin, &f);
    if (in_label && ok) f = wp.permuted_pw_inputs(f, cin, cin, in_label);
    add_pw(p + ".main.pw1+bn+relu", cin, PW_PLAIN, cin, H * W, x.p, cin, 0, ws.t1.p, cin, 0, true, f);
    wp.dw(p + ".branch_main.3", p + ".branch_main.4", cin, 3, &f);
    add_dw(p + ".main.dw3x3s2+bn", 3, 2, cin, H, W, ws.t1.p, cin, ws.t2.p, cin, false, f);
    wp.pw(p + ".branch_main.5", p + ".branch_main.6", cin, cin, &f);
    add_pw(p + ".main.pw2+bn+relu", cin, PW_PLAIN, cin, oh * ow, ws.t2.p, cin, 0, y.p, co, cin, true, f);
  }

  // ---- stage 2 in lane-per-pixel form (yfv2_stage2.hip).  Bookkeeping of the pair-plane layout:
  // label[slot] = logical channel (numbered as the input of the NEXT block) stored in slot 2*pair + element,
  // buf[pair] = which of the two stage buffers holds the pair.  A stride-1 block (shufflenetv2.py:57-63,
  // 48-51) sends its even input channels 2j to output channel j untouched and its odd input channels 2i+1
  // through the branch to output channel c2+i: in slot terms the even-labelled pairs are simply re-labelled
  // (label /= 2) and the odd-labelled pairs are read, transformed and written to the OTHER buffer's copy of
  // the same pair (no in-place halo races), re-labelled c2 + (label-1)/2.  yfv2_stage2_channel() places the
  // stride-2 block's 48 outputs so that every pair stays wholly even or wholly odd for all three blocks.
  struct Stage2Layout {
    int label[48];
    int buf[24];
  };
  // stage2.0 in lane-per-pixel form: reads the stem's pair planes, writes logical channel c to slot(c) of buffer 0
  void s2px_block(const std::string& p, int IH, int IW) {
    Folded f1, fd, f2, fpd, fpp;
    wp.dw(p + ".branch_proj.0", p + ".branch_proj.1", 24, 3, &fpd);
    wp.pw(p + ".branch_proj.2", p + ".branch_proj.3", 24, 24, &fpp);
    wp.pw(p + ".branch_main.0", p + ".branch_main.1", 24, 24, &f1);
    wp.dw(p + ".branch_main.3", p + ".branch_main.4", 24, 3, &fd);
    wp.pw(p + ".branch_main.5", p + ".branch_main.6", 24, 24, &f2);
    const int OH = IH / 2, OW = IW / 2;
    int slot_of[48];
    for (int k = 0; k < 48; ++k) slot_of[yfv2_stage2_channel(k)] = k;
    Step s;
    S2PxStep kd;
    // output positions: 0..15 = the role's eight whole pairs, 16..23 = its halves of the eight mixed pairs
    int pos[2][24];
    for (int j = 0; j < 8; ++j) {
      pos[0][2 * j] = j;      pos[0][2 * j + 1] = 8 + j;   pos[0][16 + j] = 16 + j;   // proj: logical channels 0..23
      pos[1][2 * j] = 8 + j;  pos[1][2 * j + 1] = 16 + j;  pos[1][16 + j] = j;        // main: logical 24 + (..)
    }
    for (int role = 0; role < 2; ++role) {
      for (int i = 0; i < 8; ++i) {
        const int s0 = slot_of[24 * role + pos[role][2 * i]], s1 = slot_of[24 * role + pos[role][2 * i + 1]];
        if ((s0 & 1) || s1 != s0 + 1) { ok = false; return; }
        kd.args.st2_off[role][i] = (s0 >> 1) * OH * OW * 8;
        const int ss = slot_of[24 * role + pos[role][16 + i]];
        kd.args.st1_off[role][i] = (ss >> 1) * OH * OW * 8 + (ss & 1) * 4;
      }
    }
    kd.args.in = ws.a1.p; kd.args.act = ws.s2pp.p;
    kd.args.IH = IH; kd.args.IW = IW;
    kd.args.in_stride = 24 * IH * IW; kd.args.out_stride = 2 * 48 * OH * OW;   // (an image owns both of its stage-2 buffers; this block fills buffer 0)
    kd.args.in_records = 24 * IH * IW * 4; kd.args.out_records = 48 * OH * OW * 4;
    if (ok) {
      kd.img_proj = wp.image_s2px_proj(fpd, fpp, pos[0]); kd.img_main = wp.image_s2px_main(f1, fd, f2, pos[1]);
      for (int i = 0; i < 8; ++i)   // s2h_kernel stores a mixed pair whole: proj must sit in element 0, main right behind it
        if ((kd.args.st1_off[0][i] & 7) != 0 || kd.args.st1_off[1][i] != kd.args.st1_off[0][i] + 4) ok = false;
      if (ok) kd.img16 = wp.image_s2h(f1, fd, f2, fpd, fpp, pos, kd.args.st2_off, kd.args.st1_off, IH, IW);
    }
    s.name = p + " s2 block, lane-per-pixel: proj(dw3x3s2+bn -> pw+bn+relu) | main(pw1+bn+relu -> dw3x3s2+bn -> pw2+bn+relu) -> pair planes";
    s.flops = 2.0 * ((double)IH * IW * 24 * 24 + 2.0 * OH * OW * 24 * 24 + 2.0 * OH * OW * 9 * 24);
    s.bytes = 4.0 * ((double)IH * IW * 24 + (double)OH * OW * 48);
    push(s, kd);
  }
  void s1px_block(const std::string& p, int H, int W, Stage2Layout& L, long long bufstride) {
    Folded f1, fd, f2;
    wp.pw(p + ".branch_main.0", p + ".branch_main.1", 24, 24, &f1);
    wp.dw(p + ".branch_main.3", p + ".branch_main.4", 24, 3, &fd);
    wp.pw(p + ".branch_main.5", p + ".branch_main.6", 24, 24, &f2);
    Step s;
    S1PxStep kd;
    int order[24], kk = 0;
    for (int q = 0; q < 24; ++q) {
      const bool odd0 = L.label[2 * q] & 1, odd1 = L.label[2 * q + 1] & 1;
      if (odd0 != odd1) { ok = false; return; }   // cannot happen with yfv2_stage2_channel's placement
      if (!odd0) continue;
      if (kk >= 12) { ok = false; return; }
      order[2 * kk] = (L.label[2 * q] - 1) / 2;
      order[2 * kk + 1] = (L.label[2 * q + 1] - 1) / 2;
      kd.args.src_off[kk] = (int)(((long long)L.buf[q] * bufstride + (long long)q * H * W * 2) * 4);
      kd.args.dst_off[kk] = (int)(((long long)(1 - L.buf[q]) * bufstride + (long long)q * H * W * 2) * 4);
      ++kk;
    }
    if (kk != 12) { ok = false; return; }
    for (int q = 0; q < 24; ++q) {
      if (L.label[2 * q] & 1) {
        L.label[2 * q] = 24 + (L.label[2 * q] - 1) / 2;
        L.label[2 * q + 1] = 24 + (L.label[2 * q + 1] - 1) / 2;
        L.buf[q] ^= 1;
      } else {
        L.label[2 * q] /= 2;
        L.label[2 * q + 1] /= 2;
      }
    }
    kd.args.act = ws.s2pp.p;
    kd.args.H = H; kd.args.W = W;
    kd.args.img_stride = 2 * 48 * H * W;
    kd.args.num_records = (int)((bufstride + 48LL * H * W) * 4);
    if (ok) { kd.img = wp.image_s1px(f1, fd, f2, order); kd.img16 = wp.image_s1h(f1, fd, f2, order, kd.args.src_off, kd.args.dst_off); }
    s.name = p + " s1 block, lane-per-pixel: pw1+bn+relu -> dw3x3+bn -> pw2+bn+relu on the 12 branch pairs (shuffle/pass/cat = bookkeeping)";
    s.flops = 2.0 * H * W * (2.0 * 24 * 24 + 9.0 * 24);
    s.bytes = 4.0 * H * W * (2.0 * 48);  // the layer's logical input + output; the launch itself moves half of it
    s.bytes_ext = 4.0 * H * W * (2.0 * 24);   // the 12 branch pairs in, the 12 fresh pairs out; the pass-through half never moves
    push(s, kd);
  }

  // ---- a chain of stride-1 blocks as ONE launch (block_s1chain_kernel, yfv2_block.hip).  The kernel moves data in a
  // fixed, lane-uniform way (pixel slot owned by the 4 lanes g of a 16-lane row; per block and lane: accumulator elements
  // 1, 3 -> next tile, element 0 -> held one block, element 2 -> parked in Z; next tile quads = (held 3 + parked 1 |
  // parked 2 + fresh 2 | fresh 4)); this planner decides which LOGICAL channel each of those positions carries so that
  // the whole thing is the reference's channel_shuffle / pass-through / cat chain (shufflenetv2.py:48-51,57-63):
  //   logical activation A_k (96 channels) before block k:  branch input i = A_k[2i+1],  A_{k+1} = [A_k[0::2], F_k]
  // A fresh output F_k[j] (index 48 + j in A_{k+1}) becomes a branch input after L blocks, L = 1 + trailing zeros of its
  // index: odd j at once (24 values -> elements 1, 3), j = 2 mod 4 after one pass (12 -> element 0), j = 0 mod 4 later
  // (12 -> element 2, parked).  X[2i+1] feed block 1 from the load, X[4i+2] are held for block 2, X[4i] stay in memory.
  // Outputs: the blocks' images (pw1 input columns / pw2 output rows permuted, tables PS / PL appended) and
  // z_label[pos] = logical channel of the chain's output stored at Z position pos.
  struct ChainLoc { int kind = 0, blk = 0, mt = 0, g = 0, e = 0, off = 0; };   // kind 0: X[off] (loaded up front), 1: accumulator of block blk, 2: parked at Z[off]
  void s1chain_block(const std::vector<std::string>& names, int c, int H, int W, const Buf& x, const Buf& y, int* z_label) {
    const int c2 = c / 2, NB = (int)names.size();
    std::vector<Folded> f1(NB), fd(NB), f2(NB);
    for (int k = 0; k < NB; ++k) {
      wp.pw(names[k] + ".branch_main.0", names[k] + ".branch_main.1", c2, c2, &f1[k]);
      wp.dw(names[k] + ".branch_main.3", names[k] + ".branch_main.4", c2, 3, &fd[k]);
      wp.pw(names[k] + ".branch_main.5", names[k] + ".branch_main.6", c2, c2, &f2[k]);
    }
    std::vector<float> im;
    if (ok && c2 == 48 && NB >= 3 && NB <= 7) {
      // Z positions: [12 (k - 2), + 12) = the parked inputs of block k (k = 2 .. NB-1; all of it below 60 and free until
      // the final stores), [60, 96) = parked values no block consumes (they are already where the output wants them)
      std::vector<int> group_n(NB, 0);
      int next_final = 60;
      // consumer of the value that has index idx in the activation entering block kn: the block that takes it as a
      // branch input, or NB if it survives the chain
      auto consumer = [&](int idx, int kn) {
        int steps = 0;
        while (!(idx & 1) && idx != 0) { idx >>= 1; ++steps; }
        return (idx == 0 || kn + steps > NB - 1) ? NB : kn + steps;
      };
      // n consecutive Z positions for values with consumer kc
      auto park_slots = [&](int kc, int n) {
        if (kc >= NB) { const int p0 = next_final; next_final += n; if (next_final > 96) ok = false; return p0; }
        if (kc < 2 || group_n[kc] + n > 12) { ok = false; return 0; }
        const int p0 = 12 * (kc - 2) + group_n[kc];
        group_n[kc] += n;
        return p0;
      };
      std::vector<ChainLoc> act(96);                     // where logical channel o of the current activation lives
      std::vector<std::vector<int>> tables(NB, std::vector<int>(36, 0));   // per block: PS[i][g] | (block 0) XS[c][g]
      for (int o = 0; o < 96; ++o) { act[o].kind = 0; act[o].off = o; }
      // X[16 cq + 4 g] are parked at load time.  Lane groups 1..3: the kernel stores (cq = 0,1,2) and (cq = 3,4,5) as two
      // 12-byte runs, so each triple must share a consumer; lane group 0: six single dwords (X[0] passes every block: Z[95])
      for (int g = 0; g < 4 && ok; ++g) {
        if (g == 0) {
          for (int cq = 0; cq < 6; ++cq) {
            const int o = 16 * cq;
            act[o].kind = 2;
            act[o].off = o == 0 ? 95 : park_slots(consumer(o, 0), 1);
            tables[0][12 + cq * 4 + 0] = act[o].off;
          }
          if (next_final > 95) ok = false;                // Z[95] is X[0]'s
        } else {
          for (int t = 0; t < 2; ++t) {
            const int kc = consumer(16 * (3 * t) + 4 * g, 0);
            for (int i = 1; i < 3; ++i) if (consumer(16 * (3 * t + i) + 4 * g, 0) != kc) ok = false;
            const int p0 = park_slots(kc, 3);
            for (int i = 0; i < 3; ++i) {
              const int o = 16 * (3 * t + i) + 4 * g;
              act[o].kind = 2; act[o].off = p0 + i;
              tables[0][12 + (3 * t + i) * 4 + g] = p0 + i;
            }
          }
        }
      }
      auto tile_of_fresh = [](int mt, int e) {           // accumulator (mt, element 1 | 3) -> tile (quad j, element)
        const int hi = e == 3 ? 1 : 0;
        if (mt == 0) return std::make_pair(1, 2 + hi);
        if (mt == 1) return std::make_pair(2, 0 + hi);
        return std::make_pair(2, 2 + hi);
      };
      for (int k = 0; k < NB && ok; ++k) {
        // ---- where does branch input i of this block sit in the tile?  label[physical column 16 j + 4 g + e] = i
        int label[48];
        for (int q = 0; q < 48; ++q) label[q] = -1;
        int parked_n = 0;
        for (int i = 0; i < 48; ++i) {
          const ChainLoc& L = act[2 * i + 1];
          int j = -1, g = -1, e = -1;
          if (k == 0) {                                   // loaded from X: quad cq = off / 16, lane group, element 1 | 3
            if (L.kind != 0 || !(L.off & 1)) { ok = false; break; }
            const int cq = L.off / 16; g = (L.off % 16) / 4;
            j = cq / 2; e = (cq & 1) * 2 + ((L.off & 3) == 3 ? 1 : 0);
          } else if (L.kind == 1 && L.blk == k - 1 && (L.e == 1 || L.e == 3)) {   // fresh output of the previous block
            const auto t = tile_of_fresh(L.mt, L.e); j = t.first; e = t.second; g = L.g;
          } else if (k == 1 && L.kind == 0 && (L.off & 3) == 2) {                  // X element 2, held since the load
            const int cq = L.off / 16; g = (L.off % 16) / 4;
            if (cq < 4) { j = 0; e = cq; } else { j = 1; e = cq - 4; }
          } else if (k >= 2 && L.kind == 1 && L.blk == k - 2 && L.e == 0) {        // element 0 of the block before the previous one
            j = 0; g = L.g; e = L.mt;
          } else if (k >= 2 && L.kind == 2 && L.off >= 12 * (k - 2) && L.off < 12 * (k - 2) + 12) {   // parked in this block's group
            const int n = L.off - 12 * (k - 2), pi = n % 3;
            g = n / 3; ++parked_n;
            if (pi == 0) { j = 0; e = 3; } else { j = 1; e = pi - 1; }
          } else { ok = false; break; }
          if (label[16 * j + 4 * g + e] != -1) { ok = false; break; }
          label[16 * j + 4 * g + e] = i;
        }
        if (!ok) break;
        if (k >= 2 && parked_n != 12) { ok = false; break; }
        for (int q = 0; q < 48; ++q) if (label[q] < 0) ok = false;
        if (!ok) break;
        // ---- which logical fresh channel lands in accumulator (mt, g, e)?  rowlab[16 mt + 4 g + e] = j
        int rowlab[48];
        if (k == NB - 1) {
          for (int q = 0; q < 48; ++q) rowlab[q] = q;   // last block: natural order (Z[0..47] = logical 48..95)
        } else {
          int n13 = 0, n0 = 0;
          for (int j = 0; j < 48; ++j) {
            if ((j & 3) == 0) continue;
            int slot, e;
            if (j & 1) { slot = n13 / 2; e = (n13 & 1) ? 3 : 1; ++n13; }
            else { slot = n0++; e = 0; }
            rowlab[16 * (slot / 4) + 4 * (slot % 4) + e] = j;   // slot = 4 mt + g
          }
          // the twelve j = 0 mod 4 go to elements 2: lane groups 0..2 get three values with ONE consumer each (the kernel
          // parks them with one 12-byte store), lane group 3 takes whatever is left (three dwords)
          std::vector<std::vector<int>> by_consumer(NB + 1);
          for (int j = 0; j < 48; j += 4) by_consumer[consumer(48 + j, k + 1)].push_back(j);
          std::vector<std::vector<int>> triples;
          std::vector<int> left;
          for (auto& v : by_consumer) {
            size_t t = 0;
            for (; t + 3 <= v.size(); t += 3) triples.push_back({v[t], v[t + 1], v[t + 2]});
            for (; t < v.size(); ++t) left.push_back(v[t]);
          }
          while (triples.size() > 3) { for (int q : triples.back()) left.push_back(q); triples.pop_back(); }
          if (triples.size() != 3 || left.size() != 3) { ok = false; break; }
          for (int g = 0; g < 3; ++g)
            for (int mt = 0; mt < 3; ++mt) rowlab[16 * mt + 4 * g + 2] = triples[g][mt];
          for (int mt = 0; mt < 3; ++mt) rowlab[16 * mt + 4 * 3 + 2] = left[mt];
        }
        const Folded f1k = wp.permuted_pw_inputs(f1[k], c2, c2, label);
        const Folded f2k = wp.permuted_pw_outputs(f2[k], c2, c2, rowlab);
        // ---- next activation; park positions of the element-2 values
        std::vector<ChainLoc> nxt(96);
        for (int i = 0; i < 48; ++i) nxt[i] = act[2 * i];
        int trip_base[3] = {0, 0, 0};
        if (k < NB - 1)
          for (int g = 0; g < 3; ++g) trip_base[g] = park_slots(consumer(48 + rowlab[4 * g + 2], k + 1), 3);   // its three share the consumer
        for (int q = 0; q < 48; ++q) {
          const int mt = q / 16, g = (q % 16) / 4, e = q % 4, j = rowlab[q];
          ChainLoc L; L.kind = 1; L.blk = k; L.mt = mt; L.g = g; L.e = e;
          if (k < NB - 1 && e == 2) {
            L.kind = 2;
            L.off = g < 3 ? trip_base[g] + mt : park_slots(consumer(48 + j, k + 1), 1);
            tables[k][mt * 4 + g] = L.off;
          }
          nxt[48 + j] = L;
        }
        act.swap(nxt);
        wp.append_s1_bf6(im, f1k, fd[k], f2k);
        for (int t = 0; t < 64; ++t) WeightPacker::push_bits(im, t < 36 ? tables[k][t] : 0);   // int tables as raw bits behind the BN vectors
      }
      if (ok) {
        for (int k = 2; k < NB; ++k) if (group_n[k] != 12) ok = false;
        // ---- where the chain's output lives in Z
        for (int pos = 0; pos < 96; ++pos) z_label[pos] = -1;
        for (int o = 0; o < 96 && ok; ++o) {
          const ChainLoc& L = act[o];
          int pos = -1;
          if (L.kind == 1 && L.blk == NB - 1) pos = 16 * L.mt + 4 * L.g + L.e;               // last block's accumulators
          else if (L.kind == 1 && L.blk == NB - 2 && L.e == 0) pos = 48 + 3 * L.g + L.mt;    // held elements of the block before
          else if (L.kind == 2 && L.off >= 60) pos = L.off;
          if (pos < 0 || z_label[pos] != -1) { ok = false; break; }
          z_label[pos] = o;
        }
        if ((int)(im.size() / NB) != yfv2_s1chain_image_floats()) ok = false;
      }
    } else {
      ok = false;
    }
    Step s;
    S1Step kd;
    kd.args.in = x.p; kd.args.out = y.p;
    kd.args.H = H; kd.args.W = W; kd.args.R = H; kd.args.nblk = NB;
    kd.args.presplit = 1;
    kd.args.park = ws.t1.p;     // a temporary of the layer-by-layer blocks: nothing else runs while the chain does
    if ((size_t)yfv2_s1chain_park_floats(H, W, NB) > ws.t1.per_img) ok = false;
    kd.img = wp.put(im);
    s.name = names.front() + " .. " + names.back().substr(names.back().rfind('.') + 1) + " chain of " + std::to_string(NB) +
             " fused s1 blocks in one launch (activations between them stay on chip)";
    s.flops = NB * 2.0 * H * W * (2.0 * c2 * c2 + 9.0 * c2);
    s.bytes = NB * 4.0 * H * W * (2.0 * c);   // per-layer accounting: every block reads and writes c channels
    s.bytes_ext = 4.0 * H * W * (2.0 * c);    // the launch reads the activation once and writes it once (parked dwords are internal traffic)
    push(s, kd);
  }

  // ---- a chain of stride-1 blocks with the whole activation resident in LDS (block_s1pool_kernel, yfv2_block.hip): natural
  // channel order, no bookkeeping - the image is WeightPacker::image_s1pool's
  void s1pool_block(const std::vector<std::string>& names, int c, int H, int W, const Buf& x, const Buf& y) {
    const int c2 = c / 2, NB = (int)names.size();
    const bool pre = sw.bf6;   // bf16x6 on pre-split filters; YFV2_BF6=0: the fp32-MFMA form of the same kernel
    std::vector<Folded> f1, fd, f2;
    for (int k = 0; k < NB && ok; ++k) {
      Folded a, d, b;
      wp.pw(names[k] + ".branch_main.0", names[k] + ".branch_main.1", c2, c2, &a);
      wp.dw(names[k] + ".branch_main.3", names[k] + ".branch_main.4", c2, 3, &d);
      wp.pw(names[k] + ".branch_main.5", names[k] + ".branch_main.6", c2, c2, &b);
      if (ok) { f1.push_back(a); fd.push_back(d); f2.push_back(b); }
    }
    Step s;
    S1Step kd;
    kd.pool = true;
    kd.args.in = x.p; kd.args.out = y.p;
    kd.args.H = H; kd.args.W = W; kd.args.R = H; kd.args.nblk = NB;
    kd.args.presplit = pre ? 1 : 0;
    kd.img = wp.image_s1pool(f1, fd, f2, c2, pre, &ok);
    s.name = names.front() + " .. " + names.back().substr(names.back().rfind('.') + 1) + " chain of " + std::to_string(NB) +
             " fused s1 blocks in one launch (whole activation resident in LDS)";
    s.flops = NB * 2.0 * H * W * (2.0 * c2 * c2 + 9.0 * c2);
    s.bytes = NB * 4.0 * H * W * (2.0 * c);
    s.bytes_ext = 4.0 * H * W * (2.0 * c);
    push(s, kd);
  }

  // ShuffleV2Block stride 1 (shufflenetv2.py:48-51,57-63), layer by layer: even channels pass through (copied by the pw1
  // launch), odd channels -> main; out = cat(pass, main).  The general plan for shapes the chains do not cover.
  void block_s1(const std::string& p, int c, int H, int W, const Buf& x, const Buf& y) {
    Folded f;
    const int c2 = c / 2;
    wp.pw(p + ".branch_main.0", p + ".branch_main.1", c2, c2, &f);
    Step& s = add_pw(p + ".shuffle+pass+main.pw1+bn+relu", c2, PW_SHUFFLE, c2, H * W, x.p, c, 0, ws.t1.p, c2, 0, true, f);
    pw(s).args.copy = y.p; pw(s).args.copy_stride = c; pw(s).args.copy_off = 0;
    s.bytes = 4.0 * H * W * (c + c2 + c2);  // reads both halves, writes pass-through half + pw1 output
    wp.dw(p + ".branch_main.3", p + ".branch_main.4", c2, 3, &f);
    add_dw(p + ".main.dw3x3+bn", 3, 1, c2, H, W, ws.t1.p, c2, ws.t2.p, c2, false, f);
    wp.pw(p + ".branch_main.5", p + ".branch_main.6", c2, c2, &f);
    add_pw(p + ".main.pw2+bn+relu", c2, PW_PLAIN, c2, H * W, ws.t2.p, c2, 0, y.p, c, c2, true, f);
  }

  // Maps larger than 11x11 run a tower half per launch (towerh_kernel's 2x2-patch form).  The cls and the reg tower of a level are
  // independent of each other, so their a halves (both read the FPN map) and their b halves (each reads its own a half) go side
  // by side as workgroup ranges of ONE launch each: four launches -> two, and a CU starts its next workgroup when its current one
  // ends instead of waiting for the slowest image of the launch (YFV2_TPAIR=0: four launches).  Needs the chained output convs
  // on both towers (anchors + classes <= 96) and a second intermediate buffer (tb: unused on this path otherwise).
  bool pair_level(int H, int W) const {
    if (sw.plan.towers_unpaired || sw.plan.layer_by_layer) return false;
    return yfv2_tower2_supported(H, W) && yfv2_towerh_supported(H, W) && !yfv2_towerh_multi(H, W) && cfg.anchor_num + cfg.classes <= 96;
  }

  // DWConvblock (fpn.py:12-25) + the output convs fed by this tower (detector.py:25-31)
  void tower_half(const std::string& name, int H, int W, const float* in, float* out, const Folded& fd, const Folded& fp,
                  const Folded* fh, int mh, int split, int head0, int head1) {
    TowerHalf t;
    t.name = name;
    t.args.in = in; t.args.out = out;
    t.args.H = H; t.args.W = W;
    t.args.mh = mh; t.args.split = split;
    t.img = wp.image_tower(fd, fp, fh, mh);
    // one LDS layout per launch: where the four halves of a map size share a launch (merge_tower_launches) every image is
    // packed for the widest output conv of the level (obj + cls), else for the step's own
    // (with more than 93 classes the class head runs as separate launches: the level's halves are never merged)
    const bool merged_level = yfv2_towerh_multi(H, W) && cfg.anchor_num + cfg.classes <= 96;
    t.tiles = merged_level ?((cfg.anchor_num + cfg.classes + 15) / 16 <= 1 ? 1 : 6) : (fh ? ((mh + 15) / 16 <= 1 ? 1 : 6) : 0);
    // paired level (pair_level): the two b halves share a launch, so both are packed for the wider of the two output convs
    if (pair_level(H, W) && fh) t.tiles = ((cfg.anchor_num + cfg.classes + 15) / 16 <= 1 && (4 * cfg.anchor_num + 15) / 16 <= 1) ? 1 : 6;
    if (yfv2_towerh_supported(H, W)) t.img16 = wp.image_towerh(fd, fp, fh, mh, t.tiles);
    t.has_head = fh != nullptr;
    t.head0 = head0; t.head1 = head1;
    Step s;
    s.name = name;
    s.flops = half_flops(t);
    s.bytes = half_bytes(t);
    TowerStep kd;
    kd.tiles = t.tiles;
    kd.halves.push_back(std::move(t));
    push(s, kd);
  }

  // obj + cls output convs of a model with more than 93 classes, from the finished cls tower in ws.tb: the objectness head
  // and the class head in slices of up to 96 output channels, each a PW_HEAD launch writing its channel range of the NCHW tensor
  void wide_cls_heads(const std::string& p, int px, int scale_idx) {
    const int A = cfg.anchor_num, nc = cfg.classes;
    Folded f;
    wp.heads({{"output_obj_layers", A}}, 72, &f);
    {
      Step& s = add_pw(p + " -> output_obj (bias, NCHW)", 72, PW_HEAD, A, px, ws.tb.p, 72, 0, nullptr, 0, 0, false, f);
      pw(s).args.split = A; pw(s).head0 = scale_idx * 3 + 1; pw(s).head1 = -1;
    }
    for (int c0 = 0; c0 < nc; c0 += 96) {
      const int n = std::min(96, nc - c0);
      wp.heads_range("output_cls_layers", c0, n, 72, &f);
      Step& s = add_pw(p + " -> output_cls channels " + std::to_string(c0) + ".." + std::to_string(c0 + n - 1) + " (bias, NCHW)", 72, PW_HEAD, n, px,
                       ws.tb.p, 72, 0, nullptr, 0, 0, false, f);
      pw(s).args.split = n; pw(s).args.ctot0 = nc; pw(s).args.coff0 = c0; pw(s).head0 = scale_idx * 3 + 2; pw(s).head1 = -1;
    }
  }

  void tower(const std::string& p, int H, int W, const Buf& s_in, bool is_cls, int scale_idx) {
    Folded f;
    const int px = H * W;
    {
      if (!sw.plan.layer_by_layer && yfv2_tower2_supported(H, W)) {
        Folded fd1, fp1, fd2, fp2, fh;
        wp.dw(p + ".0", p + ".1", 72, 5, &fd1);
        wp.pw(p + ".3", p + ".4", 72, 72, &fp1);
        wp.dw(p + ".5", p + ".6", 72, 5, &fd2);
        wp.pw(p + ".8", p + ".9", 72, 72, &fp2);
        const int A = cfg.anchor_num, nc = cfg.classes;
        float* mid = (!is_cls && pair_level(H, W)) ? ws.tb.p : ws.ta.p;   // (paired level: both towers' a halves are alive at once)
        tower_half(p + " half a: dw5x5+bn+relu -> pw+bn", H, W, s_in.p, mid, fd1, fp1, nullptr, 0, 0, -1, -1);
        if (is_cls && A + nc > 96) {   // more output channels than a chained output conv holds: the tower ends in memory, the heads follow as launches
          tower_half(p + " half b: dw5x5+bn+relu -> pw+bn", H, W, mid, ws.tb.p, fd2, fp2, nullptr, 0, 0, -1, -1);
          wide_cls_heads(p, px, scale_idx);
        } else if (is_cls) {
          wp.heads({{"output_obj_layers", A}, {"output_cls_layers", nc}}, 72, &fh);
          tower_half(p + " half b: dw5x5+bn+relu -> pw+bn -> output_obj+output_cls (bias, NCHW)", H, W, mid, nullptr, fd2,
                     fp2, &fh, A + nc, A, scale_idx * 3 + 1, scale_idx * 3 + 2);
        } else {
          wp.heads({{"output_reg_layers", 4 * A}}, 72, &fh);
          tower_half(p + " half b: dw5x5+bn+relu -> pw+bn -> output_reg (bias, NCHW)", H, W, mid, nullptr, fd2, fp2, &fh,
                     4 * A, 4 * A, scale_idx * 3 + 0, -1);
        }
        return;
      }
    }
    wp.dw(p + ".0", p + ".1", 72, 5, &f);
    add_dw(p + ".dw5x5+bn+relu(a)", 5, 1, 72, H, W, s_in.p, 72, ws.ta.p, 72, true, f);
    wp.pw(p + ".3", p + ".4", 72, 72, &f);
    add_pw(p + ".pw+bn(a)", 72, PW_PLAIN, 72, px, ws.ta.p, 72, 0, ws.tb.p, 72, 0, false, f);
    wp.dw(p + ".5", p + ".6", 72, 5, &f);
    add_dw(p + ".dw5x5+bn+relu(b)", 5, 1, 72, H, W, ws.tb.p, 72, ws.ta.p, 72, true, f);
    wp.pw(p + ".8", p + ".9", 72, 72, &f);
    add_pw(p + ".pw+bn(b)", 72, PW_PLAIN, 72, px, ws.ta.p, 72, 0, ws.tb.p, 72, 0, false, f);
    const int A = cfg.anchor_num, nc = cfg.classes;
    if (is_cls && A + nc > 96) {
      wide_cls_heads(p, px, scale_idx);
    } else if (is_cls) {
      wp.heads({{"output_obj_layers", A}, {"output_cls_layers", nc}}, 72, &f);
      Step& s = add_pw(p + " -> output_obj+output_cls (bias, NCHW)", 72, PW_HEAD, A + nc, px, ws.tb.p, 72, 0, nullptr,
                       0, 0, false, f);
      pw(s).args.split = A;
      pw(s).head0 = scale_idx * 3 + 1;
      pw(s).head1 = scale_idx * 3 + 2;
    } else {
      wp.heads({{"output_reg_layers", 4 * A}}, 72, &f);
      Step& s = add_pw(p + " -> output_reg (bias, NCHW)", 72, PW_HEAD, 4 * A, px, ws.tb.p, 72, 0, nullptr, 0, 0, false, f);
      pw(s).args.split = 4 * A;
      pw(s).head0 = scale_idx * 3 + 0;
      pw(s).head1 = -1;
    }
  }

  // towerh_kernel's single-pixel form (maps up to 11x11) runs the four tower halves of a map size in ONE launch (each
  // workgroup: cls a, cls b, reg a, reg b of its image, in the order the separate launches had): runs of four consecutive
  // such steps become one step.
  void merge_tower_launches() {
    std::vector<Step> out;
    for (size_t i = 0; i < plan.steps.size();) {
      const TowerHalf* first = lone_half(plan.steps[i]);
      auto mergeable = [&](const Step& s) {
        const TowerHalf* t = lone_half(s);
        return first && t && t->img16 != 0 && yfv2_towerh_multi(t->args.H, t->args.W) && t->args.H == first->args.H && t->args.W == first->args.W &&
               cfg.anchor_num + cfg.classes <= 96;
      };
      size_t n = 0;
      while (i + n < plan.steps.size() && n < 4 && mergeable(plan.steps[i + n])) ++n;
      const bool pair = n < 4 && first && i + 4 <= plan.steps.size() && pair_level(first->args.H, first->args.W) && pairable(i);
      if (!pair && n < 4) {
        out.push_back(plan.steps[i]);
        ++i;
        continue;
      }
      const TowerHalf *ca = lone_half(plan.steps[i]), *cb = lone_half(plan.steps[i + 1]), *ra = lone_half(plan.steps[i + 2]), *rb = lone_half(plan.steps[i + 3]);
      if (n == 4) {
        // half a reads the FPN map, half b writes logits; the 72-channel tensor between them is the launch's own scratch
        out.push_back(joined({ca, cb, ra, rb}, false, ca->tiles, ": cls_head (dw5+bn+relu -> pw+bn, twice) -> output_obj+output_cls | reg_head -> output_reg, four jobs in one launch", true));
      } else if (!((ca->args.H | ca->args.W) & 1)) {
        // cls a, cls b, reg a, reg b  ->  ONE step {cls a, reg a, cls b, reg b} (towerp_kernel: even maps).  At batches that fill the chip it is
        // one launch whose workgroups run their image's four halves back to back (yfv2_launch_towerh decides per call: small batches run
        // the a halves and the b halves as two launches of independent items); the tensors between the halves are the launch's own scratch
        out.push_back(joined({ca, ra, cb, rb}, true, std::max(cb->tiles, rb->tiles),
                             ": cls_head (dw5x5+bn+relu -> pw+bn, twice) -> output_obj+output_cls | reg_head -> output_reg, the four halves of an image in one workgroup", true));
      } else {
        // cls a, cls b, reg a, reg b  ->  (cls a | reg a), (cls b | reg b); every half reads and writes memory: external = bytes
        out.push_back(joined({ca, ra}, true, ca->tiles, ": cls_head half a | reg_head half a (dw5x5+bn+relu -> pw+bn), side by side in one launch", false));
        out.push_back(joined({cb, rb}, true, cb->tiles, ": cls_head half b -> output_obj+output_cls | reg_head half b -> output_reg, side by side in one launch", false));
      }
      i += 4;
    }
    for (Step& s : out)
      if (TowerStep* k = kind_of<TowerStep>(s); k && towerp_step(*k)) {
        towerp_lane_patches(k->halves[0].args.H, k->halves[0].args.W, k->lane_patch);
        k->has_lane_patch = true;
      }
    plan.steps.swap(out);
  }
  // one step from tower halves of one map size; own_scratch: what passes from an a half to its b half never leaves the launch
  static Step joined(std::initializer_list<const TowerHalf*> halves, bool par, int tiles, const std::string& what, bool own_scratch) {
    Step m;
    TowerStep kd;
    kd.par = par;
    kd.tiles = tiles;
    double ext = 0;
    for (const TowerHalf* t : halves) {
      m.flops += half_flops(*t); m.bytes += half_bytes(*t);
      ext += 4.0 * t->args.H * t->args.W * (t->has_head ? (double)t->args.mh : 72.0);
      kd.halves.push_back(*t);
    }
    m.name = "fpn towers " + std::to_string(kd.halves[0].args.H) + "x" + std::to_string(kd.halves[0].args.W) + what;
    if (own_scratch) m.bytes_ext = ext;
    m.kind = std::move(kd);
    return m;
  }
  // four consecutive tower steps of one level in the order tower() emits them, all on towerh_kernel with the same image layout per pair
  bool pairable(size_t i) const {
    const TowerHalf *ca = lone_half(plan.steps[i]), *cb = lone_half(plan.steps[i + 1]), *ra = lone_half(plan.steps[i + 2]), *rb = lone_half(plan.steps[i + 3]);
    for (const TowerHalf* t : {ca, cb, ra, rb})
      if (!t || !t->img16 || t->args.H != ca->args.H || t->args.W != ca->args.W) return false;
    return !ca->has_head && !ra->has_head && cb->has_head && rb->has_head && ca->tiles == ra->tiles && cb->tiles == rb->tiles &&
           cb->args.in == ca->args.out && rb->args.in == ra->args.out && ca->args.out != ra->args.out;
  }

  void build() {
    const int H = cfg.height, W = cfg.width;
    int hh = H / 4, ww = W / 4, cin = 24;
    const long long pp_bufstride = 48LL * (H / 8) * (W / 8);   // floats from an image's copy in buffer 0 to its copy in buffer 1 (the image stride is twice that)
    const bool fused = !sw.plan.layer_by_layer;   // yfv2_plan.layer_by_layer: every layer its own launch (the general plan)
    const bool stage2_px = fused && ws.s2pp.p && yfv2_s1px_supported(hh / 2, ww / 2) &&
                           yfv2_block_s2_rows(48, hh / 2, ww / 2) > 0;
    // the stem's output for s2h_kernel: [H/4][W/4][24] (a pixel's 96 bytes in one run: every lane group's 16-byte store lands in
    // the same 1.5 KB of a wave's row) - 126 -> 120 us against the quad planes of round 4's first half on the same box, stage2.0
    // unchanged (72.7 us either way).  The fp32-matrix plan keeps its pair planes.
    const bool stem_nhwc = stage2_px && sw.bf6;
    add_stem(ws.a1, stage2_px && !stem_nhwc);
    plan.stem_pp = stage2_px && !stem_nhwc;
    plan.front_fused = stem_nhwc && sw.front_wanted;   // YFV2_FRONT=0: the stem and stage2.0 as two launches (the form every other plan and the uint8 entry points use)
    const Buf* stage_bufs[3] = {ws.s2, ws.s3, ws.s4};
    const int repeats[3] = {4, 8, 4};
    const Buf* x = &ws.a1;
    const Buf* c2 = nullptr;   // stage 3's output
    plan.dbg[0] = {ws.a1.p, ws.a1.per_img, 24};
    Stage2Layout L2{};
    bool px_pending = false;   // the next stride-2 block reads stage 2's pair planes
    for (int si = 0; si < 3; ++si) {
      const int cout = cin * 2;
      int cur = 0;
      const bool use_px = si == 0 && stage2_px;
      for (int i = 0; i < repeats[si]; ++i) {
        const std::string p = "backbone.stage" + std::to_string(si + 2) + "." + std::to_string(i);
        const Buf* y = &stage_bufs[si][cur];
        if (i == 0) {
          if (use_px) s2px_block(p, hh, ww);
          else if (px_pending) block_s2(p, cin, hh, ww, ws.s2pp, *y, L2.label, L2.buf, pp_bufstride);
          else if (si == 2 && plan.c2_permuted) block_s2(p, cin, hh, ww, *x, *y, nullptr, nullptr, 0, plan.c2_label);
          else block_s2(p, cin, hh, ww, *x, *y);
          px_pending = false;
          hh /= 2; ww /= 2;
          if (use_px) {   // logical channel c sits at slot(c) of buffer 0
            for (int k = 0; k < 48; ++k) L2.label[k] = yfv2_stage2_channel(k);
            for (int q = 0; q < 24; ++q) L2.buf[q] = 0;
          }
        } else if (use_px) {
          s1px_block(p, hh, ww, L2, pp_bufstride);
        } else if (fused && sw.bf6 && i == 1 && repeats[si] == 8 && yfv2_s1chain_supported(cout / 2, hh, ww)) {
          std::vector<std::string> names;
          for (int q = 1; q < repeats[si]; ++q) names.push_back("backbone.stage" + std::to_string(si + 2) + "." + std::to_string(q));
          s1chain_block(names, cout, hh, ww, *x, *y, plan.c2_label);     // blocks 1..7 of the stage as one launch
          plan.c2_permuted = ok;
          i = repeats[si] - 1;
        } else if (fused && i == 1 && si == 2 && yfv2_s1pool_supported(cout / 2, hh, ww)) {
          std::vector<std::string> names;
          for (int q = 1; q < repeats[si]; ++q) names.push_back("backbone.stage" + std::to_string(si + 2) + "." + std::to_string(q));
          s1pool_block(names, cout, hh, ww, *x, *y);                     // stage 4's blocks 1..3 as one launch
          i = repeats[si] - 1;
        } else {
          block_s1(p, cout, hh, ww, *x, *y);
        }
        x = y;
        cur ^= 1;
      }
      if (use_px) {
        px_pending = true;
        plan.s2_px = true;
        for (int k = 0; k < 48; ++k) plan.s2_label[k] = L2.label[k];
        for (int q = 0; q < 24; ++q) plan.s2_buf[q] = L2.buf[q];
        plan.dbg[1] = {ws.s2pp.p, (size_t)48 * hh * ww, cout};
      } else {
        plan.dbg[1 + si] = {x->p, x->per_img, cout};
      }
      if (si == 1) c2 = x;
      cin = cout;
    }
    const Buf* c3 = x;
    const int h3 = H / 32, w3 = W / 32, h2 = H / 16, w2 = W / 16;
    Folded f;
    wp.pw("fpn.conv1x1_3.0", "fpn.conv1x1_3.1", 72, 192, &f);
    add_pw("fpn.conv1x1_3 pw192->72+bn+relu", 192, PW_PLAIN, 72, h3 * w3, c3->p, 192, 0, ws.f3.p, 72, 0, true, f);
    wp.pw("fpn.conv1x1_2.0", "fpn.conv1x1_2.1", 72, 288, &f);
    if (plan.c2_permuted && ok) {   // columns 192.. read C2 in the chain kernel's channel order
      int lab[288];
      for (int k = 0; k < 192; ++k) lab[k] = k;
      for (int k = 0; k < 96; ++k) lab[192 + k] = 192 + plan.c2_label[k];
      f = wp.permuted_pw_inputs(f, 72, 288, lab);
    }
    // Default plan (round 6): a 1x1 conv commutes with the nearest-neighbour upsample (fpn.py:57-59), so conv1x1_2's 192 upsampled channels
    // are applied ONCE per coarse pixel - Q = scale2 (W2[:, :192] C3) + shift2, by the launch that computes conv1x1_3 from the same C3 - and
    // the fine-map launch is a K = 96 conv over C2 whose epilogue adds Q at (y / 2, x / 2): a third of the matrix-core work and 25 MB less
    // traffic than the K = 288 form (which the fp32-matrix and the layer-by-layer plans keep).  Like the BatchNorm folding a
    // re-association inside one linear map: S2 = relu(scale2 (W2b C2) + Q) instead of relu(scale2 (W2a up(C3) + W2b C2) + shift2).
    const bool fpn_split = fused && sw.bf6 && ok && ws.fq.p && yfv2_pw_presplit_supported(192, PW_DUAL, 72) && yfv2_pw_presplit_supported(96, PW_FPNQ, 72);
    if (fpn_split) {
      Step& s3 = plan.steps.back();                                     // conv1x1_3 just added: it becomes the dual launch
      Folded fa = wp.pw_columns(f, 72, 288, 0, 192), fb = wp.pw_columns(f, 72, 288, 192, 96);
      Folded f3;
      wp.pw("fpn.conv1x1_3.0", "fpn.conv1x1_3.1", 72, 192, &f3);
      pw(s3).mode = PW_DUAL;
      pw(s3).args.copy = ws.fq.p; pw(s3).args.copy_stride = 72; pw(s3).args.copy_off = 0;
      pw(s3).args.presplit = 1;
      pw(s3).img = wp.image_pw_dual(f3, fa, 72, 192, 5);
      s3.name = "fpn.conv1x1_3 pw192->72+bn+relu | the C3 part of fpn.conv1x1_2 (W2[:, :192] C3, scale + shift of its bn), one launch";
      Step& s = add_pw("fpn.conv1x1_2 pw96 over C2 + the C3 part at (y/2, x/2) +bn+relu  [= up2x(C3)+cat(C2)+pw288->72+bn+relu]", 96, PW_FPNQ, 72, h2 * w2,
                       c2->p, 96, 0, ws.f2.p, 72, 0, true, fb);
      pw(s).args.in2 = ws.fq.p;
      pw(s).args.H = h2; pw(s).args.W = w2;
      s.flops = 2.0 * h2 * w2 * 288 * 72;                             // (the reference layer's count, as for every fused or re-associated launch)
      s.bytes = 4.0 * (h3 * w3 * 192.0 + h2 * w2 * 96.0 + h2 * w2 * 72.0);
    } else {
      Step& s = add_pw("fpn.conv1x1_2 up2x(C3)+cat(C2)+pw288->72+bn+relu", 288, PW_FPN, 72, h2 * w2, c3->p, 192, 0,
                       ws.f2.p, 72, 0, true, f);
      pw(s).args.in2 = c2->p;
      pw(s).args.H = h2; pw(s).args.W = w2;
      s.bytes = 4.0 * (h3 * w3 * 192.0 + h2 * w2 * 96.0 + h2 * w2 * 72.0);
    }
    plan.dbg[4] = {ws.f2.p, ws.f2.per_img, 72};
    plan.dbg[5] = {ws.f3.p, ws.f3.per_img, 72};
    tower("fpn.cls_head_3.block", h3, w3, ws.f3, true, 1);
    tower("fpn.reg_head_3.block", h3, w3, ws.f3, false, 1);
    tower("fpn.cls_head_2.block", h2, w2, ws.f2, true, 0);
    tower("fpn.reg_head_2.block", h2, w2, ws.f2, false, 0);
    merge_tower_launches();   // (also the pass that gives every towerp_kernel step its lane table: no TowerStep is created after it)
    const StemStep* stem = plan.steps.empty() ? nullptr : kind_of<StemStep>(plan.steps[0]);
    S2PxStep* s20 = plan.steps.size() > 1 ? kind_of<S2PxStep>(plan.steps[1]) : nullptr;
    if (plan.front_fused && ok && stem && s20 && s20->img16) {
      s20->front = true;
      s20->H = H; s20->W = W;
      s20->img_stem16 = stem->img16;
      plan.stem_aside = plan.steps[0];
      plan.steps.erase(plan.steps.begin());   // (stem and s20 end here)
      Step& f = plan.steps[0];
      std::get<S2PxStep>(f.kind).name_plain = f.name;
      f.name = "stem + backbone.stage2.0 in one launch: conv3x3s2+bn+relu+maxpool3x3s2 -> s2 block, lane-per-pixel (proj | main) -> pair planes";
      f.flops += plan.stem_aside.flops;
      f.bytes += plan.stem_aside.bytes;                     // per-layer accounting: both layers' reads and writes
      f.bytes_ext = 4.0 * (3.0 * H * W + 48.0 * (H / 8) * (W / 8));   // the image in, stage 2's 48 channels out
    } else {
      plan.front_fused = false;
    }
  }
};

// ---- the runner: one launch overload per kind.  Each completes a copy of the kind's argument prototype from the call and launches it;
// the return value is null, or what kind of kernel is missing for these shapes ("no <what> kernel for step '<name>'")
const char* launch(const StemStep& st, const RunCtx& c) {
  yfv2_launch_stem(stem_launch_args(st, c), c.stream);
  return nullptr;
}

const char* launch(const PwStep& st, const RunCtx& c) {
  PwArgs a = st.args;
  a.P = c.B * st.px_per_img;
  a.img = c.params + st.img;
  a.bf6 = c.bf6 ? 1 : 0;
  a.nonfinite = c.nonfinite;
  if (st.mode == PW_HEAD) {
    a.nchw0 = c.out6[st.head0];
    a.nchw1 = st.head1 >= 0 ? c.out6[st.head1] : nullptr;
  }
  return yfv2_launch_pw(st.K, st.mode, a, c.stream) ? nullptr : "pointwise";
}

const char* launch(const DwStep& st, const RunCtx& c) {
  DwArgs a = st.args;
  a.B = c.B;
  a.w = c.params + st.w; a.scale = c.params + st.scale; a.shift = c.params + st.shift;
  return yfv2_launch_dw(st.ksize, st.stride, a, c.stream) ? nullptr : "depthwise";
}

const char* launch(const S2Step& st, const RunCtx& c) {
  BlockS2Args a = st.args;
  a.B = c.B;
  a.img = c.params + st.img;
  a.bf6 = c.bf6 ? 1 : 0;
  a.trace = c.trace;
  a.img16 = (st.img16 && c.bf6) ? c.params + st.img16 : nullptr;
  a.nonfinite = c.nonfinite;
  if (a.img16 && st.cin == 48) yfv2_launch_s3h(a, c.stream);
  else if (a.img16 && st.cin == 96) yfv2_launch_s4h(a, c.stream);
  else if (!yfv2_launch_block_s2(st.cin, a, c.stream)) return "fused stride-2";
  return nullptr;
}

const char* launch(const S2PxStep& st, const RunCtx& c) {
  S2PxArgs a = st.args;
  a.B = c.B;
  a.img[0] = c.params + st.img_proj;
  a.img[1] = c.params + st.img_main;
  a.img16 = c.bf6 ? c.params + st.img16 : nullptr;   // fp32_matrix: the two role kernels on the 4x4x1 fp32 MFMA
  a.nonfinite = c.nonfinite;
  if (st.front) {
    FrontArgs f{};
    f.x = c.x; f.H = st.H; f.W = st.W; f.u8_in = c.x_u8 ? 1 : 0;
    f.img_stem = c.params + st.img_stem16;
    f.s2 = a;
    yfv2_launch_front(f, c.stream);
  } else {
    yfv2_launch_s2px(a, c.stream);
  }
  return nullptr;
}

const char* launch(const S1PxStep& st, const RunCtx& c) {
  S1PxArgs a = st.args;
  a.B = c.B;
  a.img = c.params + st.img;
  a.img16 = c.bf6 ? c.params + st.img16 : nullptr;   // fp32_matrix: s1px_kernel on the 4x4x1 fp32 MFMA
  a.nonfinite = c.nonfinite;
  yfv2_launch_s1px(a, c.stream);
  return nullptr;
}

const char* launch(const S1Step& st, const RunCtx& c) {
  BlockS1Args a = st.args;
  a.B = c.B;
  a.img = c.params + st.img;
  a.trace = (st.pool || c.trace) ? c.trace : c.trace_unnamed;   // the stage-3 chain stamps under an unnamed trace too
  a.nonfinite = c.nonfinite;
  if (st.pool) return yfv2_launch_block_s1pool(a, c.stream) ? nullptr : "pool-chain";
  return yfv2_launch_block_s1chain(a, c.stream) ? nullptr : "chain";
}

TowerArgs half_args(const TowerHalf& t, const RunCtx& c) {
  TowerArgs a = t.args;
  a.B = c.B;
  a.img = c.params + t.img;
  a.has_head = t.has_head ? 1 : 0;
  a.nchw0 = nullptr; a.nchw1 = nullptr;
  a.trace = c.trace;
  a.bf6 = c.bf6 ? 1 : 0;
  a.img16 = (t.img16 && c.bf6) ? c.params + t.img16 : nullptr;   // fp32_matrix: tower2_kernel on the fp32 MFMA
  a.nonfinite = c.nonfinite;
  if (t.has_head) {
    a.nchw0 = c.out6[t.head0];
    a.nchw1 = t.head1 >= 0 ? c.out6[t.head1] : nullptr;
  }
  return a;
}

const char* launch(const TowerStep& st, const RunCtx& c) {
  if (st.halves[0].img16 && c.bf6) {
    TowerJobs jobs{};
    jobs.n = (int)st.halves.size();
    for (int k = 0; k < jobs.n; ++k) jobs.j[k] = half_args(st.halves[k], c);
    if (towerp_step(st) && !st.has_lane_patch) return "tower lane table";
    std::copy(st.lane_patch, st.lane_patch + 128, jobs.lane_patch);
    // half a -> half b of a tower inside one launch: the tensor between them stays in the workgroup's LDS - as long as every
    // workgroup has ONE image (the job loop is outside the image loop: a second image's half a would overwrite the first's before
    // its half b has read it).  That is: as long as the launch's grid, which launch_towers takes from the same function, is B
    jobs.par = st.par ? 1 : 0;
    const Yfv2Device dev = yfv2_device();   // (the step's one look at the device: the launchers below take it from here)
    const bool one_image = yfv2_image_grid(c.B, dev) == c.B;
    for (int k = 0; k + 1 < jobs.n && !st.par; ++k)
      if (one_image && !jobs.j[k].has_head && jobs.j[k].out == jobs.j[k + 1].in) { jobs.j[k].chain |= 2; jobs.j[k + 1].chain |= 1; }
    if (yfv2_launch_towerh(jobs, st.tiles, dev, c.stream)) return nullptr;
  }
  for (const TowerHalf& t : st.halves)   // tower2_kernel, one launch per half
    if (!yfv2_launch_tower2(half_args(t, c), c.stream)) return "tower";
  return nullptr;
}

}  // namespace

bool plan_build(const yfv2_config& cfg, const PlanSwitches& sw, const Workspace& ws, WeightPacker& wp, Plan* out) {
  PlanBuilder pb{cfg, sw, ws, wp};
  pb.build();
  if (!pb.ok) return false;
  *out = std::move(pb.plan);
  return true;
}

std::string step_kernel(const Step& st) {
  struct {
    std::string operator()(const StemStep&) const { return "stem_h3_kernel"; }   // fp32 input, default plan (uint8 input: stem_h3u_kernel; fp32_matrix: stem_px_kernel)
    std::string operator()(const PwStep& k) const { return "pw_kernel<" + std::to_string(k.K) + ","; }
    std::string operator()(const DwStep& k) const { return "dw_kernel<" + std::to_string(k.ksize) + ", " + std::to_string(k.stride) + ">"; }
    std::string operator()(const S2Step& k) const {
      return k.img16 ? std::string(k.cin == 96 ? "s4h_kernel" : "s3h2_kernel") : (k.cin == 96 ? std::string("block_s2w_kernel<") : "block_s2_kernel<" + std::to_string(k.cin) + ",");
    }
    // default plan (fp32_matrix: s2px_proj_kernel + s2px_main_kernel)
    std::string operator()(const S2PxStep& k) const { return k.front ? "front2_kernel" : "s2h_kernel"; }
    std::string operator()(const S1PxStep&) const { return "s1h_kernel"; }   // default plan (fp32_matrix: s1px_kernel)
    std::string operator()(const S1Step& k) const { return k.pool ? "block_s1pool_kernel" : "block_s1chain6_kernel"; }
    std::string operator()(const TowerStep& k) const {
      const TowerHalf& t = k.halves[0];
      const int H = t.args.H, W = t.args.W;
      if (t.img16 && k.halves.size() > 1 && !k.par) return "towers_kernel<" + std::to_string(k.tiles) + ">";   // default plan, maps up to 11x11
      if (towerp_step(k))   // default plan, even maps up to 22x22
        return "towerp_kernel<" + std::to_string(k.tiles) + (k.par && k.halves.size() == 4 ? ", true>" : ", false>");
      if (t.img16) return "towerh_kernel<" + std::to_string(k.tiles) + ", " + (H > 11 || W > 11 ? "2, 4>" : "1, 1>");
      return "tower2_kernel<" + std::to_string(!t.has_head ? 0 : ((t.args.mh + 15) / 16 <= 1 ? 1 : 6)) + ", 512, " + (H * W > 128 ? "4, 4," : "1, 1,");
    }
  } name;
  return std::visit(name, st.kind);
}

size_t step_image(const Step& st) {
  struct {
    size_t operator()(const StemStep& k) const { return k.img; }
    size_t operator()(const PwStep& k) const { return k.img; }
    size_t operator()(const DwStep&) const { return 0; }
    size_t operator()(const S2Step& k) const { return k.img; }
    size_t operator()(const S2PxStep& k) const { return k.img_proj; }
    size_t operator()(const S1PxStep& k) const { return k.img; }
    size_t operator()(const S1Step& k) const { return k.img; }
    // (the cls tower's b half where an image's four halves share a workgroup: the half that step has always answered with)
    size_t operator()(const TowerStep& k) const { return k.halves[k.par && k.halves.size() == 4 ? 2 : 0].img; }
  } image;
  return std::visit(image, st.kind);
}

StemArgs stem_launch_args(const StemStep& st, const RunCtx& c) {
  StemArgs a = st.args;
  a.x = c.x; a.B = c.B; a.u8_in = c.x_u8 ? 1 : 0;
  a.img = c.params + st.img;
  a.img_u8 = c.params + st.img_u8;
  a.img16 = c.bf6 ? c.params + st.img16 : nullptr;   // fp32_matrix: the 4x4x1 fp32-MFMA stem
  a.nonfinite = c.nonfinite;
  return a;
}

int plan_run(const Plan& plan, const RunCtx& call, long long* trace, int trace_step, hipEvent_t* ev, int only_step, std::string* err) {
  // the front kernels read the image with 16-byte (fp32) / 12-byte-at-4-byte-alignment (uint8) buffer loads: a base address that
  // is not so aligned would be read at the wrong offsets without any fault (include/yfv2.h yfv2_forward)
  if (reinterpret_cast<uintptr_t>(call.x) & (call.x_u8 ? 3u : 15u)) {
    *err = call.x_u8 ? "input images: the uint8 tensor must be 4-byte aligned" : "input images: the fp32 tensor must be 16-byte aligned";
    return YFV2_ERR_ARG;
  }
  struct ProbeScope { ~ProbeScope() { yfv2_launch_probe = Yfv2LaunchProbe{}; } } probe_scope;   // (cleared on every path out, error returns included)
  RunCtx c = call;
  c.trace_unnamed = trace_step < 0 ? trace : nullptr;
  for (size_t i = 0; i < plan.steps.size(); ++i) {
    if (only_step >= 0 && (int)i != only_step) continue;
    const Step& st = plan.steps[i];
    yfv2_launch_probe = ev ? Yfv2LaunchProbe{ev[2 * i], ev[2 * i + 1], 0} : Yfv2LaunchProbe{};   // (profile pass: the step's launches stamp themselves)
    c.trace = trace_step == (int)i ? trace : nullptr;
    if (const char* what = std::visit([&](const auto& k) { return launch(k, c); }, st.kind)) {
      *err = std::string("no ") + what + " kernel for step '" + st.name + "'";
      return YFV2_ERR_CONFIG;
    }
    yfv2_launch_probe = Yfv2LaunchProbe{};
  }
  return YFV2_OK;
}
