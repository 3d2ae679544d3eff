// yfv2_train.hip - SURVEY.md 8(f) row 3, the rest of the training path: one iteration of train.py:96-123 on the device.
//   yfv2_train_forward   Detector.forward in train() mode (model/backbone/shufflenetv2.py:19-63,74-80,102-109, model/fpn.py,
//                        model/detector.py:21-47 with every nn.BatchNorm2d on BATCH statistics, running statistics moved by
//                        momentum 0.1 with the unbiased variance)
//   yfv2_train_backward  what total_loss.backward() (train.py:110) derives for the 225 parameters from the gradient of the
//                        loss w.r.t. the six logit maps (yfv2_loss)
//   yfv2_sgd_step        torch.optim.SGD(momentum, weight_decay, dampening 0, no Nesterov) as train.py:81-85 builds it
// Behaviour only was read from the reference; autograd's derivatives are restated from the layer definitions.
//
// This is the correctness-first slice of the row: plain NCHW fp32 kernels, one thread per output element (reductions: one
// block per channel / filter entry, float64 accumulators).  Instead of an autograd engine, the host half below the kernels walks
// the topology once per batch size and binding (Train::record) into a list of Op records, which yfv2_train_forward runs in order
// and yfv2_train_backward in reverse, and from which the arenas and both scratch blocks are sized.  It is NOT the
// throughput path (BASELINE.json's metric is inference); it exists so that the reference's training loop runs end to end
// on the MI355X through this library and matches tests/golden/golden_train.npz (the reference's own modules on CPU):
// gradients to 1e-5 of each tensor's largest entry, updated weights to 1e-6.  Parameters, gradients and BatchNorm buffers are
// the CALLER's device tensors in the reference's own layouts ((co, ci, k, k), (c,)): nothing is copied or re-laid-out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/yfv2.h"
#include "yfv2_ctx.h"    // DeviceGuard, DeviceBlock (and yfv2_pack.h: expected_numels)
#include "yfv2_device.h"

namespace {

// a (B, C, H, W) window into an NCHW tensor with Ctot channels: channel c of the view = channel coff + c * cstride of the tensor
struct V {
  float* p; int Ctot, coff, cstride, C, H, W;
  __host__ __device__ size_t at(int b, int c, int y, int x) const { return (((size_t)b * Ctot + coff + (size_t)c * cstride) * H + y) * W + x; }
};

struct ConvP { V in, out; const float* w; const float* bias; int k, stride, pad, dw, B; };


// Depthwise convs (3 x 3 and 5 x 5, stride 1 or 2; pad K / 2), forward and data gradient: a block stays inside ONE (image, channel)
// plane - the filter and the plane bases are wave-uniform, a thread divides once - with the generic kernels' summation order
// (row, then column; padded taps skipped), so the results are theirs bit for bit.  grid (position chunks of 256, B * C planes)
template <int K, int S>
__global__ __launch_bounds__(256) void dw_fwd_kernel(ConvP a) {
  constexpr int P = K / 2;
  const int OH = a.out.H, OW = a.out.W, IH = a.in.H, IW = a.in.W, C = a.out.C;
  const int pl = blockIdx.y, b = pl / C, c = pl - b * C;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= OH * OW) return;
  const int oy = o / OW, ox = o - oy * OW;
  const float* ip = a.in.p + a.in.at(b, c, 0, 0);
  const float* w = a.w + c * K * K;
  float acc = 0.f;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const int iy = oy * S - P + ky;
    if (iy < 0 || iy >= IH) continue;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = ox * S - P + kx;
      if (ix >= 0 && ix < IW) acc = __builtin_fmaf(w[ky * K + kx], ip[iy * IW + ix], acc);
    }
  }
  a.out.p[a.out.at(b, c, 0, 0) + o] = acc;
}
template <int K, int S>
__global__ __launch_bounds__(256) void dw_bwd_data_kernel(ConvP a) {   // a.in = gradient view of the input (accumulated into), a.out = gradient of the output
  constexpr int P = K / 2;
  const int OH = a.out.H, OW = a.out.W, IH = a.in.H, IW = a.in.W, C = a.in.C;
  const int pl = blockIdx.y, b = pl / C, c = pl - b * C;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= IH * IW) return;
  const int iy = i / IW, ix = i - iy * IW;
  const float* gp = a.out.p + a.out.at(b, c, 0, 0);
  const float* w = a.w + c * K * K;
  float acc = 0.f;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const int ny = iy + P - ky;
    if (ny < 0 || (S > 1 && (ny % S))) continue;
    const int oy = ny / S;
    if (oy >= OH) continue;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int nx = ix + P - kx;
      if (nx < 0 || (S > 1 && (nx % S))) continue;
      const int ox = nx / S;
      if (ox >= OW) continue;
      acc = __builtin_fmaf(w[ky * K + kx], gp[oy * OW + ox], acc);
    }
  }
  a.in.p[a.in.at(b, c, 0, 0) + i] += acc;
}
// The stem conv (3 x 3, stride 2, pad 1, 3 -> 24 channels): conv_fwd_kernel read its 27 inputs once per OUTPUT CHANNEL (0.96 ms at
// batch 64); here a thread owns an output pixel, reads them once and keeps the 24 sums in registers - the same fmaf chain per
// channel (input channel, then row, then column; padded taps skipped), the filter through the scalar cache.
__global__ __launch_bounds__(256) void stem_fwd_kernel(ConvP a) {
  const int OH = a.out.H, OW = a.out.W, IH = a.in.H, IW = a.in.W;
  const size_t n = (size_t)a.B * OH * OW, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ox = i % OW, oy = (i / OW) % OH, b = i / ((size_t)OW * OH);
  float acc[24];
#pragma unroll
  for (int co = 0; co < 24; ++co) acc[co] = 0.f;
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * 2 - 1 + ky;
      if (iy < 0 || iy >= IH) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 - 1 + kx;
        if (ix < 0 || ix >= IW) continue;
        const float v = a.in.p[a.in.at(b, ci, iy, ix)];
#pragma unroll
        for (int co = 0; co < 24; ++co) acc[co] = __builtin_fmaf(a.w[((co * 3 + ci) * 3 + ky) * 3 + kx], v, acc[co]);
      }
    }
#pragma unroll
  for (int co = 0; co < 24; ++co) a.out.p[a.out.at(b, co, oy, ox)] = acc[co];
}


// segments for a reduction of n elements next to `others` independent blocks: about 2048 blocks in all, at least 2048 elements each
inline unsigned reduce_segments(size_t n, size_t others) {
  size_t s = others >= 2048 ? 1 : 2048 / (others ? others : 1);
  if (s > 64) s = 64;
  if (s > n / 2048) s = n / 2048;
  return (unsigned)(s < 1 ? 1 : s);
}

__global__ __launch_bounds__(256) void bias_bwd_kernel(V g, int B, float* db) {
  __shared__ double red[256];
  const int co = blockIdx.x, n = B * g.H * g.W;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += (double)g.p[g.at(i / (g.H * g.W), co, (i / g.W) % g.H, i % g.W)];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
  if (threadIdx.x == 0) db[co] += (float)red[0];
}

// BatchNorm2d, training mode: per-channel batch mean / biased variance of y (B, C, H, W contiguous); saves mean and
// 1/sqrt(var + eps); running = 0.9 running + 0.1 (mean | unbiased variance)
// (All four kernels walk (plane, position) incrementally - no division per element - and the two elementwise ones take 1024
// elements per block; round 3's forms divided four times per element and spent a launch per layer on the per-channel finish.)
// per channel and segment: sum and sum of squares of y in double, into acc[4 c + 0, 1] (zeroed per forward)
__global__ __launch_bounds__(256) void bn_stats_part_kernel(const float* y, int B, int C, int HW, double* acc) {
  __shared__ double r0[256], r1[256];
  const int c = blockIdx.x, n = B * HW, nseg = gridDim.y, len = (n + nseg - 1) / nseg;
  const int i0 = blockIdx.y * len, i1 = i0 + len < n ? i0 + len : n;
  double a0 = 0.0, a1 = 0.0;
  int i = i0 + threadIdx.x;
  if (i < i1) {
    int b = i / HW, r = i - b * HW;
    const size_t pstride = (size_t)C * HW;
    const float* p = y + ((size_t)b * C + c) * HW;
    for (; i < i1; i += 256) {
      const double v = (double)p[r];
      a0 += v; a1 += v * v;
      r += 256;
      while (r >= HW) { r -= HW; p += pstride; }
    }
  }
  r0[threadIdx.x] = a0; r1[threadIdx.x] = a1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) { r0[threadIdx.x] += r0[threadIdx.x + s]; r1[threadIdx.x] += r1[threadIdx.x + s]; } __syncthreads(); }
  if (threadIdx.x == 0) { atomicAdd(&acc[4 * c + 0], r0[0]); atomicAdd(&acc[4 * c + 1], r1[0]); }
}
// mean, 1 / sqrt(biased variance + eps) (variance = E[y^2] - mean^2 in double: the inputs are fp32) and the running statistics are
// finished inside the apply kernel: a block of BN_EPB consecutive NCHW elements touches a few (image, channel) planes, its first
// threads finish those planes' statistics into LDS; the block that holds a channel's FIRST element (image 0) also stores
// mean / invstd for the backward pass and moves the running statistics - exactly once per channel and forward.
constexpr int BN_EPB = 1024, BN_CH = BN_EPB + 2;   // elements per block; planes a block can touch when H * W == 1 (+ slack)
struct BnWalk {     // (plane, position) of element i0 + tid + 256 j, advanced without divisions
  size_t pl; int k, c, b, r;
  __device__ BnWalk(size_t i, size_t ch0, int HW, int C) { pl = i / HW; r = (int)(i - pl * HW); k = (int)(pl - ch0); c = (int)(pl % C); b = (int)(pl / C); }
  __device__ void step(int HW, int C) { r += 256; while (r >= HW) { r -= HW; ++pl; ++k; if (++c == C) { c = 0; ++b; } } }
};
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* y, V z, int B, const double* acc, float* mean, float* invstd, float* run_mean, float* run_var,
                                                       const float* gamma, const float* beta, int relu) {
  __shared__ float s_mean[BN_CH], s_inv[BN_CH], s_gamma[BN_CH], s_beta[BN_CH];
  const int HW = z.H * z.W, C = z.C;
  const size_t n = (size_t)B * C * HW, i0 = (size_t)blockIdx.x * BN_EPB;
  const size_t ilast = i0 + BN_EPB - 1 < n ? i0 + BN_EPB - 1 : n - 1;
  const size_t ch0 = i0 / HW, nch = ilast / HW - ch0 + 1;               // (image, channel) planes this block touches
  const int nb = B * HW;
  for (size_t k = threadIdx.x; k < nch; k += 256) {
    const int c = (int)((ch0 + k) % C);
    const double m = acc[4 * c] / nb;
    double var = acc[4 * c + 1] / nb - m * m;
    if (var < 0.0) var = 0.0;
    const float fm = (float)m, fi = (float)(1.0 / sqrt(var + 1e-5));
    s_mean[k] = fm; s_inv[k] = fi; s_gamma[k] = gamma[c]; s_beta[k] = beta[c];
    if (ch0 + k < (size_t)C) {                                            // this plane belongs to image 0: the channel's one writer
      const size_t first = (ch0 + k) * HW;
      if (first >= i0 && first <= ilast) {
        mean[c] = fm; invstd[c] = fi;
        run_mean[c] = (float)(0.9 * (double)run_mean[c] + 0.1 * m);
        run_var[c] = (float)(0.9 * (double)run_var[c] + 0.1 * (nb > 1 ? var * nb / (nb - 1) : var));
      }
    }
  }
  __syncthreads();
  size_t i = i0 + threadIdx.x;
  if (i > ilast) return;
  BnWalk w(i, ch0, HW, C);
  for (; i <= ilast; i += 256) {
    float v = (y[i] - s_mean[w.k]) * s_inv[w.k] * s_gamma[w.k] + s_beta[w.k];
    if (relu && !(v > 0.f)) v = 0.f;
    z.p[z.at(w.b, w.c, 0, 0) + w.r] = v;
    w.step(HW, C);
  }
}

// per channel: sum of dz' and of dz' * xhat (dz' = dz where the ReLU let the value through); -> d beta, d gamma, and the two
// sums for bn_bwd_apply
__global__ __launch_bounds__(256) void bn_bwd_part_kernel(const float* y, V z, V dz, int B, const float* mean, const float* invstd, int relu, double* acc) {
  __shared__ double r0[256], r1[256];
  const int c = blockIdx.x, HW = z.H * z.W, n = B * HW, nseg = gridDim.y, len = (n + nseg - 1) / nseg;
  const int i0 = blockIdx.y * len, i1 = i0 + len < n ? i0 + len : n;
  double a0 = 0.0, a1 = 0.0;
  int i = i0 + threadIdx.x;
  if (i < i1) {
    int b = i / HW, r = i - b * HW;
    const float mc = mean[c], ic = invstd[c];
    for (; i < i1; i += 256) {
      float g = dz.p[dz.at(b, c, 0, 0) + r];
      if (relu && !(z.p[z.at(b, c, 0, 0) + r] > 0.f)) g = 0.f;
      const float xh = (y[((size_t)b * z.C + c) * HW + r] - mc) * ic;
      a0 += (double)g; a1 += (double)g * (double)xh;
      r += 256;
      while (r >= HW) { r -= HW; ++b; }
    }
  }
  r0[threadIdx.x] = a0; r1[threadIdx.x] = a1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) { r0[threadIdx.x] += r0[threadIdx.x + s]; r1[threadIdx.x] += r1[threadIdx.x + s]; } __syncthreads(); }
  if (threadIdx.x == 0) { atomicAdd(&acc[4 * c + 2], r0[0]); atomicAdd(&acc[4 * c + 3], r1[0]); }
}
// dy = gamma * invstd * (dz' - sum(dz') / N - xhat * sum(dz' xhat) / N)   (dy is the conv output's gradient: single consumer, overwritten)
// The two sums arrive in double (bn_bwd_part_kernel); a block converts those of the planes it touches (as bn_apply_kernel does
// with the statistics), and the block that holds a channel's first element adds them to d beta / d gamma - once per channel.
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* y, V z, V dz, float* dy, int B, const float* mean, const float* invstd, const float* gamma,
                                                          int relu, const double* acc, float* dgamma, float* dbeta) {
  __shared__ float s_mean[BN_CH], s_inv[BN_CH], s_gamma[BN_CH], s_s0[BN_CH], s_s1[BN_CH];
  const int HW = z.H * z.W, C = z.C;
  const size_t n = (size_t)B * C * HW, i0 = (size_t)blockIdx.x * BN_EPB;
  const size_t ilast = i0 + BN_EPB - 1 < n ? i0 + BN_EPB - 1 : n - 1;
  const size_t ch0 = i0 / HW, nch = ilast / HW - ch0 + 1;
  for (size_t k = threadIdx.x; k < nch; k += 256) {
    const int c = (int)((ch0 + k) % C);
    const float s0 = (float)acc[4 * c + 2], s1 = (float)acc[4 * c + 3];
    s_mean[k] = mean[c]; s_inv[k] = invstd[c]; s_gamma[k] = gamma[c]; s_s0[k] = s0; s_s1[k] = s1;
    if (ch0 + k < (size_t)C) {
      const size_t first = (ch0 + k) * HW;
      if (first >= i0 && first <= ilast) { dbeta[c] += s0; dgamma[c] += s1; }
    }
  }
  __syncthreads();
  size_t i = i0 + threadIdx.x;
  if (i > ilast) return;
  const float inv_n = 1.0f / (float)(B * HW);
  BnWalk w(i, ch0, HW, C);
  for (; i <= ilast; i += 256) {
    float g = dz.p[dz.at(w.b, w.c, 0, 0) + w.r];
    if (relu && !(z.p[z.at(w.b, w.c, 0, 0) + w.r] > 0.f)) g = 0.f;
    const float xh = (y[i] - s_mean[w.k]) * s_inv[w.k];
    dy[i] = s_gamma[w.k] * s_inv[w.k] * (g - s_s0[w.k] * inv_n - xh * s_s1[w.k] * inv_n);
    w.step(HW, C);
  }
}

// max_pool2d(3, 2, 1) as ATen's CPU kernel scans it: window rows then columns, a later value replaces the maximum only if it is
// greater - the FIRST maximum keeps the gradient
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* x, float* out, int* arg, int B, int C, int H, int W) {
  const int OH = H / 2, OW = W / 2;
  const size_t n = (size_t)B * C * OH * OW, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ox = i % OW, oy = (i / OW) % OH;
  const size_t plane = i / ((size_t)OW * OH);
  const float* xp = x + plane * H * W;
  float best = -INFINITY; int bi = -1;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * 2 - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * 2 - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const float v = xp[iy * W + ix];
      if (v > best || bi < 0) { best = v; bi = iy * W + ix; }
    }
  }
  out[i] = best; arg[i] = bi;
}
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* dout, const int* arg, float* dx, int B, int C, int H, int W) {
  const int OH = H / 2, OW = W / 2;
  const size_t n = (size_t)B * C * H * W, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ix = i % W, iy = (i / W) % H;
  const size_t plane = i / ((size_t)W * H);
  float acc = 0.f;
  for (int oy = iy / 2; oy <= (iy + 1) / 2 && oy < OH; ++oy)
    for (int ox = ix / 2; ox <= (ix + 1) / 2 && ox < OW; ++ox)
      if (arg[plane * OH * OW + oy * OW + ox] == iy * W + ix) acc += dout[plane * OH * OW + oy * OW + ox];
  dx[i] = acc;   // (the stem's ReLU output has this one consumer; the arena was zeroed)
}

// dst view (+)= src view, same (C, H, W)
__global__ __launch_bounds__(256) void view_copy_kernel(V dst, V src, int B, int accumulate) {
  const size_t n = (size_t)B * dst.C * dst.H * dst.W, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = i % dst.W, y = (i / dst.W) % dst.H, c = (i / ((size_t)dst.W * dst.H)) % dst.C, b = i / ((size_t)dst.W * dst.H * dst.C);
  const float v = src.p[src.at(b, c, y, x)];
  if (accumulate) dst.p[dst.at(b, c, y, x)] += v; else dst.p[dst.at(b, c, y, x)] = v;
}
// fpn.py:57-58: dst (2H x 2W) = nearest x2 of src; backward: d src += its four children
__global__ __launch_bounds__(256) void upsample2_kernel(V dst, V src, int B) {
  const size_t n = (size_t)B * dst.C * dst.H * dst.W, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = i % dst.W, y = (i / dst.W) % dst.H, c = (i / ((size_t)dst.W * dst.H)) % dst.C, b = i / ((size_t)dst.W * dst.H * dst.C);
  dst.p[dst.at(b, c, y, x)] = src.p[src.at(b, c, y >> 1, x >> 1)];
}
__global__ __launch_bounds__(256) void upsample2_bwd_kernel(V dsrc, V ddst, int B) {
  const size_t n = (size_t)B * dsrc.C * dsrc.H * dsrc.W, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = i % dsrc.W, y = (i / dsrc.W) % dsrc.H, c = (i / ((size_t)dsrc.W * dsrc.H)) % dsrc.C, b = i / ((size_t)dsrc.W * dsrc.H * dsrc.C);
  dsrc.p[dsrc.at(b, c, y, x)] += ddst.p[ddst.at(b, c, 2 * y, 2 * x)] + ddst.p[ddst.at(b, c, 2 * y, 2 * x + 1)] + ddst.p[ddst.at(b, c, 2 * y + 1, 2 * x)] +
                                 ddst.p[ddst.at(b, c, 2 * y + 1, 2 * x + 1)];
}



// ---- round 4: the pointwise (1x1, stride 1) convolutions - 51 of the 79 convs and 73 % of the step's arithmetic - as GEMMs on
// the fp32 matrix instruction (v_mfma_f32_16x16x4_f32), straight on the NCHW views (channel planes are contiguous pixel runs).
// Round 3 ran them on conv_fwd / conv_bwd_data / conv_bwd_weight_kernel above: one thread per output element looping over the
// channels, one BLOCK per filter entry for the weight gradient (every block re-read the whole activation and gradient: 250-300 us
// per layer whatever its size) - 13.6 + 21.2 ms of the 42 ms iteration at batch 64 (rocprofv3, tools/train_probe.py).

// out[b][r][p] (+)= sum_k Wm(r, k) in[b][k][p] (+ bias[r]);  Wm(r, k) = TRANS ? w[k * wld + r] : w[r * wld + k]
//   forward:        in = x,     out = y,      w = (Cout, Cin), wld = Cin
//   data gradient:  in = dy,    out = dx (+=), TRANS, w = the same (Cout, Cin) array, wld = Cin: dx[ci] += sum_co w[co][ci] dy[co]
// A wave = one image x 64 pixels x up to four 16-row tiles of output channels; lane (l, g): B operand = in[k0 + g][p0 + 16 e + l]
// for the four pixel tiles e (four coalesced dword loads), A operand = Wm(16 t + l, k0 + g); D lane (l, g) reg r = out row
// 16 t + 4 g + r, pixel p0 + 16 e + l.
template <bool TRANS, bool ACCUM, int MT>
__global__ __launch_bounds__(256) void pw_gemm_kernel(V in, V out, const float* __restrict__ w, const float* __restrict__ bias, int wld, int B) {
  constexpr int KS = 4;                            // MFMA steps (4 input channels each) per round of loads
  const int HW = out.H * out.W, K = in.C, M = out.C;
  const int lane = threadIdx.x & 63, l = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
  const int p0 = (blockIdx.x * 4 + wave) * 64, b = blockIdx.y, r0 = blockIdx.z * (16 * MT);
  if (p0 >= HW) return;
  f32x4 acc[MT][4];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[t][e] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* inb = in.p + ((size_t)b * in.Ctot + in.coff) * HW;
  const size_t kstride = (size_t)in.cstride * HW;
  // A round = the operands of KS MFMA steps (16 input channels), requested before the MFMAs of the round before it run.  The
  // first form fetched ONE step (4 channels) ahead: a layer was K / 4 dependent round trips to L2 with sixteen MFMAs each behind
  // them - 6 .. 72 of them, the launch's whole duration (the 51 pointwise convs of an iteration: 4.7 ms of its 12.3).  The
  // MFMAs run in the same order on the same operands: the results are bit-identical to that form.
  auto fetch = [&](int k0, float (&bv)[KS][4], float (&av)[KS][MT]) {
    // Every load is unconditional, from a clamped address, and what must not count is removed by an AND with a lane mask on the
    // FILTER operand only (a channel past K: filter entry 0 times a real, finite activation; rows past M and pixels past HW are
    // never stored).  A load behind a lane predicate - or a select the compiler turns back into one - is a branch, and the
    // compiler then waits for every load where it stands: the first version of this round waited twice per pair of loads.
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int k = k0 + 4 * j + g;
      const int kc = k < K ? k : K - 1;
      const unsigned km = k < K ? 0xffffffffu : 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) { const int p = p0 + 16 * e + l; bv[j][e] = inb[(size_t)kc * kstride + (p < HW ? p : HW - 1)]; }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int r = r0 + 16 * t + l, rc = r < M ? r : M - 1;
        const float v = TRANS ? w[(size_t)kc * wld + rc] : w[(size_t)rc * wld + kc];
        av[j][t] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & km);
      }
    }
  };
  auto mac = [&](int k0, const float (&bv)[KS][4], const float (&av)[KS][MT]) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      if (k0 + 4 * j >= K) break;                  // (wave-uniform: a step of zeros adds nothing, but costs its MFMAs)
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][t], bv[j][e], acc[t][e], 0, 0, 0);
    }
  };
  float b0[KS][4], a0[KS][MT], b1[KS][4], a1[KS][MT];
  fetch(0, b0, a0);
  for (int k0 = 0; k0 < K; k0 += 8 * KS) {
    fetch(k0 + 4 * KS, b1, a1);
    __builtin_amdgcn_sched_barrier(0);
    mac(k0, b0, a0);
    if (k0 + 4 * KS >= K) break;
    fetch(k0 + 8 * KS, b0, a0);
    __builtin_amdgcn_sched_barrier(0);
    mac(k0 + 4 * KS, b1, a1);
  }
  float* outb = out.p + ((size_t)b * out.Ctot + out.coff) * HW;
  const size_t rstride = (size_t)out.cstride * HW;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = r0 + 16 * t + 4 * g + rr;
      if (r >= M) continue;
      const float bi = bias ? bias[r] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int p = p0 + 16 * e + l;
        if (p < HW) { float* d = outb + (size_t)r * rstride + p; *d = ACCUM ? *d + acc[t][e][rr] : acc[t][e][rr] + bi; }
      }
    }
}

// weight gradient: scratch[co * Cin + ci] += sum over one image's pixel segment of dy[b][co][p] x[b][ci][p] (double atomics: the
// fp32 accumulation runs over at most `seg` pixels).  A wave = up to 3 x 3 tiles of 16 co x 16 ci x `upw` consecutive (image, segment)
// UNITS (round 5): each unit's fp32 sums are added to DOUBLE registers and the wave issues ONE set of atomics for all of them - a
// layer's ~2000 waves used to send ~2000 atomics to every filter entry (rocprofv3: 33 us per layer for ~5 us of matrix-core work; a
// sweep of the wave count alone gave 11.1 -> 10.6 ms per iteration at the price of four times longer fp32 sums - this form keeps
// the sums at `seg` pixels).  Per 16 pixels lane (l, g) holds pixels q + 4 g .. + 3 of channel row l of every tile: MFMA step e
// contracts pixel q + 4 g + e.
__global__ __launch_bounds__(64) void pw_wgrad_kernel(V x, V dy, double* __restrict__ scratch, int seg, int ci_blocks, int nseg, int units, int upw) {
  constexpr int T = 3;
  const int HW = x.H * x.W, Cin = x.C, Cout = dy.C;
  const int lane = threadIdx.x, l = lane & 15, g = lane >> 4;
  const int co0 = (blockIdx.z / ci_blocks) * (16 * T), ci0 = (blockIdx.z % ci_blocks) * (16 * T);
  const size_t xs = (size_t)x.cstride * HW, gs = (size_t)dy.cstride * HW;
  double dacc[T][T][4];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) dacc[i][j][rr] = 0.0;
#pragma unroll 1
  for (int u = blockIdx.x * upw; u < min(units, (int)(blockIdx.x + 1) * upw); ++u) {
  const int b = u / nseg, q0 = (u - b * nseg) * seg, q1 = min(HW, q0 + seg);
  f32x4 acc[T][T];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* xb = x.p + ((size_t)b * x.Ctot + x.coff) * HW;
  const float* gb = dy.p + ((size_t)b * dy.Ctot + dy.coff) * HW;
  auto fetch = [&](int q, float (&av)[T][4], float (&bv)[T][4]) {
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const int co = co0 + 16 * i + l, ci = ci0 + 16 * i + l;
      const int coc = co < Cout ? co : Cout - 1, cic = ci < Cin ? ci : Cin - 1;   // (unconditional loads, see pw_gemm_kernel: rows past
                                                                                 // Cout / Cin are never stored; a pixel past the segment
                                                                                 // gets a zero dy against a real, finite x)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int p = q + 4 * g + e, pc = p < q1 ? p : q1 - 1;
        const unsigned pm = p < q1 ? 0xffffffffu : 0u;
        av[i][e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, gb[(size_t)coc * gs + pc]) & pm);
        bv[i][e] = xb[(size_t)cic * xs + pc];
      }
    }
  };
  auto mac = [&](const float (&av)[T][4], const float (&bv)[T][4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
  };
  float a0[T][4], b0[T][4], a1[T][4], b1[T][4];
  fetch(q0, a0, b0);
  for (int q = q0; q < q1; q += 32) {
    fetch(q + 16, a1, b1);                        // (past q1: zeros)
    __builtin_amdgcn_sched_barrier(0);
    mac(a0, b0);
    if (q + 16 >= q1) break;
    fetch(q + 32, a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    mac(a1, b1);
  }
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) dacc[i][j][rr] += (double)acc[i][j][rr];
  }
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int co = co0 + 16 * i + 4 * g + rr, ci = ci0 + 16 * j + l;
        if (co < Cout && ci < Cin) atomicAdd(&scratch[(size_t)co * Cin + ci], dacc[i][j][rr]);
      }
}
// Every layer's weight gradient is summed in double in its own range of one scratch (zeroed per backward) and added to the bound
// gradient tensors by ONE launch at the end of the backward pass (round 4: it was a launch per layer, 79 of them).
struct FinishItem { const double* scr; float* dw; int n; int pad; };
struct FinishChunk { FinishItem it[96]; };
__global__ __launch_bounds__(256) void wgrad_finish_multi_kernel(FinishChunk c) {
  const FinishItem& t = c.it[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < t.n) t.dw[i] += (float)t.scr[i];
}

// the stem's weight gradient (3 x 3, stride 2, pad 1, 3 -> 24 channels, 176 x 176 outputs per image: the longest reduction of
// the network - 2 M terms per filter entry at batch 64; conv_bwd_weight_kernel: 3.9 ms): a thread walks output pixels with a
// stride, holds 8 output channels x 9 taps of one input channel as fp32 partial sums over at most 16 pixels, the block meets in
// LDS, one double atomic per entry and block.  grid (pixel blocks, 3 input channels, 3 groups of 8 output channels)
__global__ __launch_bounds__(256) void stem_wgrad_kernel(ConvP a, double* __restrict__ scratch) {
  const int OH = a.out.H, OW = a.out.W, IH = a.in.H, IW = a.in.W;
  const int ci = blockIdx.y, cog = blockIdx.z;
  const long long n = (long long)a.B * OH * OW;
  float acc[8][9];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[c][t] = 0.f;
  const long long i0 = (long long)blockIdx.x * 4096;
  for (int it = 0; it < 16; ++it) {
    const long long i = i0 + it * 256 + threadIdx.x;
    if (i >= n) break;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH), b = (int)(i / ((long long)OW * OH));
    float xv[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
        xv[ky * 3 + kx] = (iy >= 0 && iy < IH && ix >= 0 && ix < IW) ? a.in.p[a.in.at(b, ci, iy, ix)] : 0.f;
      }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float gv = a.out.p[a.out.at(b, 8 * cog + c, oy, ox)];
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[c][t] = __builtin_fmaf(gv, xv[t], acc[c][t]);
    }
  }
  __shared__ float red[4][72];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float v = acc[c][t];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
      if (lane == 0) red[wave][c * 9 + t] = v;
    }
  __syncthreads();
  if (threadIdx.x < 72) {
    const int c = threadIdx.x / 9, t = threadIdx.x % 9;
    const double v = (double)red[0][threadIdx.x] + (double)red[1][threadIdx.x] + (double)red[2][threadIdx.x] + (double)red[3][threadIdx.x];
    atomicAdd(&scratch[((size_t)(8 * cog + c) * a.in.C + ci) * 9 + t], v);
  }
}


// depthwise weight gradient (k x k, stride 1 or 2): dW[c][ky][kx] += sum_{b, oy, ox} dy[b][c][oy][ox] x[b][c][s oy - pad + ky][..].
// grid (pixel blocks of 4096, channels): a thread walks 16 output pixels of its channel with k*k fp32 partial sums, the block
// meets by wave shuffles + LDS, one double atomic per tap and block (conv_bwd_weight_kernel: a double LDS tree per tap, 98 us per
// layer at batch 64)
template <int KS>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(ConvP a, double* __restrict__ scratch) {
  constexpr int KK = KS * KS;
  const int OH = a.out.H, OW = a.out.W, IH = a.in.H, IW = a.in.W, c = blockIdx.y;
  const long long n = (long long)a.B * OH * OW;
  float acc[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t) acc[t] = 0.f;
  const long long i0 = (long long)blockIdx.x * 4096;
  for (int it = 0; it < 16; ++it) {
    const long long i = i0 + it * 256 + threadIdx.x;
    if (i >= n) break;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH), b = (int)(i / ((long long)OW * OH));
    const float gv = a.out.p[a.out.at(b, c, oy, ox)];
#pragma unroll
    for (int ky = 0; ky < KS; ++ky)
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
        const float xv = (iy >= 0 && iy < IH && ix >= 0 && ix < IW) ? a.in.p[a.in.at(b, c, iy, ix)] : 0.f;
        acc[ky * KS + kx] = __builtin_fmaf(gv, xv, acc[ky * KS + kx]);
      }
  }
  __shared__ float red[4][KK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < KK; ++t) {
    float v = acc[t];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) red[wave][t] = v;
  }
  __syncthreads();
  if (threadIdx.x < KK)
    atomicAdd(&scratch[(size_t)c * KK + threadIdx.x], (double)red[0][threadIdx.x] + (double)red[1][threadIdx.x] + (double)red[2][threadIdx.x] + (double)red[3][threadIdx.x]);
}

struct SgdChunk { yfv2_sgd_item it[96]; };
__global__ __launch_bounds__(256) void sgd_multi_kernel(SgdChunk c, float lr, float momentum, float wd) {
  const yfv2_sgd_item& t = c.it[blockIdx.y];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= t.n) return;
  const float d = t.grad[i] + wd * t.param[i];
  const float bb = t.first_step ? d : momentum * t.momentum_buf[i] + d;
  t.momentum_buf[i] = bb;
  t.param[i] = t.param[i] - lr * bb;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
inline unsigned bn_blocks(size_t n) { return (unsigned)((n + BN_EPB - 1) / BN_EPB); }

// A V with an offset (floats) in place of the pointer: a tensor of the arenas, or a channel window of one.  The activation sits at `off`
// of the activation arena, its gradient at `off` of the gradient arena; at() makes the V over either, or over a caller's dense tensor
struct Tens { size_t off = 0; int Ctot = 0, coff = 0, cstride = 1, C = 0, H = 0, W = 0; };
inline Tens dense(int C, int H, int W) { Tens t; t.Ctot = t.C = C; t.H = H; t.W = W; return t; }
inline Tens slice(Tens t, int coff, int cstride, int C) { t.coff = coff; t.cstride = cstride; t.C = C; return t; }   // of a whole tensor
inline V at(const Tens& t, const float* base) { return V{const_cast<float*>(base) + t.off, t.Ctot, t.coff, t.cstride, t.C, t.H, t.W}; }

// The kernels that serve a conv + BatchNorm op, decided when the op is recorded; kernel size, stride, padding and depthwise follow from it
enum class Conv { Pointwise, Dw3s1, Dw3s2, Dw5s1, Stem };
struct ConvGeom { int k, stride, pad, dw; };
constexpr ConvGeom GEOM[] = {{1, 1, 0, 0}, {3, 1, 1, 1}, {3, 2, 1, 1}, {5, 1, 2, 1}, {3, 2, 1, 0}};

// One step of the network, as data: Train::record writes the list, Train::run_forward / run_backward launch one step of it.  Offsets,
// not pointers, into everything this unit allocates (the blocks are sized from the finished list); the caller's tensors are resolved
enum class OpKind { ConvBn, MaxPool, Pass, UpCat, Head };
struct Op {
  OpKind kind = OpKind::ConvBn;
  Conv conv = Conv::Pointwise;   // ConvBn: its kernels (a Head is pointwise)
  Tens in, in2, out, y;          // Stem: `in` is the caller's image.  UpCat: out = cat(upsample2x(in), in2).  Head: `out` is the caller's logit tensor `slot`.  y: a conv's output before BatchNorm
  bool relu = false;
  int slot = 0;
  size_t stat = 0, bn_scr = 0, wg_scr = 0;   // ConvBn: mean | invstd in the activation arena; the op's range (doubles) of the BatchNorm scratch, of the weight-gradient scratch
  float *w = nullptr, *gw = nullptr, *bias = nullptr, *gbias = nullptr;            // conv weight, BatchNorm's (or the Head's) bias, and their gradients
  float *gam = nullptr, *ggam = nullptr, *rm = nullptr, *rv = nullptr;             // BatchNorm weight, its gradient, running statistics
  std::string name;              // the conv's state-dict name (yfv2_debug_train_relu_output)
};
struct Finish { size_t scr; float* dw; int n; };   // a weight gradient: its range of the scratch -> the bound tensor

struct Train {
  yfv2_config cfg{};
  std::map<std::string, float*> param, pgrad;   // the binding
  int B = 0; std::vector<Op> ops; size_t n_body = 0;   // the list recorded for batch B (empty after a new binding); ops[n_body ..] are the six output convs
  std::vector<Finish> fin;                      // in the order the backward first meets them (wgrad_finish_multi_kernel's chunks)
  std::vector<std::pair<std::string, Tens>> named;   // the tensors no conv names: the max-pool output, each block's output, the FPN concat (yfv2_debug_train_tensor)
  size_t arena_floats = 0, pool_ints = 0, bn_doubles = 0, wg_doubles = 0;   // what the list uses of the blocks below
  DeviceBlock acts, grads, pool_arg;            // the two arenas; the max-pool's winners
  DeviceBlock dscr;                             // four doubles per BatchNorm channel: sum, sum of squares, the two backward sums (zeroed per forward)
  DeviceBlock wscr;                             // double partial sums of every layer's weight gradient (zeroed per backward)
  const float* x = nullptr;                     // the last forward's input (a raw caller pointer: the stem's weight gradient re-reads it)
  bool forward_done = false;                    // a forward since the last backward
  std::string err;

  // ---- recording: ONE walk of the topology, which launches nothing
  Tens alloc(int C, int H, int W) {
    Tens t = dense(C, H, W); t.off = arena_floats;
    arena_floats += (((size_t)B * C * H * W) + 63) & ~(size_t)63;
    return t;
  }
  float* P(const std::string& n) { auto it = param.find(n); if (it == param.end() || !it->second) { if (err.empty()) err = "yfv2_train: tensor '" + n + "' is not bound"; return nullptr; } return it->second; }
  float* G(const std::string& n) { auto it = pgrad.find(n); if (it == pgrad.end() || !it->second) { if (err.empty()) err = "yfv2_train: gradient of '" + n + "' is not bound"; return nullptr; } return it->second; }
  void plain(OpKind kind, const Tens& in, const Tens& in2, const Tens& out) { Op o; o.kind = kind; o.in = in; o.in2 = in2; o.out = out; ops.push_back(o); }
  // conv (no bias) `prefix.i` + BatchNorm `prefix.(i + 1)` on batch statistics [+ ReLU]: `in` -> `out`, a channel window of a tensor
  void conv_bn(Conv conv, const Tens& in, const Tens& out, const std::string& prefix, int i, bool relu) {
    Op o; o.conv = conv; o.in = in; o.out = out; o.relu = relu; o.name = prefix + "." + std::to_string(i);
    const std::string bn = prefix + "." + std::to_string(i + 1);
    o.y = alloc(out.C, out.H, out.W);
    o.stat = alloc(1, 1, 4 * out.C).off;   // mean | invstd | (2 per channel unused)
    o.bn_scr = bn_doubles; bn_doubles += 4 * (size_t)out.C;
    o.w = P(o.name + ".weight"); o.gam = P(bn + ".weight"); o.bias = P(bn + ".bias"); o.rm = P(bn + ".running_mean"); o.rv = P(bn + ".running_var");
    o.gw = G(o.name + ".weight"); o.ggam = G(bn + ".weight"); o.gbias = G(bn + ".bias");
    ops.push_back(o);
  }
  Tens conv_bn(Conv conv, const Tens& in, int Cout, const std::string& prefix, int i, bool relu) {   // ... -> a new tensor of Cout channels
    const ConvGeom g = GEOM[(int)conv];
    const Tens out = alloc(Cout, (in.H + 2 * g.pad - g.k) / g.stride + 1, (in.W + 2 * g.pad - g.k) / g.stride + 1);
    conv_bn(conv, in, out, prefix, i, relu);
    return out;
  }
  Tens tower(const std::string& p, const Tens& in) {   // fpn.py: two DWConvblocks
    const Tens a = conv_bn(Conv::Dw5s1, in, 72, p, 0, true), b = conv_bn(Conv::Pointwise, a, 72, p, 3, false), c = conv_bn(Conv::Dw5s1, b, 72, p, 5, true);
    return conv_bn(Conv::Pointwise, c, 72, p, 8, false);
  }
  // biased 1x1 output conv (detector.py:25-31): tower -> the caller's NCHW logit tensor `slot`; its gradient arrives from the caller
  void head(const Tens& in, const std::string& name, int Cout, int slot) {
    Op o; o.kind = OpKind::Head; o.in = in; o.out = dense(Cout, in.H, in.W); o.slot = slot; o.name = name;
    o.w = P(name + ".weight"); o.bias = P(name + ".bias"); o.gw = G(name + ".weight"); o.gbias = G(name + ".bias");
    ops.push_back(o);
  }
  // the order yfv2_train_backward launches in: the six output convs as recorded, then everything before them in reverse
  template <class F> void for_each_backward(F f) {
    for (size_t i = n_body; i < ops.size(); ++i) f(ops[i]);
    for (size_t i = n_body; i-- > 0;) f(ops[i]);
  }
  // shufflenetv2.py:19-63,102-109, fpn.py, detector.py:21-47 for `batch` images: the list, every arena offset, both scratch ranges.
  // A tensor missing from the binding: `err`, and the list is not to be run
  void record(int batch) {
    B = batch; ops.clear(); fin.clear(); named.clear(); err.clear();
    arena_floats = bn_doubles = wg_doubles = 0;
    const int H = cfg.height, W = cfg.width, A = cfg.anchor_num;
    // the input is NOT copied: the stem reads the caller's tensor (it needs no gradient)
    const Tens stem = conv_bn(Conv::Stem, dense(3, H, W), 24, "backbone.first_conv", 0, true);
    Tens cur = alloc(24, H / 4, W / 4), c2;
    plain(OpKind::MaxPool, stem, {}, cur);
    named.emplace_back("backbone.maxpool", cur);
    pool_ints = (size_t)B * 24 * cur.H * cur.W;
    const int repeats[3] = {4, 8, 4}, chans[4] = {24, 48, 96, 192};
    for (int si = 0; si < 3; ++si) {
      const int cin = chans[si], cout = chans[si + 1], mid = cout / 2;
      for (int i = 0; i < repeats[si]; ++i) {
        const std::string p = "backbone.stage" + std::to_string(si + 2) + "." + std::to_string(i);
        const Tens out = alloc(cout, i ? cur.H : cur.H / 2, i ? cur.W : cur.W / 2);
        if (i == 0) {   // stride 2: out = cat(proj(x), main(x))
          const Tens pd = conv_bn(Conv::Dw3s2, cur, cin, p + ".branch_proj", 0, false);
          conv_bn(Conv::Pointwise, pd, slice(out, 0, 1, cin), p + ".branch_proj", 2, true);
          const Tens m1 = conv_bn(Conv::Pointwise, cur, mid, p + ".branch_main", 0, true), m2 = conv_bn(Conv::Dw3s2, m1, mid, p + ".branch_main", 3, false);
          conv_bn(Conv::Pointwise, m2, slice(out, cin, 1, cout - cin), p + ".branch_main", 5, true);
        } else {        // stride 1: even channels pass, odd channels -> main; out = cat(pass, main)
          plain(OpKind::Pass, slice(cur, 0, 2, mid), {}, slice(out, 0, 1, mid));
          const Tens m1 = conv_bn(Conv::Pointwise, slice(cur, 1, 2, mid), mid, p + ".branch_main", 0, true), m2 = conv_bn(Conv::Dw3s1, m1, mid, p + ".branch_main", 3, false);
          conv_bn(Conv::Pointwise, m2, slice(out, mid, 1, mid), p + ".branch_main", 5, true);
        }
        cur = out;
        named.emplace_back(p, out);
      }
      if (si == 1) c2 = cur;
    }
    const Tens c3 = cur, s3 = conv_bn(Conv::Pointwise, c3, 72, "fpn.conv1x1_3", 0, true);
    const Tens cls3 = tower("fpn.cls_head_3.block", s3), reg3 = tower("fpn.reg_head_3.block", s3);
    const Tens p2 = alloc(c3.C + c2.C, c2.H, c2.W);
    plain(OpKind::UpCat, c3, c2, p2);
    named.emplace_back("fpn.p2", p2);
    const Tens s2 = conv_bn(Conv::Pointwise, p2, 72, "fpn.conv1x1_2", 0, true);
    const Tens cls2 = tower("fpn.cls_head_2.block", s2), reg2 = tower("fpn.reg_head_2.block", s2);
    n_body = ops.size();
    head(reg2, "output_reg_layers", 4 * A, 0);
    head(cls2, "output_obj_layers", A, 1);
    head(cls2, "output_cls_layers", cfg.classes, 2);
    head(reg3, "output_reg_layers", 4 * A, 3);
    head(cls3, "output_obj_layers", A, 4);
    head(cls3, "output_cls_layers", cfg.classes, 5);
    // weight-gradient scratch, in the backward's order.  An output conv serves both scales with ONE tensor and keeps ONE range, where its
    // gradients accumulate (the output convs come first: `fin` holds at most three entries when it is searched)
    for_each_backward([&](Op& o) {
      if (o.kind != OpKind::ConvBn && o.kind != OpKind::Head) return;
      if (o.kind == OpKind::Head) for (const Finish& f : fin) if (f.dw == o.gw) { o.wg_scr = f.scr; return; }
      const ConvGeom g = GEOM[(int)o.conv];
      const int n = (g.dw ? o.out.C : o.out.C * o.in.C) * g.k * g.k;
      o.wg_scr = wg_doubles; wg_doubles += ((size_t)n + 1) & ~(size_t)1;
      fin.push_back(Finish{o.wg_scr, o.gw, n});
    });
  }

  // ---- running the list
  V act(const Tens& t) const { return at(t, acts.as<float>()); }
  V grad(const Tens& t) const { return at(t, grads.as<float>()); }
  V src(const Op& o) const { return o.conv == Conv::Stem ? at(o.in, x) : act(o.in); }   // what a conv reads: the stem, the caller's image
  // pointwise conv launchers (round 4): forward / data gradient as one GEMM, weight gradient = GEMM into the double scratch + finish
  void pw_forward(const V& in, const V& out, const float* w, const float* bias, hipStream_t s) const {
    const int HW = out.H * out.W;
    if (out.C <= 32) hipLaunchKernelGGL((pw_gemm_kernel<false, false, 2>), dim3((HW + 255) / 256, B, 1), dim3(256), 0, s, in, out, w, bias, in.C, B);   // (stage 2's 24 channels: two row tiles)
    else hipLaunchKernelGGL((pw_gemm_kernel<false, false, 4>), dim3((HW + 255) / 256, B, (out.C + 63) / 64), dim3(256), 0, s, in, out, w, bias, in.C, B);
  }
  void pw_data_grad(const V& din, const V& dout, const float* w, hipStream_t s) const {   // din += w^T dout
    const int HW = din.H * din.W;
    if (din.C <= 32) hipLaunchKernelGGL((pw_gemm_kernel<true, true, 2>), dim3((HW + 255) / 256, B, 1), dim3(256), 0, s, dout, din, w, (const float*)nullptr, din.C, B);
    else hipLaunchKernelGGL((pw_gemm_kernel<true, true, 4>), dim3((HW + 255) / 256, B, (din.C + 63) / 64), dim3(256), 0, s, dout, din, w, (const float*)nullptr, din.C, B);
  }
  void pw_weight_grad(const V& x, const V& dout, double* scr, hipStream_t s) const {
    const int HW = x.H * x.W, cob = (dout.C + 47) / 48, cib = (x.C + 47) / 48;
    int seg = 256;                                     // pixels per wave: enough waves for the machine, fp32 partial sums over few terms
    while (seg > 64 && (long long)((HW + seg - 1) / seg) * B * cob * cib < 2048) seg >>= 1;
    const int nseg = (HW + seg - 1) / seg, units = nseg * B;
    int upw = (int)(((long long)units * cob * cib) / 512);     // about 512 waves per layer (a launch below ~256 waves leaves CUs idle)
    if (upw < 1) upw = 1;
    if (upw > 16) upw = 16;
    hipLaunchKernelGGL(pw_wgrad_kernel, dim3((units + upw - 1) / upw, 1, cob * cib), dim3(64), 0, s, x, dout, scr, seg, cib, nseg, units, upw);
  }

  void conv_bn_forward(const Op& o, hipStream_t s) const {
    const ConvGeom g = GEOM[(int)o.conv];
    const int C = o.y.C, HW = o.y.H * o.y.W;
    const ConvP c{src(o), act(o.y), o.w, nullptr, g.k, g.stride, g.pad, g.dw, B};
    const dim3 planes((HW + 255) / 256, B * C);
    switch (o.conv) {
      case Conv::Pointwise: pw_forward(c.in, c.out, o.w, nullptr, s); break;
      case Conv::Dw3s1: hipLaunchKernelGGL((dw_fwd_kernel<3, 1>), planes, dim3(256), 0, s, c); break;
      case Conv::Dw3s2: hipLaunchKernelGGL((dw_fwd_kernel<3, 2>), planes, dim3(256), 0, s, c); break;
      case Conv::Dw5s1: hipLaunchKernelGGL((dw_fwd_kernel<5, 1>), planes, dim3(256), 0, s, c); break;
      case Conv::Stem: hipLaunchKernelGGL(stem_fwd_kernel, dim3(blocks_for((size_t)B * HW)), dim3(256), 0, s, c); break;
    }
    float* mean = acts.as<float>() + o.stat;
    double* ds = dscr.as<double>() + o.bn_scr;
    hipLaunchKernelGGL(bn_stats_part_kernel, dim3(C, reduce_segments((size_t)B * HW, C)), dim3(256), 0, s, c.out.p, B, C, HW, ds);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(bn_blocks((size_t)B * C * HW)), dim3(256), 0, s, c.out.p, act(o.out), B, ds, mean, mean + C, o.rm, o.rv, o.gam, o.bias, o.relu ? 1 : 0);
  }
  void conv_bn_backward(const Op& o, hipStream_t s) const {
    const ConvGeom g = GEOM[(int)o.conv];
    const int C = o.y.C, HW = o.y.H * o.y.W, relu = o.relu ? 1 : 0;
    const V y = act(o.y), dy = grad(o.y), z = act(o.out), dz = grad(o.out);
    float* mean = acts.as<float>() + o.stat;
    double* ds = dscr.as<double>() + o.bn_scr; double* scr = wscr.as<double>() + o.wg_scr;
    hipLaunchKernelGGL(bn_bwd_part_kernel, dim3(C, reduce_segments((size_t)B * HW, C)), dim3(256), 0, s, y.p, z, dz, B, mean, mean + C, relu, ds);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(bn_blocks((size_t)B * C * HW)), dim3(256), 0, s, y.p, z, dz, dy.p, B, mean, mean + C, o.gam, relu, ds, o.ggam, o.gbias);
    const ConvP cw{src(o), dy, nullptr, nullptr, g.k, g.stride, g.pad, g.dw, B};
    const unsigned chunks = (unsigned)(((size_t)B * HW + 4095) / 4096);   // of 4096 output pixels
    switch (o.conv) {
      case Conv::Pointwise: pw_weight_grad(cw.in, dy, scr, s); break;
      case Conv::Dw3s1:
      case Conv::Dw3s2: hipLaunchKernelGGL((dw_wgrad_kernel<3>), dim3(chunks, C), dim3(256), 0, s, cw, scr); break;
      case Conv::Dw5s1: hipLaunchKernelGGL((dw_wgrad_kernel<5>), dim3(chunks, C), dim3(256), 0, s, cw, scr); break;
      case Conv::Stem: hipLaunchKernelGGL(stem_wgrad_kernel, dim3(chunks, 3, 3), dim3(256), 0, s, cw, scr); break;
    }
    const ConvP cd{grad(o.in), dy, o.w, nullptr, g.k, g.stride, g.pad, g.dw, B};
    const dim3 planes((o.in.H * o.in.W + 255) / 256, B * o.in.C);
    switch (o.conv) {
      case Conv::Pointwise: pw_data_grad(cd.in, dy, o.w, s); break;
      case Conv::Dw3s1: hipLaunchKernelGGL((dw_bwd_data_kernel<3, 1>), planes, dim3(256), 0, s, cd); break;
      case Conv::Dw3s2: hipLaunchKernelGGL((dw_bwd_data_kernel<3, 2>), planes, dim3(256), 0, s, cd); break;
      case Conv::Dw5s1: hipLaunchKernelGGL((dw_bwd_data_kernel<5, 1>), planes, dim3(256), 0, s, cd); break;
      case Conv::Stem: break;   // the image needs no gradient
    }
  }

  void run_forward(const Op& o, float* const out6[6], hipStream_t s) const {
    const size_t n_out = (size_t)B * o.out.C * o.out.H * o.out.W;
    switch (o.kind) {
      case OpKind::ConvBn: conv_bn_forward(o, s); break;
      case OpKind::MaxPool: hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(blocks_for(n_out)), dim3(256), 0, s, act(o.in).p, act(o.out).p, pool_arg.as<int>(), B, o.in.C, o.in.H, o.in.W); break;
      case OpKind::Pass: hipLaunchKernelGGL(view_copy_kernel, dim3(blocks_for(n_out)), dim3(256), 0, s, act(o.out), act(o.in), B, 0); break;
      case OpKind::UpCat:
        hipLaunchKernelGGL(upsample2_kernel, dim3(blocks_for((size_t)B * o.in.C * o.out.H * o.out.W)), dim3(256), 0, s, act(slice(o.out, 0, 1, o.in.C)), act(o.in), B);
        hipLaunchKernelGGL(view_copy_kernel, dim3(blocks_for((size_t)B * o.in2.C * o.out.H * o.out.W)), dim3(256), 0, s, act(slice(o.out, o.in.C, 1, o.in2.C)), act(o.in2), B, 0);
        break;
      case OpKind::Head: pw_forward(act(o.in), at(o.out, out6[o.slot]), o.w, o.bias, s); break;
    }
  }
  void run_backward(const Op& o, const float* const grad6[6], hipStream_t s) const {
    const size_t n_in = (size_t)B * o.in.C * o.in.H * o.in.W;
    switch (o.kind) {
      case OpKind::ConvBn: conv_bn_backward(o, s); break;
      case OpKind::MaxPool: hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(blocks_for(n_in)), dim3(256), 0, s, grad(o.out).p, pool_arg.as<int>(), grad(o.in).p, B, o.in.C, o.in.H, o.in.W); break;
      case OpKind::Pass: hipLaunchKernelGGL(view_copy_kernel, dim3(blocks_for(n_in)), dim3(256), 0, s, grad(o.in), grad(o.out), B, 1); break;
      case OpKind::UpCat:
        hipLaunchKernelGGL(upsample2_bwd_kernel, dim3(blocks_for(n_in)), dim3(256), 0, s, grad(o.in), grad(slice(o.out, 0, 1, o.in.C)), B);
        hipLaunchKernelGGL(view_copy_kernel, dim3(blocks_for((size_t)B * o.in2.C * o.in2.H * o.in2.W)), dim3(256), 0, s, grad(o.in2), grad(slice(o.out, o.in.C, 1, o.in2.C)), B, 1);
        break;
      case OpKind::Head: {   // weights shared by the two scales -> their gradients accumulate (the caller zeroed the parameter gradients)
        const V go = at(o.out, grad6[o.slot]);
        hipLaunchKernelGGL(bias_bwd_kernel, dim3(go.C), dim3(256), 0, s, go, B, o.gbias);
        pw_weight_grad(act(o.in), go, wscr.as<double>() + o.wg_scr, s);
        pw_data_grad(grad(o.in), go, o.w, s);
        break;
      }
    }
  }
};

}  // namespace

// the training state hangs off the handle through an opaque slot (the handle is yfv2_ctx.h's; this unit reaches it through three accessors)
static Train* train_of(yfv2_handle h, bool create) {
  void** slot = yfv2_ctx_train_slot(h);
  if (!slot) return nullptr;
  if (!*slot && create) { Train* t = new Train(); t->cfg = *yfv2_ctx_config(h); *slot = t; }
  return static_cast<Train*>(*slot);
}
void yfv2_train_release(void* p) { delete static_cast<Train*>(p); }

extern "C" {

int yfv2_train_bind(yfv2_handle h, const yfv2_tensor_desc* tensors, int32_t n, const yfv2_tensor_desc* grads, int32_t ng) {
  if (!h || !tensors || n <= 0 || !grads || ng <= 0) return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_train_bind: bad argument");
  Train* t = train_of(h, true);
  // every bound buffer is indexed with the shapes the handle's configuration implies: a mis-sized one is refused here
  // (YFV2_ERR_WEIGHTS, like yfv2_load_weights), not read or written out of bounds later
  const std::map<std::string, int64_t> want = expected_numels(t->cfg);
  auto check = [&](const yfv2_tensor_desc& d, const char* what) -> int {
    auto it = want.find(d.name);
    if (it == want.end()) return YFV2_OK;               // not a tensor of this model: never looked up
    if (!d.data || d.numel != it->second)
      return yfv2_ctx_fail(h, YFV2_ERR_WEIGHTS, (std::string("yfv2_train_bind: ") + what + " '" + d.name + "' has " + std::to_string((long long)d.numel) +
                                                 " elements, expected " + std::to_string((long long)it->second)).c_str());
    return YFV2_OK;
  };
  for (int i = 0; i < n; ++i) if (tensors[i].name) if (int rc = check(tensors[i], "tensor")) return rc;
  for (int i = 0; i < ng; ++i) if (grads[i].name) if (int rc = check(grads[i], "gradient buffer")) return rc;
  t->param.clear(); t->pgrad.clear();
  for (int i = 0; i < n; ++i) if (tensors[i].name) t->param[tensors[i].name] = const_cast<float*>(tensors[i].data);
  for (int i = 0; i < ng; ++i) if (grads[i].name) t->pgrad[grads[i].name] = const_cast<float*>(grads[i].data);
  t->ops.clear(); t->forward_done = false;   // the list holds the OLD binding's pointers: the next forward records it again
  return YFV2_OK;
}

int yfv2_train_forward(yfv2_handle h, const float* x, int32_t B, float* const out6[6], void* stream) {
  if (!h || !x || !out6 || B < 1) return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_train_forward: bad argument");
  Train* t = train_of(h, false);
  if (!t || t->param.empty()) return yfv2_ctx_fail(h, YFV2_ERR_STATE, "yfv2_train_forward: yfv2_train_bind has not been called");
  // nn.BatchNorm2d in train mode refuses a channel with a single value (the coarsest map is height / 32 x width / 32 per image): the
  // batch variance of one value is 0 and the unbiased one undefined
  if ((int64_t)B * (t->cfg.height / 32) * (t->cfg.width / 32) <= 1)
    return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_train_forward: expected more than 1 value per channel when training (batch 1 on a 1 x 1 map)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->cfg.device);
  t->forward_done = false;
  if (t->ops.empty() || t->B != B) {
    t->record(B);
    if (!t->err.empty()) { t->ops.clear(); return yfv2_ctx_fail(h, YFV2_ERR_WEIGHTS, t->err.c_str()); }
  }
  // the five blocks, exactly as large as the list says (a block that grows waits for the device before it frees)
  if (int rc = t->acts.reserve(h, t->arena_floats * sizeof(float), true)) return rc;
  if (int rc = t->grads.reserve(h, t->arena_floats * sizeof(float), true)) return rc;
  if (int rc = t->pool_arg.reserve(h, t->pool_ints * sizeof(int), true)) return rc;
  if (int rc = t->dscr.reserve(h, t->bn_doubles * sizeof(double), true)) return rc;
  if (int rc = t->wscr.reserve(h, t->wg_doubles * sizeof(double), true)) return rc;
  if (hipMemsetAsync(t->dscr.p, 0, t->bn_doubles * sizeof(double), s) != hipSuccess) return yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_train_forward: memset failed");
  t->x = x;
  for (const Op& o : t->ops) t->run_forward(o, out6, s);
  if (hipGetLastError() != hipSuccess) return yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_train_forward: launch failed");
  t->forward_done = true;
  return YFV2_OK;
}

int yfv2_train_backward(yfv2_handle h, const float* const grad6[6], void* stream) {
  Train* t = h ? train_of(h, false) : nullptr;
  if (!t || !t->forward_done) return yfv2_ctx_fail(h, YFV2_ERR_STATE, "yfv2_train_backward: no recorded yfv2_train_forward");
  if (!grad6) return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_train_backward: null pointer");
  for (int i = 0; i < 6; ++i) if (!grad6[i]) return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_train_backward: null gradient tensor");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->cfg.device);
  if (hipMemsetAsync(t->grads.p, 0, t->arena_floats * sizeof(float), s) != hipSuccess) return yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_train_backward: memset failed");
  if (hipMemsetAsync(t->wscr.p, 0, t->wg_doubles * sizeof(double), s) != hipSuccess) return yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_train_backward: memset failed");
  t->forward_done = false;
  t->for_each_backward([&](const Op& o) { t->run_backward(o, grad6, s); });
  for (size_t i0 = 0; i0 < t->fin.size(); i0 += 96) {   // every weight gradient: scratch (double) -> the bound tensors
    FinishChunk c{};
    const int m = (int)std::min<size_t>(96, t->fin.size() - i0);
    int nmax = 0;
    for (int k = 0; k < m; ++k) {
      const Finish& f = t->fin[i0 + k];
      c.it[k] = FinishItem{t->wscr.as<double>() + f.scr, f.dw, f.n, 0};
      nmax = std::max(nmax, f.n);
    }
    hipLaunchKernelGGL(wgrad_finish_multi_kernel, dim3(blocks_for((size_t)nmax), m), dim3(256), 0, s, c);
  }
  if (hipGetLastError() != hipSuccess) return yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_train_backward: launch failed");
  return YFV2_OK;
}

// which: 0 the conv output y, 1 the op's output window (a named tensor: its value), 2 / 3 their gradients, 4 / 5 the saved mean / invstd
int64_t yfv2_debug_train_tensor(yfv2_handle h, const char* name, int32_t which, float* host_dst, int64_t capacity) {
  Train* t = h ? train_of(h, false) : nullptr;
  if (!t || !name || which < 0 || which > 5) { (void)yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_debug_train_tensor: bad argument"); return -1; }
  const auto it = std::find_if(t->ops.begin(), t->ops.end(), [&](const Op& o) { return o.kind == OpKind::ConvBn && o.name == name; });
  const auto nt = std::find_if(t->named.begin(), t->named.end(), [&](const std::pair<std::string, Tens>& p) { return p.first == name; });
  const bool is_conv = it != t->ops.end(), is_named = !is_conv && nt != t->named.end() && (which == 1 || which == 3);
  if ((!is_conv && !is_named) || !t->acts.p || !t->grads.p) {
    (void)yfv2_ctx_fail(h, YFV2_ERR_STATE, "yfv2_debug_train_tensor: no such tensor in the last yfv2_train_forward"); return -1;
  }
  DeviceGuard guard(t->cfg.device);
  Tens src;
  if (which >= 4) { src = dense(it->y.C, 1, 1); src.off = it->stat + (which == 5 ? (size_t)it->y.C : 0); }   // (C,): one "image" of C channels
  else src = is_named ? nt->second : ((which & 1) ? it->out : it->y);
  const int images = which >= 4 ? 1 : t->B;
  const V z = (which == 2 || which == 3) ? t->grad(src) : t->act(src);
  const int64_t n = (int64_t)images * z.C * z.H * z.W;
  if (!host_dst || capacity < n) return n;
  float* dense_p = nullptr;
  if (hipDeviceSynchronize() != hipSuccess || hipMalloc(reinterpret_cast<void**>(&dense_p), (size_t)n * sizeof(float)) != hipSuccess) {
    (void)yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_debug_train_tensor: device error"); return -1;
  }
  const V d{dense_p, z.C, 0, 1, z.C, z.H, z.W};
  hipLaunchKernelGGL(view_copy_kernel, dim3(blocks_for((size_t)n)), dim3(256), 0, nullptr, d, z, images, 0);
  const hipError_t e = hipMemcpy(host_dst, dense_p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(dense_p);
  if (e != hipSuccess) { (void)yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_debug_train_tensor: copy failed"); return -1; }
  return n;
}

int64_t yfv2_debug_train_relu_output(yfv2_handle h, const char* conv_name, float* host_dst, int64_t capacity) {
  Train* t = h ? train_of(h, false) : nullptr;
  if (!t || !conv_name) { (void)yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_debug_train_relu_output: bad argument"); return -1; }
  const auto it = std::find_if(t->ops.begin(), t->ops.end(), [&](const Op& o) { return o.kind == OpKind::ConvBn && o.relu && o.name == conv_name; });
  if (it == t->ops.end() || !t->acts.p) { (void)yfv2_ctx_fail(h, YFV2_ERR_STATE, "yfv2_debug_train_relu_output: no such ReLU output in the last yfv2_train_forward"); return -1; }
  return yfv2_debug_train_tensor(h, conv_name, 1, host_dst, capacity);   // the op's output window
}

int yfv2_sgd_step(yfv2_handle h, float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                  int32_t first_step, void* stream) {
  if (!h || !param || !grad || !momentum_buf || n < 0) return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_sgd_step: bad argument");
  if (n == 0) return YFV2_OK;
  const yfv2_sgd_item one{param, grad, momentum_buf, n, first_step ? 1 : 0, 0};   // (one tensor = a table of one: the same kernel)
  return yfv2_sgd_step_multi(h, &one, 1, lr, momentum, weight_decay, stream);
}

int yfv2_sgd_step_multi(yfv2_handle h, const yfv2_sgd_item* items, int32_t n_items, float lr, float momentum, float weight_decay, void* stream) {
  if (!h || !items || n_items < 0) return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_sgd_step_multi: bad argument");
  DeviceGuard guard(yfv2_ctx_config(h)->device);
  for (int i0 = 0; i0 < n_items; i0 += 96) {
    SgdChunk c{};
    const int m = n_items - i0 < 96 ? n_items - i0 : 96;
    int64_t nmax = 0;
    for (int k = 0; k < m; ++k) {
      const yfv2_sgd_item& t = items[i0 + k];
      if (!t.param || !t.grad || !t.momentum_buf || t.n < 0) return yfv2_ctx_fail(h, YFV2_ERR_ARG, "yfv2_sgd_step_multi: bad item");
      c.it[k] = t;
      if (t.n > nmax) nmax = t.n;
    }
    if (nmax == 0) continue;
    hipLaunchKernelGGL(sgd_multi_kernel, dim3(blocks_for((size_t)nmax), m), dim3(256), 0, static_cast<hipStream_t>(stream), c, lr, momentum, weight_decay);
  }
  if (hipGetLastError() != hipSuccess) return yfv2_ctx_fail(h, YFV2_ERR_DEVICE, "yfv2_sgd_step_multi: launch failed");
  return YFV2_OK;
}

}  // extern "C"
