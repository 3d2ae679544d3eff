// Host-only sanitizer driver for the 8-bit YUV samplings beyond 4:2:0 (tests/test_yuv_any_host.py builds it with
// `make -C yolo_fastestv2_amd/csrc yuv_any_san`): this file and the API units compiled with -fsanitize=address,undefined on the host
// side only, into a program of its own that opens no device.  Two things run here:
//   yfv2_debug_rows_any   the general launch's LDS bytes and width limit, swept over w, W and the five row kinds against the layout
//                         restated below; the limit is exact
//   yfv2_yuv_move         the HOST instance of the fold (yfv2_internal.h; crop_plan_kernel runs the device instance): for every
//                         format and origins 0..3 x 0..3, what the kernel reads for pixel (r, c) of the moved descriptor is the byte
//                         that include/yfv2.h's table names for pixel (dy + r, dx + c) of the planes; a fold of a fold is the fold
//                         of the sum
// Exits 0 and prints "yuv_any_san ok" when nothing was reported and every comparison held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/yfv2.h"
#include "../../yolo_fastestv2_amd/csrc/yfv2_internal.h"

static long g_checks = 0;
#define CHECK(cond, ...)                                                        \
  do {                                                                          \
    ++g_checks;                                                                 \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);           \
      std::fprintf(stderr, __VA_ARGS__);                                        \
      std::fprintf(stderr, "\n");                                               \
      std::exit(1);                                                             \
    }                                                                           \
  } while (0)

// ---- the general launch's LDS, from the layout: six slots of a full-width row, then the row kind's own bytes
static long long slot(long long n, int a) { return (n + 3 + a - 1) / a * a; }
static long long model_lds(int kind, int w, int W) {
  const int a = kind <= 1 ? 4 : 16;
  const long long own = kind <= 1 ? 3ll * W : kind == 2 ? 1024 + 12ll * W : kind == 3 ? 12ll * W : 6ll * W;
  return 6 * slot(w, a) + own;
}

static void sweep_rows() {
  const long long FULL = 160 * 1024;
  for (int kind = 0; kind < 5; ++kind)
    for (int W : {32, 352, 4096}) {
      int64_t lds = -1, lds1 = -1;
      int32_t limit = -1, limit420 = -1;
      CHECK(yfv2_debug_rows_any(kind, 1, W, &lds, &limit) == YFV2_OK && limit >= 1, "rows_any(%d, 1, %d)", kind, W);
      CHECK(yfv2_debug_rows(kind, 1, 1, W, nullptr, &limit420) == YFV2_OK && limit <= limit420, "kind %d W %d: general limit %d above the 4:2:0 limit %d", kind, W, limit, limit420);
      std::vector<int> ws;
      for (int w = 1; w <= 4100; ++w) ws.push_back(w);
      for (int d = -2; d <= 2; ++d)
        if (limit + d >= 1) ws.push_back(limit + d);
      for (int w : ws) {
        int32_t l2 = -1;
        CHECK(yfv2_debug_rows_any(kind, w, W, &lds, &l2) == YFV2_OK && l2 == limit, "rows_any(%d, %d, %d)", kind, w, W);
        CHECK(lds == model_lds(kind, w, W), "kind %d w %d W %d: %lld bytes, the layout takes %lld", kind, w, W, (long long)lds, model_lds(kind, w, W));
        // what the staging writes fits: a full-width row in one slot, a packed row of 2 w + 4 bytes in three, at misalignments 0..3
        const int a = kind <= 1 ? 4 : 16;
        for (int mis = 0; mis < 4; ++mis) {
          CHECK(4 * ((mis + (long long)w + 3) >> 2) <= slot(w, a), "a row of %d bytes at misalignment %d leaves its slot", w, mis);
          CHECK(4 * ((mis + 2ll * w + 4 + 3) >> 2) <= 3 * slot(w, a), "a packed row of %d pixels at misalignment %d leaves its three slots", w, mis);
        }
      }
      CHECK(yfv2_debug_rows_any(kind, limit, W, &lds, nullptr) == YFV2_OK && yfv2_debug_rows_any(kind, limit + 1, W, &lds1, nullptr) == YFV2_OK, "at the limit");
      CHECK(lds <= FULL && FULL < lds1, "kind %d W %d: limit %d is not exact (%lld, %lld)", kind, W, limit, (long long)lds, (long long)lds1);
    }
  CHECK(yfv2_debug_rows_any(5, 8, 8, nullptr, nullptr) == YFV2_ERR_ARG && yfv2_debug_rows_any(0, 0, 8, nullptr, nullptr) == YFV2_ERR_ARG &&
            yfv2_debug_rows_any(0, 8, 0, nullptr, nullptr) == YFV2_ERR_ARG && yfv2_debug_rows_any(-1, 8, 8, nullptr, nullptr) == YFV2_ERR_ARG,
        "rows_any arguments");
  CHECK(yfv2_debug_rows_any(0, 1920, 352, nullptr, nullptr) == YFV2_OK, "either output may be NULL");
}

// ---- the fold.  A caller's frame as its descriptor at origin (0, 0): what YuvFrames::expand (yfv2_api_frames.hip) writes in front
// of its yfv2_yuv_move.
struct Planes { const unsigned char *y, *u, *v; long long pitch_y, pitch_c; };
static ResizeFrameYuv descriptor(const Planes& p, int format) {
  ResizeFrameYuv r{};
  r.format = format; r.px = 0; r.py = 0;
  r.y = p.y; r.ca = p.u; r.cb = yfv2_yuv_planar(format) ? p.v : nullptr;
  r.pitch_y = p.pitch_y; r.pitch_c = p.pitch_c;
  if (yfv2_yuv_packed(format)) { r.y = p.y + (format == YFV2_YUV_UYVY ? 1 : 0); r.ca = p.y + (format == YFV2_YUV_YUYV ? 1 : 0); r.pitch_c = p.pitch_y; }
  if (yfv2_yuv_grey(format)) { r.ca = nullptr; r.pitch_c = 0; }
  return r;
}
// include/yfv2.h's table: the addresses pixel (R, C) of the planes reads (U and V null for GREY)
struct Reads { const unsigned char *y, *u, *v; };
static Reads table(const Planes& p, int format, long long R, long long C) {
  const int sb = (format & 16) ? 2 : 1;
  switch (format) {
    case YFV2_YUV_NV12: case YFV2_YUV_P010: return {p.y + R * p.pitch_y + sb * C, p.u + (R >> 1) * p.pitch_c + 2 * sb * (C >> 1), p.u + (R >> 1) * p.pitch_c + 2 * sb * (C >> 1) + sb};
    case YFV2_YUV_NV21: return {p.y + R * p.pitch_y + C, p.u + (R >> 1) * p.pitch_c + 2 * (C >> 1) + 1, p.u + (R >> 1) * p.pitch_c + 2 * (C >> 1)};
    case YFV2_YUV_I420: case YFV2_YUV_I010: return {p.y + R * p.pitch_y + sb * C, p.u + (R >> 1) * p.pitch_c + sb * (C >> 1), p.v + (R >> 1) * p.pitch_c + sb * (C >> 1)};
    case YFV2_YUV_I422: return {p.y + R * p.pitch_y + C, p.u + R * p.pitch_c + (C >> 1), p.v + R * p.pitch_c + (C >> 1)};
    case YFV2_YUV_I440: return {p.y + R * p.pitch_y + C, p.u + (R >> 1) * p.pitch_c + C, p.v + (R >> 1) * p.pitch_c + C};
    case YFV2_YUV_I444: return {p.y + R * p.pitch_y + C, p.u + R * p.pitch_c + C, p.v + R * p.pitch_c + C};
    case YFV2_YUV_YUYV: return {p.y + R * p.pitch_y + 2 * C, p.y + R * p.pitch_y + 4 * (C >> 1) + 1, p.y + R * p.pitch_y + 4 * (C >> 1) + 3};
    case YFV2_YUV_UYVY: return {p.y + R * p.pitch_y + 2 * C + 1, p.y + R * p.pitch_y + 4 * (C >> 1), p.y + R * p.pitch_y + 4 * (C >> 1) + 2};
    default: return {p.y + R * p.pitch_y + C, nullptr, nullptr};   // YFV2_YUV_GREY
  }
}
// what resize_frames_yuv_kernel reads for pixel (r, c) of a descriptor (yfv2_pre.hip), restated
static Reads kernel_reads(const ResizeFrameYuv& d, long long r, long long c) {
  const int f = d.format, sb = (f & 16) ? 2 : 1;
  const int sx = yfv2_yuv_shift_x(f), sy = yfv2_yuv_shift_y(f);
  const long long cr = (r + d.py) >> sy, j = (c + d.px) >> sx;
  if (yfv2_yuv_grey(f)) return {d.y + r * d.pitch_y + c, nullptr, nullptr};
  if (yfv2_yuv_packed(f)) return {d.y + r * d.pitch_y + 2 * c, d.ca + cr * d.pitch_c + 4 * j, d.ca + cr * d.pitch_c + 4 * j + 2};
  if (d.cb) return {d.y + r * d.pitch_y + sb * c, d.ca + cr * d.pitch_c + sb * j, d.cb + cr * d.pitch_c + sb * j};
  const unsigned char* a = d.ca + cr * d.pitch_c + 2 * sb * j;
  return f == YFV2_YUV_NV21 ? Reads{d.y + r * d.pitch_y + c, a + 1, a} : Reads{d.y + r * d.pitch_y + sb * c, a, a + sb};
}

static void sweep_fold() {
  const int formats[] = {YFV2_YUV_NV12, YFV2_YUV_NV21, YFV2_YUV_I420, YFV2_YUV_I422, YFV2_YUV_I440, YFV2_YUV_I444,
                         YFV2_YUV_YUYV, YFV2_YUV_UYVY, YFV2_YUV_GREY, YFV2_YUV_P010, YFV2_YUV_I010};
  // one heap block per plane, exactly as large as an 8 x 8 picture of 2-byte samples at these pitches needs: every pointer the
  // fold forms for origins up to (3 + 3, 3 + 3) and pixels up to (1, 1) beyond stays inside its block
  const long long pitch_y = 37, pitch_c = 41;
  std::vector<unsigned char> by((size_t)(8 * pitch_y)), bu((size_t)(8 * pitch_c)), bv((size_t)(8 * pitch_c));
  const Planes p{by.data(), bu.data(), bv.data(), pitch_y, pitch_c};
  for (int format : formats) {
    const bool sub_x = yfv2_yuv_shift_x(format) == 1 && !yfv2_yuv_grey(format), sub_y = yfv2_yuv_shift_y(format) == 1;
    for (int dy = 0; dy < 4; ++dy)
      for (int dx = 0; dx < 4; ++dx) {
        ResizeFrameYuv d = descriptor(p, format);
        yfv2_yuv_move(d, dx, dy);
        CHECK(d.px == (sub_x ? dx & 1 : 0) && d.py == (sub_y ? dy & 1 : 0), "format %d origin (%d, %d): parity (%d, %d)", format, dx, dy, d.px, d.py);
        for (int r = 0; r < 2; ++r)
          for (int c = 0; c < 2; ++c) {
            const Reads want = table(p, format, dy + r, dx + c), got = kernel_reads(d, r, c);
            CHECK(got.y == want.y && got.u == want.u && got.v == want.v, "format %d origin (%d, %d) pixel (%d, %d): luma %td / %td, U %td / %td, V %td / %td", format, dx, dy, r,
                  c, got.y - p.y, want.y - p.y, got.u ? got.u - p.u : -1, want.u ? want.u - p.u : -1, got.v ? got.v - p.u : -1, want.v ? want.v - p.u : -1);
          }
        // a tile's origin, then a crop's inside it: the fold of a fold
        for (int ey = 0; ey < 3; ++ey)
          for (int ex = 0; ex < 3; ++ex) {
            ResizeFrameYuv two = d, one = descriptor(p, format);
            yfv2_yuv_move(two, ex, ey);
            yfv2_yuv_move(one, dx + ex, dy + ey);
            CHECK(two.y == one.y && two.ca == one.ca && two.cb == one.cb && two.px == one.px && two.py == one.py, "format %d: (%d, %d) then (%d, %d)", format, dx, dy, ex, ey);
          }
      }
  }
}

int main() {
  sweep_rows();
  sweep_fold();
  std::printf("yuv_any_san ok: %ld checks\n", g_checks);
  return 0;
}
