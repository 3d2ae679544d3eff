// yfv2_ap_test.cpp - torch-free driver of yfv2::Detector::apPerClass (include/yfv2.hpp over yfv2_ap_per_class).
//   yfv2_ap_test <statistics file>
// The file: int64 N, int64 T, then tp int32[N], conf float[N], pred_cls float[N], target_cls float[T] (little endian, as numpy
// writes them).  Prints "present <count> bad <flag>", one line "<class> <n_gt> <n_pred> <p> <r> <ap>" per present class and
// "means <p> <r> <ap> <f1>", floating-point numbers as C99 hex floats (every bit).  tests/test_gpu_ap.py compares the lines
// with the numpy model.  Exit status: 0 ok, 2 usage / file, 3 library error.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../include/yfv2.hpp"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <statistics file>\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int64_t n = 0, t = 0;
  if (std::fread(&n, 8, 1, f) != 1 || std::fread(&t, 8, 1, f) != 1 || n < 0 || t < 0 || n > (1 << 26) || t > (1 << 26)) { std::fclose(f); return 2; }
  std::vector<int32_t> tp((size_t)n);
  std::vector<float> conf((size_t)n), cls((size_t)n), tgt((size_t)t);
  const bool ok = (!n || (std::fread(tp.data(), 4, (size_t)n, f) == (size_t)n && std::fread(conf.data(), 4, (size_t)n, f) == (size_t)n &&
                          std::fread(cls.data(), 4, (size_t)n, f) == (size_t)n)) &&
                  (!t || std::fread(tgt.data(), 4, (size_t)t, f) == (size_t)t);
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "truncated statistics file\n"); return 2; }

  const double anchors[12] = {1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6};   // any configuration will do: no forward runs
  yfv2::Detector det(1, anchors, 32, 32);
  if (!det.ok()) { std::fprintf(stderr, "create: %s\n", det.lastError()); return 3; }
  yfv2_ap_result res{};
  if (det.apPerClass(tp.data(), conf.data(), cls.data(), n, tgt.data(), t, res) != YFV2_OK) { std::fprintf(stderr, "apPerClass: %s\n", det.lastError()); return 3; }
  std::printf("present %d bad %d\n", res.classes_present, res.bad_input);
  for (int c = 0; c < 256; ++c)
    if (res.n_gt[c] > 0) std::printf("%d %" PRId64 " %" PRId64 " %a %a %a\n", c, res.n_gt[c], res.n_pred[c], res.p[c], res.r[c], res.ap[c]);
  std::printf("means %a %a %a %a\n", res.mean_p, res.mean_r, res.mean_ap, res.mean_f1);
  return 0;
}
