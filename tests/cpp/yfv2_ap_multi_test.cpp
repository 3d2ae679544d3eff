// yfv2_ap_multi_test.cpp - torch-free driver of yfv2::Detector::apPerClassMulti (include/yfv2.hpp over yfv2_ap_per_class_multi).
//   yfv2_ap_multi_test <statistics file>
// The file: int64 N, int64 T, int64 K, then tpmask uint32[N], conf float[N], pred_cls float[N], target_cls float[T] (little endian,
// as numpy writes them).  Prints, for k = 0..K-1, "threshold <k> present <count> bad <flag>", one line
// "<class> <n_gt> <n_pred> <p> <r> <ap>" per present class and "means <p> <r> <ap> <f1>", floating-point numbers as C99 hex floats
// (every bit).  tests/test_gpu_ap_multi.py compares the lines with the Python path.  Exit status: 0 ok, 2 usage / file, 3 library error.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../include/yfv2.hpp"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <statistics file>\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int64_t n = 0, t = 0, k = 0;
  if (std::fread(&n, 8, 1, f) != 1 || std::fread(&t, 8, 1, f) != 1 || std::fread(&k, 8, 1, f) != 1 || n < 0 || t < 0 || n > (1 << 26) || t > (1 << 26) ||
      k < 1 || k > 32) { std::fclose(f); return 2; }
  std::vector<uint32_t> mask((size_t)n);
  std::vector<float> conf((size_t)n), cls((size_t)n), tgt((size_t)t);
  const bool ok = (!n || (std::fread(mask.data(), 4, (size_t)n, f) == (size_t)n && std::fread(conf.data(), 4, (size_t)n, f) == (size_t)n &&
                          std::fread(cls.data(), 4, (size_t)n, f) == (size_t)n)) &&
                  (!t || std::fread(tgt.data(), 4, (size_t)t, f) == (size_t)t);
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "truncated statistics file\n"); return 2; }

  const double anchors[12] = {1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6};   // any configuration will do: no forward runs
  yfv2::Detector det(1, anchors, 32, 32);
  if (!det.ok()) { std::fprintf(stderr, "create: %s\n", det.lastError()); return 3; }
  std::vector<yfv2_ap_result> res((size_t)k);
  if (det.apPerClassMulti(mask.data(), conf.data(), cls.data(), n, tgt.data(), t, (int)k, res.data()) != YFV2_OK) {
    std::fprintf(stderr, "apPerClassMulti: %s\n", det.lastError());
    return 3;
  }
  for (int j = 0; j < (int)k; ++j) {
    const yfv2_ap_result& r = res[(size_t)j];
    std::printf("threshold %d present %d bad %d\n", j, r.classes_present, r.bad_input);
    for (int c = 0; c < 256; ++c)
      if (r.n_gt[c] > 0) std::printf("%d %" PRId64 " %" PRId64 " %a %a %a\n", c, r.n_gt[c], r.n_pred[c], r.p[c], r.r[c], r.ap[c]);
    std::printf("means %a %a %a %a\n", r.mean_p, r.mean_r, r.mean_ap, r.mean_f1);
  }
  return 0;
}
