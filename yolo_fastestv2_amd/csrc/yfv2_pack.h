// yfv2_pack.h - the host-side weight packer of libyfv2.so: reference state_dict -> one blob of kernel-ready parameters
// (BatchNorm folded, every filter laid out in the register / LDS order its kernel reads).  Host only: no kernel, no HIP
// runtime call.  The layouts are specified above the definitions in yfv2_pack.hip; the plan (yfv2_plan.hip: PlanBuilder)
// decides which images a configuration needs and in which order they enter the blob.  Not part of the public ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/yfv2.h"

struct Folded { size_t w = 0, scale = 0, shift = 0; };  // offsets (floats) into the param blob

// name -> element count of every floating-point state_dict entry of the architecture for this configuration: what a weight load
// (WeightPacker::index) and a training bind (yfv2_train.hip) hold the caller's tensors against
std::map<std::string, int64_t> expected_numels(const yfv2_config& cfg);

struct WeightPacker {
  std::map<std::string, const yfv2_tensor_desc*> byname;
  std::vector<float> blob;
  std::string missing;   // why index() refused: the first entry of the table that is missing or mis-sized

  // Indexes the caller's tensors and checks them against expected_numels(cfg): false (and `missing`) at the first entry, in the
  // table's order, that is absent, has null data or another element count.  Nothing below may run before this has returned true:
  // the folds read every tensor they name without looking again.
  bool index(const yfv2_config& cfg, const yfv2_tensor_desc* tensors, int32_t n);
  const float* get(const std::string& name) const { return byname.find(name)->second->data; }
  size_t reserve(size_t n) {  // 16-byte aligned slots
    size_t off = (blob.size() + 3) & ~size_t(3);
    blob.resize(off + n, 0.f);
    return off;
  }
  size_t put(const std::vector<float>& im) {
    const size_t off = reserve(im.size());
    std::memcpy(&blob[off], im.data(), sizeof(float) * im.size());
    return off;
  }
  // a 32-bit pattern (packed fp16 / bf16 pairs, int tables) as one float of an image
  static void push_bits(std::vector<float>& im, uint32_t u) { float f; std::memcpy(&f, &u, 4); im.push_back(f); }
  static void push_bits(std::vector<float>& im, int v) { push_bits(im, (uint32_t)v); }

  // ---- folded layers: raw arrays in the blob (BatchNorm -> scale / shift)
  void bn(const std::string& name, int c, Folded* f);
  void pw(const std::string& conv, const std::string& bnname, int co, int ci, Folded* f);
  void dw(const std::string& conv, const std::string& bnname, int c, int k, Folded* f);
  void stem(const std::string& conv, const std::string& bnname, Folded* f);
  void heads(const std::vector<std::pair<std::string, int>>& parts, int ci, Folded* f);
  void heads_range(const std::string& name, int r0, int n, int ci, Folded* f);   // rows [r0, r0 + n) of the conv's rows
  Folded pw_columns(const Folded& f, int co, int ci, int c0, int n);
  Folded permuted_pw_inputs(const Folded& f, int co, int ci, const int* label);
  Folded permuted_pw_outputs(const Folded& f, int co, int ci, const int* label);
  Folded permuted_dw_channels(const Folded& f, int c, int kk, const int* label);

  // ---- images: the exact, zero-padded block of floats a kernel copies into LDS (or its registers) in its prologue,
  // built from the arrays above; each returns the image's offset in the blob
  size_t image_stem(const Folded& f, float in_scale = 1.0f);
  size_t image_stem16(const Folded& f);
  size_t image_pw(const Folded& f, int M, int K, int MT /* the M tiles of the kernel instantiation, yfv2_pw_tiles */, bool presplit = false);
  size_t image_pw_dual(const Folded& f0, const Folded& f1, int M, int K, int MT);
  size_t image_s2(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, int cin, bool w1_split3 = false);
  size_t image_s2w(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp) { return image_s2(f1, fd, f2, fpd, fpp, 96, true); }
  size_t image_tower(const Folded& fd, const Folded& fp, const Folded* fh, int mh);
  size_t image_towerh(const Folded& fd, const Folded& fp, const Folded* fh, int mh, int mh_tiles);
  size_t image_s1px(const Folded& f1, const Folded& fd, const Folded& f2, const int (&order)[24]);
  size_t image_s1h(const Folded& f1, const Folded& fd, const Folded& f2, const int (&order)[24], const int (&src_off)[12], const int (&dst_off)[12]);
  size_t image_s2px_proj(const Folded& fpd, const Folded& fpp, const int (&pos)[24]);
  size_t image_s2px_main(const Folded& f1, const Folded& fd, const Folded& f2, const int (&pos)[24]);
  size_t image_s2h(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, const int (&pos)[2][24],
                   const int (&st2_off)[2][8], const int (&st1_off)[2][8], int IH, int IW);
  size_t image_s3h(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, unsigned pp_mask,
                   long long pp_bufstride, int IH, int IW);
  size_t image_s4h(const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp);
  // one block of block_s1chain6_kernel's image, appended to im (the plan adds the block's int tables behind it)
  void append_s1_bf6(std::vector<float>& im, const Folded& f1, const Folded& fd, const Folded& f2);
  // block_s1pool_kernel's image of a whole chain; *ok is cleared if a pass is not yfv2_s1pool_image_floats(pre) floats
  size_t image_s1pool(const std::vector<Folded>& f1, const std::vector<Folded>& fd, const std::vector<Folded>& f2, int c2, bool pre, bool* ok);

 private:
  void build_pw(std::vector<float>& im, const Folded& f, int M, int K, int MT, bool presplit);
  void build_s2_stream(std::vector<float>& im, const Folded& f1, const Folded& fd, const Folded& f2, const Folded& fpd, const Folded& fpp, int C);
};
