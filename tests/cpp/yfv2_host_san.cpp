// Host-only sanitizer driver (tests/test_abi_and_host.py builds it with `make -C yolo_fastestv2_amd/csrc host_san`): the API, plan
// and pack units compiled with -fsanitize=address,undefined, called through entry points that never open a device.  Every tensor
// is a heap block of exactly its element count, so a fold that reads past a tensor, or a plan built from an incomplete set, is a
// sanitizer report.  Exits 0 and prints "host_san ok" when nothing was reported and every call returned what it must.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/yfv2.h"
#include "../../yolo_fastestv2_amd/csrc/yfv2_pack.h"   // expected_numels: the table yfv2_load_weights checks against

static int g_checks = 0;
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

// a complete state dict from the table: a fixed pattern, positive variances
struct StateDict {
  std::vector<std::string> names;
  std::vector<std::unique_ptr<float[]>> data;
  std::vector<yfv2_tensor_desc> descs;
  explicit StateDict(const std::map<std::string, int64_t>& table) {
    names.reserve(table.size());
    for (const auto& [name, numel] : table) {
      names.push_back(name);
      data.emplace_back(new float[(size_t)numel]);
      const bool var = name.size() > 12 && name.compare(name.size() - 12, 12, ".running_var") == 0;
      const int64_t k = (int64_t)names.size();
      for (int64_t i = 0; i < numel; ++i) data.back()[(size_t)i] = var ? 0.5f + 0.1f * (float)(i % 7) : 0.01f * (float)((i * 37 + k * 11) % 41 - 20);
      descs.push_back(yfv2_tensor_desc{});
      descs.back().name = names.back().c_str();
      descs.back().data = data.back().get();
      descs.back().numel = numel;
    }
  }
};

// towerp_kernel's lane -> patch table and the maps that take it.  Declared by hand because yfv2_internal.h needs the HIP headers: keep
// the two lines in step with their declarations there (next to yfv2_towerh_supported)
void towerp_lane_patches(int H, int W, unsigned char (&tbl)[128]);
bool yfv2_towerp_map(int H, int W);

static int dryrun(const yfv2_config& cfg, const yfv2_plan& plan, const std::vector<yfv2_tensor_desc>& descs, int32_t* steps, int64_t* blob) {
  return yfv2_debug_plan_dryrun_ex(&cfg, &plan, descs.data(), (int32_t)descs.size(), steps, blob);
}

int main() {
  const int classes[2] = {80, 100}, sizes[2][2] = {{352, 352}, {64, 96}};
  for (int c : classes)
    for (const auto& hw : sizes)
      for (int layer : {0, 1}) {
        yfv2_config cfg{};
        cfg.classes = c; cfg.anchor_num = 3; cfg.height = hw[0]; cfg.width = hw[1]; cfg.max_batch = 2; cfg.device = 0;
        yfv2_plan plan{};
        plan.struct_size = (int32_t)sizeof(plan);
        plan.layer_by_layer = layer;
        const std::map<std::string, int64_t> table = expected_numels(cfg);
        int32_t steps = 0; int64_t blob = 0;
        const StateDict sd(table);
        CHECK(dryrun(cfg, plan, sd.descs, &steps, &blob) == YFV2_OK && steps >= 11 && blob > 0, "%d classes %dx%d layer_by_layer=%d: %s", c, hw[0], hw[1],
              layer, yfv2_last_error(nullptr));
        for (size_t i = 0; i < sd.descs.size(); ++i) {
          const std::string& name = sd.names[i];
          const int64_t numel = sd.descs[i].numel;
          std::vector<yfv2_tensor_desc> without = sd.descs;
          without.erase(without.begin() + (long)i);
          CHECK(dryrun(cfg, plan, without, &steps, &blob) == YFV2_ERR_WEIGHTS, "without %s", name.c_str());
          CHECK(std::string(yfv2_last_error(nullptr)) == "missing tensor '" + name + "'", "without %s: %s", name.c_str(), yfv2_last_error(nullptr));
          std::vector<yfv2_tensor_desc> one_short = sd.descs;
          const std::unique_ptr<float[]> shorter(new float[(size_t)numel - 1]());   // a block of its own: reading element numel - 1 is a report
          one_short[i].data = shorter.get();
          one_short[i].numel = numel - 1;
          CHECK(dryrun(cfg, plan, one_short, &steps, &blob) == YFV2_ERR_WEIGHTS, "%s one element short", name.c_str());
          CHECK(std::string(yfv2_last_error(nullptr)) == "tensor '" + name + "' has " + std::to_string(numel - 1) + " elements, expected " + std::to_string(numel),
                "%s one element short: %s", name.c_str(), yfv2_last_error(nullptr));
        }
      }

  // the tile plan of a 1000 x 1500 frame: counted, then written into an array of exactly that many tiles
  const int n_tiles = yfv2_tile_plan(1000, 1500, 352, 352, 64, 64, 1, nullptr, 0);
  CHECK(n_tiles == 4 * 5 + 1, "%d tiles", n_tiles);   // stride 288: rows at 0, 288, 576, 648; columns at 0, .., 1148; the whole frame
  {
    std::unique_ptr<yfv2_tile[]> tiles(new yfv2_tile[(size_t)n_tiles]);
    CHECK(yfv2_tile_plan(1000, 1500, 352, 352, 64, 64, 1, tiles.get(), n_tiles) == n_tiles, "%s", yfv2_last_error(nullptr));
    for (int k = 0; k < n_tiles; ++k)
      CHECK(tiles[k].frame == 0 && tiles[k].x0 >= 0 && tiles[k].y0 >= 0 && tiles[k].x0 + tiles[k].width <= 1500 && tiles[k].y0 + tiles[k].height <= 1000, "tile %d", k);
    CHECK(tiles[n_tiles - 1].width == 1500 && tiles[n_tiles - 1].height == 1000, "the whole-frame tile comes last");
    CHECK(yfv2_tile_plan(1000, 1500, 352, 352, 64, 64, 1, tiles.get(), n_tiles - 1) == YFV2_ERR_ARG, "cap below the count");
  }

  // towerp_kernel's lane table (the plan computes it once per tower step): on every map the kernel takes - even, up to 22x22, not both
  // sides <= 11, at most 128 2x2 patches - every patch sits on exactly one (round, lane) and every other entry says "none"
  int n_maps = 0;
  for (int H = 1; H <= 24; ++H)
    for (int W = 1; W <= 24; ++W) {
      const int patches = ((H + 1) / 2) * ((W + 1) / 2);
      const bool takes = !(H & 1) && !(W & 1) && H <= 22 && W <= 22 && (H > 11 || W > 11) && patches <= 128;
      CHECK(yfv2_towerp_map(H, W) == takes, "yfv2_towerp_map(%d, %d)", H, W);
      if (!takes) continue;
      ++n_maps;
      unsigned char tbl[128];
      std::memset(tbl, 0, sizeof(tbl));
      towerp_lane_patches(H, W, tbl);
      int seen[128] = {}, none = 0;
      for (int i = 0; i < 128; ++i) {
        if (tbl[i] == 255) { ++none; continue; }
        CHECK(tbl[i] < patches, "%dx%d: entry %d = %d of %d patches", H, W, i, tbl[i], patches);
        ++seen[tbl[i]];
      }
      for (int pid = 0; pid < patches; ++pid) CHECK(seen[pid] == 1, "%dx%d: patch %d occurs %d times", H, W, pid, seen[pid]);
      CHECK(none == 128 - patches, "%dx%d: %d empty entries", H, W, none);
    }
  CHECK(n_maps == 96, "%d maps", n_maps);

  // the row launches' LDS and width limits (yfv2_debug_rows): every kind at the ends of its argument ranges - the arithmetic stays
  // inside int - and the widest frame it admits fits a CU's LDS
  for (int kind = 0; kind < 5; ++kind)
    for (int yuv = 0; yuv < 2; ++yuv)
      for (int W : {1, 4, 352, 4096, 1 << 20}) {
        int64_t lds = -1;
        int32_t limit = -1;
        for (int w : {1, 1920, 1 << 26}) CHECK(yfv2_debug_rows(kind, yuv, w, W, &lds, &limit) == YFV2_OK && lds > 0, "debug_rows(%d, %d, %d, %d)", kind, yuv, w, W);
        if (W > 4096) continue;
        CHECK(limit >= 1 && yfv2_debug_rows(kind, yuv, limit, W, &lds, nullptr) == YFV2_OK && lds <= 160 * 1024, "debug_rows limit (%d, %d, %d)", kind, yuv, W);
      }
  CHECK(yfv2_debug_rows(5, 0, 8, 8, nullptr, nullptr) == YFV2_ERR_ARG && yfv2_debug_rows(0, 0, 0, 8, nullptr, nullptr) == YFV2_ERR_ARG, "debug_rows arguments");

  // the null-handle path of every entry point that takes a handle: a code (or 0 / -1 where the return value is a count), no access
  const yfv2_handle h = nullptr;
  yfv2_destroy(h);
  CHECK(yfv2_last_error(h) != nullptr, "last_error");
  CHECK(yfv2_load_weights(h, nullptr, 0) == YFV2_ERR_ARG, "load_weights");
  CHECK(yfv2_set_anchors(h, nullptr) == YFV2_ERR_ARG, "set_anchors");
  CHECK(yfv2_forward(h, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "forward");
  CHECK(yfv2_forward_u8(h, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "forward_u8");
  CHECK(yfv2_nonfinite(h, nullptr, nullptr) == YFV2_ERR_ARG && yfv2_nonfinite_peek(h, nullptr) == YFV2_ERR_ARG, "nonfinite");
  CHECK(yfv2_decode(h, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "decode");
  CHECK(yfv2_nms(h, nullptr, 1, 0.3f, 0.4, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "nms");
  CHECK(yfv2_detect(h, nullptr, 1, 0.3f, 0.4, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "detect");
  CHECK(yfv2_detect_u8(h, nullptr, 1, 0.3f, 0.4, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "detect_u8");
  CHECK(yfv2_debug_post(h, nullptr, 1, 0.3f, 0.4, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "debug_post");
  CHECK(yfv2_resize_u8(h, nullptr, 1, 1, 1, nullptr, nullptr) == YFV2_ERR_ARG, "resize_u8");
  CHECK(yfv2_resize_frames_u8(h, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "resize_frames_u8");
  CHECK(yfv2_detect_frames_u8(h, nullptr, 1, 0.3f, 0.4, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "detect_frames_u8");
  CHECK(yfv2_resize_frames_yuv(h, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "resize_frames_yuv");
  CHECK(yfv2_detect_frames_yuv(h, nullptr, 1, 0.3f, 0.4, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "detect_frames_yuv");
  CHECK(yfv2_merge_tiles(h, nullptr, nullptr, nullptr, 1, 1, 0.5, 0, 300, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "merge_tiles");
  CHECK(yfv2_detect_tiled_u8(h, nullptr, 1, nullptr, 1, 0.3f, 0.4, 0.5, 0, 300, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "detect_tiled_u8");
  CHECK(yfv2_detect_tiled_yuv(h, nullptr, 1, nullptr, 1, 0.3f, 0.4, 0.5, 0, 300, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "detect_tiled_yuv");
  CHECK(yfv2_batch_statistics(h, nullptr, nullptr, 1, nullptr, 0, 0.5f, nullptr, nullptr) == YFV2_ERR_ARG, "batch_statistics");
  CHECK(yfv2_batch_statistics_async(h, nullptr, nullptr, 1, nullptr, 0, 0.5f, nullptr, nullptr) == YFV2_ERR_ARG, "batch_statistics_async");
  CHECK(yfv2_batch_statistics_overflow(h, nullptr, nullptr) == YFV2_ERR_ARG, "batch_statistics_overflow");
  CHECK(yfv2_batch_statistics_multi(h, nullptr, nullptr, 1, nullptr, 0, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "batch_statistics_multi");
  CHECK(yfv2_batch_statistics_multi_async(h, nullptr, nullptr, 1, nullptr, 0, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "batch_statistics_multi_async");
  CHECK(yfv2_loss(h, nullptr, 1, nullptr, 0, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "loss");
  CHECK(yfv2_anchor_kmeans(h, nullptr, 1, nullptr, 6, 10, nullptr, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "anchor_kmeans");
  CHECK(yfv2_debug_kmeans_group(h, 8) == YFV2_ERR_ARG, "debug_kmeans_group");
  CHECK(yfv2_ap_per_class(h, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == YFV2_ERR_ARG, "ap_per_class");
  CHECK(yfv2_ap_per_class_multi(h, nullptr, nullptr, nullptr, 0, nullptr, 0, 3, nullptr, nullptr) == YFV2_ERR_ARG, "ap_per_class_multi");
  CHECK(yfv2_train_bind(h, nullptr, 0, nullptr, 0) == YFV2_ERR_ARG, "train_bind");
  CHECK(yfv2_train_forward(h, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "train_forward");
  CHECK(yfv2_train_backward(h, nullptr, nullptr) == YFV2_ERR_STATE, "train_backward");
  CHECK(yfv2_sgd_step(h, nullptr, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 0, nullptr) == YFV2_ERR_ARG, "sgd_step");
  CHECK(yfv2_sgd_step_multi(h, nullptr, 0, 0.1f, 0.9f, 0.f, nullptr) == YFV2_ERR_ARG, "sgd_step_multi");
  CHECK(yfv2_num_rows(h) == 0 && yfv2_num_stages(h) == 0, "num_rows / num_stages");
  CHECK(yfv2_stage_info(h, 0, nullptr, 0, nullptr, nullptr, nullptr) == YFV2_ERR_ARG, "stage_info");
  CHECK(yfv2_stage_kernel(h, 0, nullptr, 0) == YFV2_ERR_ARG, "stage_kernel");
  CHECK(yfv2_profile_forward(h, nullptr, 1, nullptr, 1, nullptr, nullptr) == YFV2_ERR_ARG, "profile_forward");
  CHECK(yfv2_clock_probe_begin(h, 1, 1.f, 0, nullptr) == YFV2_ERR_ARG && yfv2_clock_probe_end(h, nullptr, nullptr) == YFV2_ERR_ARG, "clock_probe");
  CHECK(yfv2_debug_repeat_step(h, nullptr, 1, nullptr, 0, 1, nullptr) == YFV2_ERR_ARG, "debug_repeat_step");
  CHECK(yfv2_debug_activation(h, 0, 1, nullptr, 0) == YFV2_ERR_ARG, "debug_activation");
  CHECK(yfv2_debug_train_relu_output(h, "x", nullptr, 0) == -1, "debug_train_relu_output");
  CHECK(yfv2_debug_train_tensor(h, "x", 0, nullptr, 0) == -1, "debug_train_tensor");

  std::printf("host_san ok: %d checks\n", g_checks);
  return 0;
}
