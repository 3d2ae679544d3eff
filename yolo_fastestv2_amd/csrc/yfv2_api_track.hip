// yfv2_api_track.hip - host side of libyfv2.so, the entry points of the per-stream tracker behind the detect calls (DESIGN.md 4.18,
// its motion form 4.19, its two-pass form 4.20, its appearance form 4.22): the sizes of its buffers and the four yfv2_track_update*
// calls, which are one routine.  The handle and the shared plumbing: yfv2_ctx.h.  The kernel, its one launcher and the host-only
// arithmetic entry points (yfv2_track_iou, _cosine, _feature_step, _filter_step, _birth, which call the kernel's own functions under
// that unit's flags): yfv2_track.hip.  The limits checked here are written once, beside the TRACK_* constants (yfv2_internal.h).
#include <algorithm>
#include <cmath>

#include "yfv2_ctx.h"

extern "C" {

int64_t yfv2_track_state_words(int32_t max_tracks) {
  if (!yfv2_track_tracks_ok(max_tracks)) return fail(nullptr, YFV2_ERR_ARG, "yfv2_track_state_words: max_tracks must be in 1.." + std::to_string(TRACK_MAX_M));
  return (int64_t)TRACK_HEADER + (int64_t)TRACK_SLOT * max_tracks;
}

int64_t yfv2_track_motion_state_words(int32_t max_tracks) {
  if (!yfv2_track_tracks_ok(max_tracks)) return fail(nullptr, YFV2_ERR_ARG, "yfv2_track_motion_state_words: max_tracks must be in 1.." + std::to_string(TRACK_MAX_M));
  return (int64_t)TRACK_HEADER + (int64_t)TRACK_SLOT_MOTION * max_tracks;
}

int64_t yfv2_track_feature_words(int32_t max_tracks, int32_t D) {
  if (!yfv2_track_tracks_ok(max_tracks)) return fail(nullptr, YFV2_ERR_ARG, "yfv2_track_feature_words: max_tracks must be in 1.." + std::to_string(TRACK_MAX_M));
  if (!yfv2_track_dim_ok(D)) return fail(nullptr, YFV2_ERR_ARG, "yfv2_track_feature_words: D must be a multiple of 16 in 16..2048");
  return (int64_t)max_tracks * (TRACK_FEAT_HEAD + D);
}

}  // extern "C"

// One update as its entry point received it.  An entry point names what its signature has; the rest stays null.  need_*: the
// signature REQUIRES that pointer (NULL is an error there, not another form).  The form of the update is what was given:
// motion - the table has 32-word slots; second - two association passes; appearance (with emb and feat) - the cosine joins the IoU.
struct TrackCall {
  const char* name;
  yfv2_handle h;
  const float* dets;
  const int32_t* count;
  int32_t R, B;
  const int32_t* stream_of;
  int32_t* state;
  int32_t S;
  const yfv2_track_rule* rule;
  int32_t* track_id;
  int32_t* track_hits;
  void* stream;
  bool need_motion = false, need_second = false, need_appearance = false;
  const yfv2_track_motion* motion = nullptr;
  const yfv2_track_second* second = nullptr;
  const yfv2_track_appearance* appearance = nullptr;
  const float* emb = nullptr;
  int32_t* feat = nullptr;
  int32_t* track_pass = nullptr;
  float* track_box = nullptr;
  float* track_cos = nullptr;
  float* fresh_dets = nullptr;
  int32_t* fresh_src = nullptr;
  int32_t* fresh_count = nullptr;
};

// Every check first; then one launch per TRACK_CHUNK frames (the streams of a launch travel in its arguments: no table, no copy,
// no workspace).  The frames of a call are distinct streams, so the launches share nothing.
static int track_update(const TrackCall& c) {
  yfv2_handle h = c.h;
  const std::string w_ = c.name;
  if (!h) return fail(nullptr, YFV2_ERR_ARG, "null handle");
  if (!c.dets || !c.count || !c.stream_of || !c.state || !c.rule || !c.track_id || (c.need_motion && !c.motion) || (c.need_second && !c.second) ||
      (c.need_appearance && (!c.appearance || !c.emb || !c.feat)))
    return fail(h, YFV2_ERR_ARG, w_ + ": null pointer");
  const TrackForm form{c.motion != nullptr, c.second != nullptr, c.appearance != nullptr};
  const int given = (c.fresh_dets != nullptr) + (c.fresh_src != nullptr) + (c.fresh_count != nullptr);
  if (given != 0 && given != 3) return fail(h, YFV2_ERR_ARG, w_ + ": fresh_dets, fresh_src and fresh_count must all be given or all be NULL");
  const int32_t B = c.B, S = c.S, R = c.R;
  if (B < 1) return fail(h, YFV2_ERR_ARG, w_ + ": B < 1");
  if (S < 1) return fail(h, YFV2_ERR_ARG, w_ + ": S < 1");
  if (R < 1 || R > TRACK_MAX_R) return fail(h, YFV2_ERR_ARG, w_ + ": R must be in 1.." + std::to_string(TRACK_MAX_R));
  const yfv2_track_rule& q = *c.rule;
  if (!yfv2_track_tracks_ok(q.max_tracks)) return fail(h, YFV2_ERR_ARG, w_ + ": max_tracks must be in 1.." + std::to_string(TRACK_MAX_M));
  if (!std::isfinite(q.match_thres) || q.match_thres < 0.0) return fail(h, YFV2_ERR_ARG, w_ + ": match_thres must be a finite number >= 0");
  if (std::isnan(q.init_conf)) return fail(h, YFV2_ERR_ARG, w_ + ": init_conf is not a number");
  if (q.max_misses < 0) return fail(h, YFV2_ERR_ARG, w_ + ": max_misses must be >= 0");
  if (q.confirm_hits < 1) return fail(h, YFV2_ERR_ARG, w_ + ": confirm_hits must be >= 1");
  if (form.motion && !yfv2_track_motion_ok(c.motion->std_pos, c.motion->std_vel, c.motion->std_meas))
    return fail(h, YFV2_ERR_ARG, w_ + ": std_pos, std_vel and std_meas must be finite and > 0");
  if (form.two_pass) {
    const yfv2_track_second& t = *c.second;
    if (std::isnan(t.high_conf) || std::isnan(t.low_conf)) return fail(h, YFV2_ERR_ARG, w_ + ": high_conf or low_conf is not a number");
    if (t.low_conf > t.high_conf) return fail(h, YFV2_ERR_ARG, w_ + ": low_conf must not exceed high_conf");
    if (!std::isfinite(t.match_thres_low) || t.match_thres_low < 0.0) return fail(h, YFV2_ERR_ARG, w_ + ": match_thres_low must be a finite number >= 0");
  }
  // an output of a form that was not asked for (the two-pass and the appearance entry points: motion and second are optional there)
  if (c.track_box && !form.motion) return fail(h, YFV2_ERR_ARG, w_ + ": track_box needs motion");
  if (c.track_pass && !form.two_pass) return fail(h, YFV2_ERR_ARG, w_ + ": track_pass needs second");
  if (form.appearance) {
    const yfv2_track_appearance& p = *c.appearance;
    if ((reinterpret_cast<uintptr_t>(c.emb) & 15) != 0) return fail(h, YFV2_ERR_ARG, w_ + ": emb must be 16-byte aligned");
    if (!yfv2_track_dim_ok(p.dim)) return fail(h, YFV2_ERR_ARG, w_ + ": dim must be a multiple of 16 in 16..2048");
    if (!std::isfinite(p.prox_thres) || p.prox_thres < 0.0) return fail(h, YFV2_ERR_ARG, w_ + ": prox_thres must be a finite number >= 0");
    if (std::isnan(p.app_thres)) return fail(h, YFV2_ERR_ARG, w_ + ": app_thres is not a number");
    if (!std::isfinite(p.alpha) || p.alpha < 0.0f || p.alpha > 1.0f) return fail(h, YFV2_ERR_ARG, w_ + ": alpha must be in [0, 1]");
    if (yfv2_track_lds_bytes(true, R, q.max_tracks) > TRACK_APP_LDS_MAX)
      return fail(h, YFV2_ERR_ARG, w_ + ": 28 R + 52 max_tracks must not exceed " + std::to_string(TRACK_APP_LDS_MAX) + " bytes of LDS");
  }
  std::vector<int32_t> sorted(c.stream_of, c.stream_of + B);
  std::sort(sorted.begin(), sorted.end());
  if (sorted.front() < 0 || sorted.back() >= S)
    return fail(h, YFV2_ERR_ARG, w_ + ": stream " + std::to_string(sorted.front() < 0 ? sorted.front() : sorted.back()) + " outside [0, S)");
  for (int32_t b = 1; b < B; ++b)
    if (sorted[b] == sorted[b - 1]) return fail(h, YFV2_ERR_ARG, w_ + ": stream " + std::to_string(sorted[b]) + " named twice (one frame per stream and call)");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(c.stream);
  TrackAppArgs a{};                        // the launch of a form takes the part that is its kernel's argument type
  a.R = R; a.M = q.max_tracks; a.state = c.state; a.thres = q.match_thres; a.class_aware = q.class_aware; a.init_conf = q.init_conf;
  a.max_misses = q.max_misses; a.confirm_hits = q.confirm_hits;
  if (form.motion) a.motion = TrackMotion{c.motion->std_pos, c.motion->std_vel, c.motion->std_meas};
  if (form.two_pass) { a.high_conf = c.second->high_conf; a.low_conf = c.second->low_conf; a.thres_low = c.second->match_thres_low; a.tracked_only = c.second->tracked_only; }
  if (form.appearance) {
    a.feat = c.feat; a.D = c.appearance->dim; a.prox = c.appearance->prox_thres; a.app = c.appearance->app_thres;
    a.alpha = c.appearance->alpha; a.beta = 1.0f - a.alpha;
  }
  for (int32_t b0 = 0; b0 < B; b0 += TRACK_CHUNK) {
    const int frames = std::min<int32_t>(TRACK_CHUNK, B - b0);
    const size_t row0 = (size_t)b0 * R;
    if (form.appearance) { a.emb = c.emb + row0 * (size_t)a.D; a.track_cos = c.track_cos ? c.track_cos + row0 : nullptr; }
    a.dets = c.dets + row0 * 6; a.count = c.count + b0; a.track_id = c.track_id + row0; a.track_hits = c.track_hits ? c.track_hits + row0 : nullptr;
    a.fresh_dets = c.fresh_dets ? c.fresh_dets + row0 * 6 : nullptr; a.fresh_src = c.fresh_src ? c.fresh_src + row0 : nullptr;
    a.fresh_count = c.fresh_count ? c.fresh_count + b0 : nullptr;
    a.track_box = c.track_box ? c.track_box + row0 * 4 : nullptr;
    a.track_pass = c.track_pass ? c.track_pass + row0 : nullptr;
    std::copy(c.stream_of + b0, c.stream_of + b0 + frames, a.stream_of);
    yfv2_launch_track(a, form, frames, s);
  }
  HIP_TRY(h, hipGetLastError());
  return YFV2_OK;
}

extern "C" {

int yfv2_track_update(yfv2_handle h, const float* dets, const int32_t* count, int32_t R, int32_t B, const int32_t* stream_of, int32_t* state, int32_t S,
                      const yfv2_track_rule* rule, int32_t* track_id, int32_t* track_hits, float* fresh_dets, int32_t* fresh_src, int32_t* fresh_count,
                      void* stream) {
  return track_update({.name = "yfv2_track_update", .h = h, .dets = dets, .count = count, .R = R, .B = B, .stream_of = stream_of, .state = state, .S = S,
                       .rule = rule, .track_id = track_id, .track_hits = track_hits, .stream = stream, .fresh_dets = fresh_dets, .fresh_src = fresh_src,
                       .fresh_count = fresh_count});
}

int yfv2_track_update_motion(yfv2_handle h, const float* dets, const int32_t* count, int32_t R, int32_t B, const int32_t* stream_of, int32_t* state,
                             int32_t S, const yfv2_track_rule* rule, const yfv2_track_motion* motion, int32_t* track_id, int32_t* track_hits,
                             float* track_box, float* fresh_dets, int32_t* fresh_src, int32_t* fresh_count, void* stream) {
  return track_update({.name = "yfv2_track_update_motion", .h = h, .dets = dets, .count = count, .R = R, .B = B, .stream_of = stream_of, .state = state,
                       .S = S, .rule = rule, .track_id = track_id, .track_hits = track_hits, .stream = stream, .need_motion = true, .motion = motion,
                       .track_box = track_box, .fresh_dets = fresh_dets, .fresh_src = fresh_src, .fresh_count = fresh_count});
}

int yfv2_track_update_two_pass(yfv2_handle h, const float* dets, const int32_t* count, int32_t R, int32_t B, const int32_t* stream_of, int32_t* state,
                               int32_t S, const yfv2_track_rule* rule, const yfv2_track_motion* motion, const yfv2_track_second* second, int32_t* track_id,
                               int32_t* track_hits, int32_t* track_pass, float* track_box, float* fresh_dets, int32_t* fresh_src, int32_t* fresh_count,
                               void* stream) {
  return track_update({.name = "yfv2_track_update_two_pass", .h = h, .dets = dets, .count = count, .R = R, .B = B, .stream_of = stream_of, .state = state,
                       .S = S, .rule = rule, .track_id = track_id, .track_hits = track_hits, .stream = stream, .need_second = true, .motion = motion,
                       .second = second, .track_pass = track_pass, .track_box = track_box, .fresh_dets = fresh_dets, .fresh_src = fresh_src,
                       .fresh_count = fresh_count});
}

int yfv2_track_update_appearance(yfv2_handle h, const float* dets, const int32_t* count, int32_t R, int32_t B, const int32_t* stream_of, int32_t* state,
                                 int32_t S, const yfv2_track_rule* rule, const yfv2_track_motion* motion, const yfv2_track_second* second,
                                 const yfv2_track_appearance* appearance, const float* emb, int32_t* feat, int32_t* track_id, int32_t* track_hits,
                                 int32_t* track_pass, float* track_box, float* track_cos, float* fresh_dets, int32_t* fresh_src, int32_t* fresh_count,
                                 void* stream) {
  return track_update({.name = "yfv2_track_update_appearance", .h = h, .dets = dets, .count = count, .R = R, .B = B, .stream_of = stream_of, .state = state,
                       .S = S, .rule = rule, .track_id = track_id, .track_hits = track_hits, .stream = stream, .need_appearance = true, .motion = motion,
                       .second = second, .appearance = appearance, .emb = emb, .feat = feat, .track_pass = track_pass, .track_box = track_box,
                       .track_cos = track_cos, .fresh_dets = fresh_dets, .fresh_src = fresh_src, .fresh_count = fresh_count});
}

}  // extern "C"
