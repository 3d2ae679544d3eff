"""Identity across frames: a per-stream IoU tracker whose state lives on the device (include/yfv2.h yfv2_track_update; DESIGN.md
4.18).  `Tracker` owns the state tensor and the rule's parameters; every update is one enqueue-only launch, and with fresh=True it
hands back exactly the rows whose track was confirmed in this frame, in the (dets, count) layout Engine.crop_detections takes:

    tr = Tracker(engine, streams=256)
    dets, idx, count = engine.detect_frames(frames, 0.3, 0.4)
    track_id, track_hits, fresh_dets, fresh_src, fresh_count = tr.update(dets, count, fresh=True)
    crops, *_ = engine.crop_detections(frames, fresh_dets, fresh_count, (128, 128))      # once per object, not once per frame

With motion=True (or a dict of std_pos, std_vel, std_meas) every track carries a constant-velocity Kalman filter per coordinate
(yfv2_track_update_motion): rows are matched against the box the filter predicts, so an object hidden for a few
frames keeps its id.

With two_pass=True (or a dict of high_conf, low_conf, match_thres_low, tracked_only) there are two association passes
(yfv2_track_update_two_pass): detect at a LOW threshold; rows with conf >= high_conf are matched first, the rows
below it are offered only to the tracks still unmatched and start no track, so an object whose score dips for a few frames keeps its
id and no spurious row becomes a track.  It combines with motion:

    tr = Tracker(engine, streams=256, two_pass=True, init_conf=0.6)
    dets, idx, count = engine.detect_frames(frames, 0.1, 0.4)                            # low_conf, iou
    track_id, track_hits, fresh_dets, fresh_src, fresh_count, track_pass = tr.update(dets, count, fresh=True, passes=True)

With appearance=True (or a dict of dim, prox_thres, app_thres, alpha) every track also keeps a unit-norm feature, a moving average of
the embeddings of the rows it matched, and update takes emb (B, R, dim), the second-stage network's output for every row's crop
(yfv2_track_update_appearance): where a row and a track overlap by more than prox_thres, the edge between them is
valued by the cosine of the two when that is above app_thres and above the IoU - an object that jumps, or whose neighbour's box
fits better, keeps its id.  It combines with motion and two_pass:

    tr = Tracker(engine, streams=256, motion=True, appearance=dict(dim=128))
    crops, *_ = engine.crop_tensors(frames, dets, count, (128, 64))                      # every row, every frame
    emb = reid(crops)                                                                    # the caller's network -> (B, R, 128) fp32
    track_id, track_hits, track_cos = tr.update(dets, count, emb=emb, cos=True)
"""
import ctypes as C

import torch

from . import _lib

HEADER_WORDS, SLOT_WORDS = 8, 10
MOTION_SLOT_WORDS, FILTER_WORD = 32, 10          # the motion form's slot; its filters: words 10..29, cx, cy, w, h as x, v, p00, p01, p11
MOTION_DEFAULTS = dict(std_pos=1.0 / 20, std_vel=1.0 / 160, std_meas=1.0 / 20)
TWO_PASS_DEFAULTS = dict(high_conf=0.5, low_conf=0.1, match_thres_low=0.5, tracked_only=True)
APPEARANCE_DEFAULTS = dict(dim=128, prox_thres=0.5, app_thres=0.75, alpha=0.9)
FEATURE_HEAD_WORDS = 4                           # a track's feature: n_feat, three zero words, then dim fp32
HEADER_FIELDS = ("issued", "live", "frames", "births", "deaths", "dropped")


class _Completed(dict):
    """what option() returns: handing it to option() again (Tracker.update does, on every call) costs nothing"""


def option(caller, name, value, defaults):
    """The rule of motion / two_pass / appearance, for every caller that takes one: None or False - the form is off, None; True or a
    dict with any of the defaults' keys - the completed dict, each value as the type of its default."""
    if value is None or value is False:
        return None
    if type(value) is _Completed:
        return value
    given = {} if value is True else dict(value)
    if given.keys() - defaults.keys():
        keys = list(defaults)
        raise ValueError("%s: %s takes %s and %s, not %s" % (caller, name, ", ".join(keys[:-1]), keys[-1], sorted(given.keys() - defaults.keys())))
    return _Completed((k, type(v)(given[k]) if k in given else v) for k, v in defaults.items())


def outputs(B, R, fresh=False, box=False, passes=False, cos=False):
    """What an update returns, in order: a list of (name, shape, dtype).  Allocation, the check of a caller's `out` and the pointers
    of the native call all read it by name; a new optional output is one line here."""
    i32, f32 = torch.int32, torch.float32
    out = [("track_id", (B, R), i32), ("track_hits", (B, R), i32)]
    if fresh:
        out += [("fresh_dets", (B, R, 6), f32), ("fresh_src", (B, R), i32), ("fresh_count", (B,), i32)]
    if box:
        out.append(("track_box", (B, R, 4), f32))
    if passes:
        out.append(("track_pass", (B, R), i32))
    if cos:
        out.append(("track_cos", (B, R), f32))
    return out


# The native call of a form - the entry point that takes the LAST of motion, second, appearance that is given - and what it takes
# between the rule and the three fresh outputs, by name (include/yfv2.h): the structs, emb and feat, and the outputs (None: absent).
_FRESH = ("fresh_dets", "fresh_src", "fresh_count")
_NATIVE = {
    None: ("yfv2_track_update", ("track_id", "track_hits")),
    "motion": ("yfv2_track_update_motion", ("motion", "track_id", "track_hits", "track_box")),
    "second": ("yfv2_track_update_two_pass", ("motion", "second", "track_id", "track_hits", "track_pass", "track_box")),
    "appearance": ("yfv2_track_update_appearance", ("motion", "second", "appearance", "emb", "feat", "track_id", "track_hits", "track_pass", "track_box",
                                                    "track_cos")),
}
_NATIVE = {form: (native, takes + _FRESH) for form, (native, takes) in _NATIVE.items()}


def update(engine, name, dets, count, streams, state, max_tracks, rule, motion=None, second=None, appearance=None, emb=None, feat=None, fresh=False,
           box=False, passes=False, cos=False, out=None):
    """The checks and the call of every form, on engine's handle, device and current stream (Engine.track_update* are this).  rule:
    (match_thres, class_aware, init_conf, max_misses, confirm_hits); motion: None or the three stds; second: None or the two-pass
    form's four values; appearance: None or the appearance form's four values, with emb and feat."""
    device = engine.device
    if (not torch.is_tensor(dets) or dets.dim() != 3 or dets.shape[2] != 6 or dets.dtype != torch.float32 or dets.device != device
            or not dets.is_contiguous()):
        raise ValueError(name + ": dets must be contiguous fp32 (B,R,6) on %s" % (device,))
    B, R = int(dets.shape[0]), int(dets.shape[1])
    if not torch.is_tensor(count) or tuple(count.shape) != (B,) or count.dtype != torch.int32 or count.device != device or not count.is_contiguous():
        raise ValueError(name + ": count must be contiguous int32 (%d,) on %s" % (B, device))
    streams = [int(s) for s in streams]
    if len(streams) != B:
        raise ValueError(name + ": %d streams for %d frames" % (len(streams), B))
    max_tracks = int(max_tracks)
    if not 1 <= max_tracks <= 1024:
        raise ValueError(name + ": max_tracks must be in 1..1024")
    words = HEADER_WORDS + (SLOT_WORDS if motion is None else MOTION_SLOT_WORDS) * max_tracks
    if (not torch.is_tensor(state) or state.dim() != 2 or state.shape[1] != words or state.dtype != torch.int32 or state.device != device
            or not state.is_contiguous()):
        raise ValueError(name + ": state must be contiguous int32 (S,%d) on %s" % (words, device))
    S = int(state.shape[0])
    if appearance is not None:
        D = appearance["dim"]
        if (not torch.is_tensor(emb) or tuple(emb.shape) != (B, R, D) or emb.dtype != torch.float32 or emb.device != device
                or not emb.is_contiguous()):
            raise ValueError(name + ": emb must be contiguous fp32 (%d,%d,%d) on %s" % (B, R, D, device))
        if (not torch.is_tensor(feat) or tuple(feat.shape) != (S, max_tracks * (FEATURE_HEAD_WORDS + D)) or feat.dtype != torch.int32
                or feat.device != device or not feat.is_contiguous()):
            raise ValueError(name + ": feat must be contiguous int32 (%d,%d) on %s" % (S, max_tracks * (FEATURE_HEAD_WORDS + D), device))
    desc = outputs(B, R, fresh, box, passes, cos)
    if out is None:
        out = tuple(torch.empty(sh, device=device, dtype=dt) for _, sh, dt in desc)
    else:
        if len(out) != len(desc):
            raise ValueError(name + ": out must hold %d tensors" % len(desc))
        for t, (_, sh, dt) in zip(out, desc):
            if not torch.is_tensor(t) or tuple(t.shape) != sh or t.dtype != dt or t.device != device or not t.is_contiguous():
                raise ValueError(name + ": out must be contiguous tensors of shapes %s on %s" % (tuple(sh for _, sh, _ in desc), device))
    arg = {key: t.data_ptr() for (key, _, _), t in zip(desc, out)}      # the prototypes (_lib.py) take addresses as ints
    match_thres, class_aware, init_conf, max_misses, confirm_hits = rule
    ru = _lib.TrackRule()
    ru.max_tracks, ru.match_thres, ru.class_aware = max_tracks, float(match_thres), 1 if class_aware else 0
    ru.init_conf, ru.max_misses, ru.confirm_hits = float(init_conf), int(max_misses), int(confirm_hits)
    if motion is not None:
        mo = _lib.TrackMotion(float(motion["std_pos"]), float(motion["std_vel"]), float(motion["std_meas"]))
        arg["motion"] = C.byref(mo)
    if second is not None:
        se = _lib.TrackSecond(float(second["high_conf"]), float(second["low_conf"]), float(second["match_thres_low"]), 1 if second["tracked_only"] else 0)
        arg["second"] = C.byref(se)
    if appearance is not None:
        ap = _lib.TrackAppearance(D, float(appearance["prox_thres"]), float(appearance["app_thres"]), float(appearance["alpha"]))
        arg["appearance"], arg["emb"], arg["feat"] = C.byref(ap), emb.data_ptr(), feat.data_ptr()
    native, takes = _NATIVE["appearance" if appearance is not None else "second" if second is not None else "motion" if motion is not None else None]
    _lib.check(getattr(_lib.lib(), native)(engine._h, dets.data_ptr(), count.data_ptr(), R, B, (C.c_int32 * max(B, 1))(*streams), state.data_ptr(), S, C.byref(ru),
                                           *map(arg.get, takes), torch.cuda.current_stream(device).cuda_stream), engine._h)
    return out


class Tracker:
    def __init__(self, engine, streams, max_tracks=64, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30, confirm_hits=3, motion=None,
                 two_pass=None, appearance=None):
        """engine: the Engine whose device and stream the updates run on; streams: S, the number of video streams; max_tracks:
        slots per stream (1..1024).  An edge between a row and a track needs IoU > match_thres (and equal classes if class_aware);
        an unmatched row with conf >= init_conf starts a track; a track dies at its (max_misses + 1)-th consecutive miss; a row is
        fresh in the frame in which its track's hits reach confirm_hits.  motion: None - the IoU is taken with the track's last box;
        True or a dict with any of std_pos, std_vel, std_meas - with the box its filter predicts.  two_pass: None - one association
        pass over every row; True or a dict with any of high_conf, low_conf, match_thres_low, tracked_only - rows with conf >=
        high_conf first, then the rows down to low_conf against the tracks still unmatched (tracked_only: those matched in their
        last frame) with IoU > match_thres_low; only a row with conf >= high_conf starts a track.  appearance: None - the IoU
        alone; True or a dict with any of dim, prox_thres, app_thres, alpha - update takes the rows' embeddings (B, R, dim), the tracker
        owns the features (self.feat), and a first-pass edge with IoU > prox_thres is valued by the cosine of the row's embedding and
        the track's feature when that is > app_thres and above the IoU; alpha is the feature's momentum.  The rule, bit for bit:
        include/yfv2.h."""
        self.engine = engine
        self.streams, self.max_tracks = int(streams), int(max_tracks)
        if self.streams < 1 or not 1 <= self.max_tracks <= 1024:
            raise ValueError("Tracker: streams must be >= 1 and max_tracks in 1..1024")
        self.rule = dict(match_thres=float(match_thres), class_aware=bool(class_aware), init_conf=float(init_conf), max_misses=int(max_misses),
                         confirm_hits=int(confirm_hits))
        self.motion = option("Tracker", "motion", motion, MOTION_DEFAULTS)
        self.two_pass = option("Tracker", "two_pass", two_pass, TWO_PASS_DEFAULTS)
        self.appearance = option("Tracker", "appearance", appearance, APPEARANCE_DEFAULTS)
        if self.appearance is not None and (not 16 <= self.appearance["dim"] <= 2048 or self.appearance["dim"] % 16):
            raise ValueError("Tracker: appearance dim must be a multiple of 16 in 16..2048")
        self.slot_words = SLOT_WORDS if self.motion is None else MOTION_SLOT_WORDS
        self.state = torch.zeros((self.streams, HEADER_WORDS + self.slot_words * self.max_tracks), dtype=torch.int32, device=engine.device)
        self.feat = None
        if self.appearance is not None:
            self.feat_words = FEATURE_HEAD_WORDS + self.appearance["dim"]
            self.feat = torch.zeros((self.streams, self.feat_words * self.max_tracks), dtype=torch.int32, device=engine.device)

    def update(self, dets, count, streams=None, fresh=False, out=None, box=False, passes=False, emb=None, cos=False):
        """dets (B, R, 6) fp32 / count (B) int32 on the device; streams: the stream of each frame, B distinct indices (None: frame b
        is stream b).  Returns (track_id, track_hits) and, with fresh=True, (.., fresh_dets, fresh_src, fresh_count); with box=True
        (the motion form only) track_box (B, R, 4), the filtered corners of each row's track, comes after them; with passes=True (a
        two-pass tracker only) track_pass (B, R) int32 - 1: matched in the first pass or born, 2: matched in the second - comes after
        those.  emb (B, R, dim) fp32: the rows' embeddings - required by a tracker with appearance, refused by one without; with
        cos=True (such a tracker only) track_cos (B, R) fp32, the cosine of each matched row with its track's feature, comes last."""
        if streams is None:
            streams = range(int(dets.shape[0]))
        if box and self.motion is None:
            raise ValueError("Tracker.update: box=True needs a tracker with a motion model")
        if passes and self.two_pass is None:
            raise ValueError("Tracker.update: passes=True needs a tracker with two_pass")
        if self.appearance is None:
            if emb is not None or cos:
                raise ValueError("Tracker.update: emb and cos=True need a tracker with appearance")
        else:
            if emb is None:
                raise ValueError("Tracker.update: a tracker with appearance needs emb, the rows' embeddings")
            return self.engine.track_update_appearance(dets, count, emb, streams, self.state, self.feat, self.max_tracks, motion=self.motion,
                                                       two_pass=self.two_pass, fresh=fresh, box=box, passes=passes, cos=cos, out=out, **self.rule,
                                                       **self.appearance)
        if self.two_pass is not None:
            return self.engine.track_update_two_pass(dets, count, streams, self.state, self.max_tracks, motion=self.motion, fresh=fresh, box=box,
                                                     passes=passes, out=out, **self.rule, **self.two_pass)
        if self.motion is None:
            return self.engine.track_update(dets, count, streams, self.state, self.max_tracks, fresh=fresh, out=out, **self.rule)
        return self.engine.track_update_motion(dets, count, streams, self.state, self.max_tracks, fresh=fresh, box=box, out=out, **self.rule, **self.motion)

    def _slots(self, stream):
        return self.state[int(stream), HEADER_WORDS:].view(self.max_tracks, self.slot_words)

    def tracks(self, stream):
        """The live tracks of a stream, in slot order: a dict of tensors box (n, 4), conf (n), cls (n) fp32 and id, hits, misses, age
        (n) int32, gathered from the state (this reads the device: it waits for the updates enqueued so far).  With a motion model
        also pred (n, 4), the corners of the current filter state, and vel (n, 4), the velocities of cx, cy, w, h per update."""
        slots = self._slots(stream)
        live = slots[slots[:, 6] != 0]
        fl = live[:, :6].contiguous().view(torch.float32)
        out = {"box": fl[:, :4], "conf": fl[:, 4], "cls": fl[:, 5], "id": live[:, 6], "hits": live[:, 7], "misses": live[:, 8], "age": live[:, 9]}
        if self.motion is not None:
            f = live[:, FILTER_WORD:FILTER_WORD + 20].contiguous().view(torch.float32).view(-1, 4, 5)
            x, half = f[:, :, 0], f[:, 2:, 0] * 0.5
            out["pred"] = torch.cat([x[:, :2] - half, x[:, :2] + half], dim=1)
            out["vel"] = f[:, :, 1].contiguous()
        return out

    def features(self, stream):
        """The features of a stream's live tracks, in slot order like tracks(): a dict of n_feat (n) int32, the embeddings each has
        absorbed (0: none yet), and f (n, dim) fp32, the unit-norm features (a tracker with appearance only; waits for the device)."""
        if self.appearance is None:
            raise ValueError("Tracker.features: the tracker has no appearance")
        live = self._slots(stream)[:, 6] != 0
        words = self.feat[int(stream)].view(self.max_tracks, self.feat_words)[live]
        return {"n_feat": words[:, 0], "f": words[:, FEATURE_HEAD_WORDS:].contiguous().view(torch.float32)}

    def header(self, stream):
        """The stream's counters as a dict of ints: issued, live, frames, births, deaths, dropped and, on a two-pass tracker, second,
        the matches made in the second pass; on a tracker with appearance also by_appearance, the first-pass matches whose edge
        was valued by the cosine (waits for the device)."""
        words = [int(v) for v in self.state[int(stream), :HEADER_WORDS].tolist()]
        out = dict(zip(HEADER_FIELDS, words))
        if self.two_pass is not None:
            out["second"] = words[6]
        if self.appearance is not None:
            out["by_appearance"] = words[7]
        return out

    def reset(self, stream=None):
        """Forget every track of one stream, or of all of them (ids start again at 1)."""
        if stream is None:
            self.state.zero_()
        else:
            self.state[int(stream)].zero_()
        if self.feat is not None:
            (self.feat if stream is None else self.feat[int(stream)]).zero_()
