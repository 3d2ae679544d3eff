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
import torch

HEADER_WORDS, SLOT_WORDS = 8, 10
MOTION_SLOT_WORDS, FILTER_WORD = 32, 10          # the motion form's slot; its filters: words 10..29, cx, cy, w, h as x, v, p00, p01, p11
MOTION_DEFAULTS = dict(std_pos=1.0 / 20, std_vel=1.0 / 160, std_meas=1.0 / 20)
TWO_PASS_DEFAULTS = dict(high_conf=0.5, low_conf=0.1, match_thres_low=0.5, tracked_only=True)
APPEARANCE_DEFAULTS = dict(dim=128, prox_thres=0.5, app_thres=0.75, alpha=0.9)
FEATURE_HEAD_WORDS = 4                           # a track's feature: n_feat, three zero words, then dim fp32
HEADER_FIELDS = ("issued", "live", "frames", "births", "deaths", "dropped")


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
        if motion is None or motion is False:
            self.motion = None
        else:
            given = {} if motion is True else dict(motion)
            if set(given) - set(MOTION_DEFAULTS):
                raise ValueError("Tracker: motion takes std_pos, std_vel and std_meas, not %s" % sorted(set(given) - set(MOTION_DEFAULTS)))
            self.motion = {k: float(given.get(k, v)) for k, v in MOTION_DEFAULTS.items()}
        if two_pass is None or two_pass is False:
            self.two_pass = None
        else:
            given = {} if two_pass is True else dict(two_pass)
            if set(given) - set(TWO_PASS_DEFAULTS):
                raise ValueError("Tracker: two_pass takes high_conf, low_conf, match_thres_low and tracked_only, not %s"
                                 % sorted(set(given) - set(TWO_PASS_DEFAULTS)))
            self.two_pass = {k: type(v)(given.get(k, v)) for k, v in TWO_PASS_DEFAULTS.items()}
        if appearance is None or appearance is False:
            self.appearance = None
        else:
            given = {} if appearance is True else dict(appearance)
            if set(given) - set(APPEARANCE_DEFAULTS):
                raise ValueError("Tracker: appearance takes dim, prox_thres, app_thres and alpha, not %s" % sorted(set(given) - set(APPEARANCE_DEFAULTS)))
            self.appearance = {k: type(v)(given.get(k, v)) for k, v in APPEARANCE_DEFAULTS.items()}
            if not 16 <= self.appearance["dim"] <= 2048 or self.appearance["dim"] % 16:
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
