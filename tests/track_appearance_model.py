"""The numpy statement of the tracker's appearance form (include/yfv2.h "identity across frames, appearance association"; DESIGN.md
4.22; the library's functions of the cosine and of the feature update are behind yfv2_track_cosine and yfv2_track_feature_step).
Everything that is not appearance - the IoU, the valid rows, the walk and its parallel form, the filter, the rows' classes - is
track_model's, track_motion_model's and track_two_pass_model's, imported and not changed; this file restates the frame's order with
the places the appearance rule changes: the rows' norms, the value of a first-pass edge, track_cos, header word 7 and the features.

One function covers both layouts and both pass forms, as the one entry point does: motion=None is the plain 10-word slot, a dict the
32-word motion slot; second=None is one pass (every valid row is HIGH: track_two_pass_model.ONE_PASS, which the two-pass tests pin to
the one-pass forms), a dict two passes.  Every fp32 operation below is a numpy float32 operation of its own, in the order the header
writes it; dot16 is a loop over i on arrays."""
import numpy as np

import track_model as tm
import track_motion_model as mm
import track_two_pass_model as tp
from track_model import F32, HEADER, greedy, mutual_best  # noqa: F401  (the rule's shared parts)
from track_motion_model import canon

HEAD = 4                                                            # a feature slot's words in front of the D floats: n_feat, 0, 0, 0
DEFAULT = dict(dim=128, prox_thres=0.5, app_thres=0.75, alpha=0.9)


def appearance_of(appearance):
    a = dict(DEFAULT)
    a.update({} if appearance in (None, True) else appearance)
    return a


def feature_words(M, D):
    return M * (HEAD + D)


def dot16(a, b):
    """a (..., D), b (..., D) fp32, broadcast against each other, D a multiple of 16 -> (...) fp32: sixteen partial sums over i
    ascending, then the tree with strides 8, 4, 2, 1"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    D = a.shape[-1]
    assert D % 16 == 0 and b.shape[-1] == D
    a, b = a.reshape(a.shape[:-1] + (D // 16, 16)), b.reshape(b.shape[:-1] + (D // 16, 16))
    with np.errstate(all="ignore"):
        P = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (16,), F32)
        for i in range(D // 16):
            P = P + a[..., i, :] * b[..., i, :]
        for stride in (8, 4, 2, 1):
            P = P[..., :stride] + P[..., stride:2 * stride]
    assert P.dtype == F32
    return P[..., 0]


def norm(e):
    """e (..., D) -> (n (...) fp32 = sqrt(dot16(e, e)) with NaNs canonical, has (...) bool: n finite and > 0)"""
    with np.errstate(all="ignore"):
        n = canon(np.sqrt(dot16(e, e)))
        return n, np.isfinite(n) & (n > 0)


def cosine(e, f, n):
    """e (..., D), f (..., D), n (...) the norms of e -> dot16(e, f) / n, NaNs canonical"""
    with np.errstate(all="ignore"):
        return canon(dot16(e, f) / np.asarray(n, F32))


def feature_step(f, n_feat, e, alpha):
    """one track's feature f (D) with n_feat embeddings absorbed, the matched row's embedding e (D) -> (f', n_feat', skipped):
    skipped = the moving average had no norm, so the feature stayed"""
    f, e = np.asarray(f, F32), np.asarray(e, F32)
    n, has = norm(e)
    if not has:
        return f.copy(), int(n_feat), False
    with np.errstate(all="ignore"):
        if n_feat == 0:
            return (e / n).astype(F32), 1, False
        alpha = F32(alpha)
        beta = F32(1.0) - alpha
        g = alpha * f + beta * (e / n)
        m, ok = norm(g)
        if not ok:
            return f.copy(), int(n_feat), True
        return (g / m).astype(F32), int(n_feat) + 1, False


def edge_values(V, rows_has, rows_n, emb, feat_f, feat_n, app):
    """V (n, M) the IoUs -> (S (n, M) the first-pass edge values, C (n, M) the cosines, A (n, M) bool: the value is the cosine)"""
    C = cosine(emb[:, None, :], feat_f[None, :, :], rows_n[:, None])
    with np.errstate(all="ignore"):
        A = (rows_has[:, None] & (feat_n > 0)[None, :] & (V.astype(np.float64) > float(app["prox_thres"])) & np.isfinite(C)
             & (C.astype(np.float64) > float(app["app_thres"])) & (C > V))
    return np.where(A, C, V).astype(F32), C, A


def update_stream(st, ft, rows, emb, count, rule, app, second=None, motion=None, match=greedy, match_low=None, stats=None):
    """One frame of one stream.  st: the state of the layout, ft: (M * (4 + D)) int32 the features, both changed in place; rows
    (R, 6), emb (R, D) fp32; app: dict with dim, prox_thres, app_thres, alpha; second: None (one pass) or the two-pass dict.
    -> (track_id (R), track_hits (R), track_pass (R), track_box (R, 4), track_cos (R), fresh rows' indices)"""
    plain = motion is None
    two = second is not None
    second = tp.ONE_PASS if second is None else second
    match_low = match if match_low is None else match_low
    M, D = int(rule["max_tracks"]), int(app["dim"])
    SLOT = tm.SLOT if plain else mm.SLOT
    rows = np.ascontiguousarray(rows, F32).reshape(-1, 6)
    R = rows.shape[0]
    emb = np.ascontiguousarray(emb, F32).reshape(R, D)
    n = min(max(int(count), 0), R)
    head, slots = st[:HEADER], st[HEADER:].reshape(M, SLOT)
    fslots = ft.reshape(M, HEAD + D)
    feat_f = fslots[:, HEAD:].view(F32)                             # views: writes go to the features
    fl = slots[:, :6].view(F32)
    live = slots[:, 6] != 0
    misses0 = slots[:, 8].copy()
    if plain:
        ok = tm.valid_rows(rows[:n])
        offered, boxes = live, fl[:, :4].copy()
    else:
        filt = slots[:, mm.FILTER:mm.FILTER + 20].view(F32).reshape(M, 4, 5)
        pred = mm.predict(filt, mm.scales(filt), motion)            # 0 predict
        filt[live] = pred[live]
        with np.errstate(all="ignore"):
            blind = ~(np.isfinite(filt).all(axis=(1, 2)) & (filt[:, 2, mm.X] > 0) & (filt[:, 3, mm.X] > 0))
        z = mm.measure(rows[:n])
        ok = tm.valid_rows(rows[:n]) & np.isfinite(z).all(axis=1)
        offered, boxes = live & ~blind, mm.corners(filt)
    high, low = tp.classes(rows[:n], ok, second)                    # 1 valid, the classes, and the rows' norms
    rows_n, rows_has = norm(emb[:n])
    # 2 / 3 the first pass: the HIGH rows; an edge's value is the cosine where the pair qualifies, else the IoU
    V, E_iou = tm.edges(rows[:n], boxes, fl[:, 5], offered, rule["match_thres"], rule["class_aware"])
    S, C, A = edge_values(V, rows_has, rows_n, emb[:n], feat_f, fslots[:, 0].copy(), app)
    with np.errstate(all="ignore"):
        E = ok[:, None] & offered[None, :] & (S.astype(np.float64) > float(rule["match_thres"]))
        if rule["class_aware"]:
            E &= rows[:n, 5][:, None] == fl[:, 5][None, :]
    E &= high[:, None]
    slot_of_row, rounds1 = tp._run(match, S, E)
    slot_of_row = np.array(slot_of_row, np.int64)
    iou_alone, _ = tp._run(greedy, V, E_iou & high[:, None])        # what the walk would have done without appearance
    taken = np.zeros(M, bool)
    taken[slot_of_row[slot_of_row >= 0]] = True
    # 3b the second pass: the IoU alone
    cand = offered & ~taken
    if second["tracked_only"]:
        cand = cand & (misses0 == 0)
    _, E_any = tm.edges(rows[:n], boxes, fl[:, 5], offered, second["match_thres_low"], rule["class_aware"])
    E2 = E_any & low[:, None] & cand[None, :]
    second_slot, rounds2 = tp._run(match_low, V, E2)
    second_slot = np.array(second_slot, np.int64)
    pass_of_row = np.where(slot_of_row >= 0, 1, np.where(second_slot >= 0, 2, 0)).astype(np.int32)
    slot_of_row = np.where(slot_of_row >= 0, slot_of_row, second_slot)
    box = np.zeros((R, 4), F32)
    cos = np.zeros(R, F32)
    rs = np.nonzero(slot_of_row >= 0)[0]                            # 4 matched
    ss = slot_of_row[rs]
    by_app = int((A[rs, ss] & (pass_of_row[rs] == 1)).sum())
    if stats is not None:
        stats["by_appearance"] = stats.get("by_appearance", 0) + by_app
        stats["not_by_iou"] = stats.get("not_by_iou", 0) + int(((pass_of_row[:n] == 1) & (slot_of_row[:n] != np.array(iou_alone, np.int64))).sum())
        stats["matched_without"] = stats.get("matched_without", 0) + int((~rows_has[rs]).sum())
        stats["second"] = stats.get("second", 0) + int((pass_of_row == 2).sum())
        with np.errstate(all="ignore"):
            stats["gated"] = stats.get("gated", 0) + int(((ok & high & rows_has)[:, None] & offered[None, :] & (fslots[:, 0] > 0)[None, :]
                                                          & (V.astype(np.float64) > float(app["prox_thres"]))
                                                          & ((rows[:n, 5][:, None] == fl[:, 5][None, :]) | (not rule["class_aware"]))).sum())
        stats.setdefault("rounds", []).append((rounds1, rounds2))
    for r, s in zip(rs, ss):
        if rows_has[r] and fslots[s, 0] > 0:
            cos[r] = C[r, s]
        f, nf, skipped = feature_step(feat_f[s], int(fslots[s, 0]), emb[r], app["alpha"])
        feat_f[s] = f
        fslots[s, 0] = nf
        if stats is not None:
            stats["skipped"] = stats.get("skipped", 0) + int(skipped)
    if not plain and len(rs):
        filt[ss] = mm.update(filt[ss], z[rs], mm.scales(filt[ss]), motion)
        box[rs] = mm.corners(filt[ss])
    slots[ss, :6] = rows[rs].view(np.int32)
    slots[ss, 7] += 1; slots[ss, 8] = 0; slots[ss, 9] += 1
    unmatched = live.copy()                                         # 5 unmatched
    unmatched[ss] = False
    slots[unmatched, 8] += 1; slots[unmatched, 9] += 1
    dead = unmatched & (slots[:, 8] > int(rule["max_misses"]))
    slots[dead, :] = 0
    fslots[dead, :] = 0
    head[4] += int(dead.sum())
    free = [s for s in range(M) if slots[s, 6] == 0]
    k = 0
    for r in range(n):                                              # 6 births: HIGH rows only
        if slot_of_row[r] >= 0 or not high[r] or not rows[r, 4] >= F32(rule["init_conf"]):
            continue
        if k < len(free):
            s = free[k]
            k += 1
            head[0] += 1
            slots[s, :6] = rows[r].view(np.int32)
            slots[s, 6:10] = (head[0], 1, 0, 1)
            if not plain:
                filt[s] = mm.birth(rows[r, :4], motion)
                box[r] = mm.corners(filt[s])
            fslots[s, :] = 0
            if rows_has[r]:
                with np.errstate(all="ignore"):
                    feat_f[s] = emb[r] / rows_n[r]
                fslots[s, 0] = 1
            elif stats is not None:
                stats["born_without"] = stats.get("born_without", 0) + 1
            head[3] += 1
            slot_of_row[r] = s
            pass_of_row[r] = 1
        else:
            head[5] += 1
    head[2] += 1                                                    # 7 header
    head[1] = int((slots[:, 6] != 0).sum())
    head[6] += int((pass_of_row == 2).sum())
    head[7] += by_app
    tid, hits, tpass = np.zeros(R, np.int32), np.zeros(R, np.int32), np.zeros(R, np.int32)
    for r in range(n):
        if slot_of_row[r] >= 0:
            tid[r], hits[r], tpass[r] = slots[slot_of_row[r], 6], slots[slot_of_row[r], 7], pass_of_row[r]
    if not two:
        assert not (tpass == 2).any()
    return tid, hits, tpass, box, cos, np.nonzero(hits == int(rule["confirm_hits"]))[0].astype(np.int32)


class Model(tm.Model):
    """S streams of M slots in the appearance form: the state of the layout (motion) and the features; second=None is one pass.
    update returns track_cos too, track_pass (all 0 / 1 with one pass) and, with motion, track_box.  self.stats adds up, over every
    frame: by_appearance (first-pass matches whose edge was valued by the cosine: header word 7), not_by_iou (first-pass rows whose
    slot is not the one the walk over the IoUs alone gives them), matched_without (matched rows without appearance), born_without
    (births without appearance), skipped (feature updates whose moving average had no norm), second, gated (pairs whose cosine the
    first pass needed) and rounds."""

    def __init__(self, streams, appearance=None, second=None, motion=None, **rule):
        super().__init__(streams, **rule)
        self.app = appearance_of(appearance)
        self.D = int(self.app["dim"])
        self.second = None if second is None or second is False else tp.second_of(second)
        if motion is None or motion is False:
            self.motion = None
        else:
            self.motion = dict(mm.DEFAULT)
            self.motion.update({} if motion is True else motion)
            self.state = np.zeros((self.S, mm.state_words(self.M)), np.int32)
        self.feat = np.zeros((self.S, feature_words(self.M, self.D)), np.int32)
        self.stats = {}

    def update(self, dets, count, emb, streams=None, match=greedy, match_low=None):
        dets, emb = np.ascontiguousarray(dets, F32), np.ascontiguousarray(emb, F32)
        B, R = dets.shape[0], dets.shape[1]
        assert emb.shape == (B, R, self.D)
        streams = list(range(B)) if streams is None else [int(s) for s in streams]
        assert len(streams) == B and len(set(streams)) == B and all(0 <= s < self.S for s in streams)
        out = {"track_id": np.zeros((B, R), np.int32), "track_hits": np.zeros((B, R), np.int32), "track_pass": np.zeros((B, R), np.int32),
               "track_cos": np.zeros((B, R), F32), "fresh_dets": np.zeros((B, R, 6), F32), "fresh_src": np.zeros((B, R), np.int32),
               "fresh_count": np.zeros(B, np.int32)}
        if self.motion is not None:
            out["track_box"] = np.zeros((B, R, 4), F32)
        for b, s in enumerate(streams):
            tid, hits, tpass, box, cos, fresh = update_stream(self.state[s], self.feat[s], dets[b], emb[b], count[b], self.rule, self.app, self.second,
                                                              self.motion, match, match_low, self.stats)
            out["track_id"][b], out["track_hits"][b], out["track_pass"][b], out["track_cos"][b] = tid, hits, tpass, cos
            if self.motion is not None:
                out["track_box"][b] = box
            out["fresh_count"][b] = len(fresh)
            out["fresh_src"][b, :len(fresh)] = fresh
            out["fresh_dets"][b, :len(fresh)] = dets[b, fresh]
        return out

    def features(self, stream=0):
        """(n_feat (M) int32, f (M, D) fp32) views of the stream's features"""
        w = self.feat[stream].reshape(self.M, HEAD + self.D)
        return w[:, 0], w[:, HEAD:].view(F32)


# ---- the scenarios: inputs that do what they claim on the model alone (tests/test_track_appearance_host.py asserts it)
def unit(D, k):
    """the k-th basis vector of D floats"""
    e = np.zeros(D, F32)
    e[k] = 1.0
    return e


def jump_case(D=16, frames=8, R=2):
    """One 40 x 40 box of class 0 moving 30 px per frame - IoU with its last box 400 / 2800 = 0.143 - with a constant embedding.
    -> a list of (dets (1, R, 6), count (1), emb (1, R, D))"""
    out = []
    for t in range(frames):
        d, e = np.zeros((1, R, 6), F32), np.zeros((1, R, D), F32)
        x = F32(30.0 * t)
        d[0, 0] = (x, 0.0, x + F32(40.0), 40.0, 0.9, 0.0)
        e[0, 0] = unit(D, 3) * F32(2.5)                             # not normalised: the rule divides by its norm
        out.append((d, np.array([1], np.int32), e))
    return out


def neighbour_case(D=16, R=2, tie=False):
    """Two tracks 40 wide at x = 0 and x = 20 with orthogonal features, then one row at x = 8 (IoU 32 / 48 = 0.667 with the first,
    28 / 52 = 0.538 with the second) that carries the SECOND track's embedding.  tie: the second track is at x = 10 and the row
    sits exactly on the first track (IoU 1 with it, 30 / 50 = 0.6 with the second), still with the second's embedding (cosine 1):
    the stated limit - the maximum cannot tell the two apart, and the walk's order (row, then slot) gives the IoU pair.
    -> two (dets, count, emb)"""
    d0, e0 = np.zeros((1, R, 6), F32), np.zeros((1, R, D), F32)
    d0[0, 0] = (0.0, 0.0, 40.0, 40.0, 0.9, 0.0)
    x2 = F32(10.0 if tie else 20.0)
    d0[0, 1] = (x2, 0.0, x2 + F32(40.0), 40.0, 0.9, 0.0)
    e0[0, 0], e0[0, 1] = unit(D, 0), unit(D, 1)
    d1, e1 = np.zeros((1, R, 6), F32), np.zeros((1, R, D), F32)
    x = F32(0.0 if tie else 8.0)
    d1[0, 0] = (x, 0.0, x + F32(40.0), 40.0, 0.9, 0.0)
    e1[0, 0] = unit(D, 1)
    return [(d0, np.array([2], np.int32), e0), (d1, np.array([1], np.int32), e1)]


def flip_case(D=16, R=2):
    """One track at rest whose row comes back with the NEGATED embedding: with alpha = 0.5 the moving average is exactly zero, has
    no norm, and the feature stays (the match itself is the IoU's: the cosine is -1).  -> two (dets, count, emb)"""
    out = []
    for sign in (1.0, -1.0):
        d, e = np.zeros((1, R, 6), F32), np.zeros((1, R, D), F32)
        d[0, 0] = (0.0, 0.0, 40.0, 40.0, 0.9, 0.0)
        e[0, 0] = unit(D, 2) * F32(sign)
        out.append((d, np.array([1], np.int32), e))
    return out


# The random walks of the host and of the device tests: (R, M) -> D, and the generator's objects, noise, jump, the rule's
# max_misses and the seed.  LEAST: what the model's counters must show at every shape, layout and pass form before a device is
# asked.  At R = 1 there is one object: 60 stream-frames of at most one row each must give 20 matches by the cosine, so it leaps in
# nearly half of its frames, and the seed is one whose few rows without appearance include a matched one and a born one and whose counts show a 0, a negative
# one and one beyond R.
WALKS = {(1, 1): (16, 1, 0.15, 0.45, 1, 423), (65, 64): (64, 80, 0.15, 0.25, 2, 265), (300, 256): (128, 260, 0.15, 0.25, 2, 500),
         (1030, 40): (16, 1150, 0.15, 0.25, 2, 1230)}
LEAST = dict(by_appearance=20, not_by_iou=1, matched_without=1, deaths=1, born_without=1)
WALK_APP = dict(prox_thres=0.1, app_thres=0.75, alpha=0.9)


def walk_calls(R, M, motion, second, S=2, T=30, seed=None):
    """The walk of a shape run on the model: -> (model, [(dets, count, emb, streams, outputs, state after, feat after)], counters)"""
    D, objects, noise, jump, max_misses, seed0 = WALKS[(R, M)]
    rule = dict(max_tracks=M, match_thres=0.3, init_conf=0.3, max_misses=max_misses, confirm_hits=3)
    m = Model(S, appearance=dict(WALK_APP, dim=D), second=second, motion=motion, **rule)
    seq = walk_case(seed0 if seed is None else seed, S, T, R, M, D, objects, noise, jump)
    rng = np.random.default_rng(9)
    calls = []
    for d, c, e in seq:
        perm = rng.permutation(S)
        d, c, e = np.ascontiguousarray(d[perm]), np.ascontiguousarray(c[perm]), np.ascontiguousarray(e[perm])
        calls.append((d, c, e, perm.tolist(), m.update(d, c, e, perm.tolist()), m.state.copy(), m.feat.copy()))
    shown = dict(m.stats, deaths=int(m.state[:, 4].sum()), dropped=int(m.state[:, 5].sum()))
    shown.pop("rounds", None)
    return m, calls, shown


def walk_case(seed, S, T, R, M, D, objects=None, noise=0.15, jump=0.25, bad=0.05, dip_rate=0.2):
    """track_two_pass_model.walk_case's boxes, scores, dropouts and odd counts with an embedding per row: every object has a unit
    vector of its own, a row's embedding is that vector times a random scale plus noise; with chance `jump` per object and frame
    the object leaps by about its own size (an IoU below match_thres with its last box, above prox_thres 0.1); a share `bad` of
    the rows gets an all-zero or a NaN embedding.  (The generator is restated here, not imported: an embedding follows its
    object through the dropouts and the permutation of the rows.)
    -> a list of T (dets (S, R, 6), count (S), emb (S, R, D))"""
    rng = np.random.default_rng(seed)
    objects = max(1, min(R, M + M // 4 + 1) * 2 // 3) if objects is None else objects
    pos = rng.uniform(0, 300.0 + 45.0 * np.sqrt(objects), (S, objects, 2))
    vel = rng.uniform(-4, 4, (S, objects, 2))
    size = rng.uniform(30, 70, (S, objects, 2))
    cls = rng.integers(0, 3, (S, objects)).astype(F32)
    proto = rng.normal(size=(S, objects, D))
    proto /= np.linalg.norm(proto, axis=2, keepdims=True)
    dip = np.zeros((S, objects), np.int64)
    out = []
    for t in range(T):
        dets = np.tile(np.array([3000.0, 3000.0, 3040.0, 3040.0, 0.97, 1.0], F32), (S, R, 1))
        emb = np.ones((S, R, D), F32)                               # beyond the rows: valid embeddings that must not be read
        count = np.zeros(S, np.int32)
        leap = rng.random((S, objects)) < jump
        pos += vel + rng.uniform(-1, 1, pos.shape) + leap[:, :, None] * size * rng.uniform(0.45, 0.6, pos.shape) * rng.choice([-1.0, 1.0], pos.shape)
        start = (dip == 0) & (rng.random(dip.shape) < dip_rate)
        dip = np.where(start, rng.integers(1, 5, dip.shape), np.maximum(dip - 1, 0))
        for s in range(S):
            seen = rng.random(objects) >= 0.12
            lowc = dip[s] > 0
            conf = np.where(lowc, rng.uniform(0.02, 0.5, objects), rng.uniform(0.5, 1.0, objects))
            own = np.concatenate([pos[s], pos[s] + size[s], conf[:, None], cls[s][:, None]], axis=1)
            rows = own[seen].astype(F32)
            e = (proto[s][seen] * rng.uniform(0.5, 3.0, (int(seen.sum()), 1)) + noise * rng.normal(size=(int(seen.sum()), D)) / np.sqrt(D)).astype(F32)
            u = rng.random(len(rows))
            e[u < bad / 2] = 0.0
            e[(u >= bad / 2) & (u < bad), rng.integers(0, D)] = np.nan
            perm = rng.permutation(len(rows))
            rows, e = rows[perm][:R], e[perm][:R]
            dets[s, :len(rows)] = rows
            emb[s, :len(rows)] = e
            count[s] = len(rows)
            u = rng.random()
            if u < 0.04:
                count[s] = 0
            elif u < 0.07:
                count[s] = -3
            elif u < 0.10:
                dets[s, len(rows):] = 0.0
                count[s] = R + 5
        out.append((dets, count, emb))
    return out
