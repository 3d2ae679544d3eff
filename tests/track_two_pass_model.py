"""The numpy statement of the tracker's two-pass form (include/yfv2.h "identity across frames, two association passes"; DESIGN.md
4.20).  Everything that is not the second pass - the IoU, the valid rows, the walk and its parallel form, the filter - is
track_model's and track_motion_model's, imported and not changed; this file restates the frame's order with the places the two-pass
rule changes: the rows' classes, the first pass over the HIGH rows, the second pass over the LOW rows and the slots still unmatched,
births from HIGH rows only, header word 6 and track_pass.

One function covers both layouts, as the one entry point does: motion=None is the plain 10-word slot (the IoU against the last
box), a dict the 32-word motion slot (step 0, the IoU against the predicted corners, the filter update, track_box).  `match` and
`match_low` are the matching of the first and of the second pass: track_model.greedy, the rule's walk as written, or
track_model.mutual_best, the parallel form the kernel runs, which also reports its rounds."""
import numpy as np

import track_model as tm
import track_motion_model as mm
from track_model import F32, HEADER, greedy, mutual_best  # noqa: F401  (the rule's shared parts)

DEFAULT = dict(high_conf=0.5, low_conf=0.1, match_thres_low=0.5, tracked_only=True)
ONE_PASS = dict(high_conf=-np.inf, low_conf=-np.inf, match_thres_low=0.5, tracked_only=True)   # every valid row is HIGH


def second_of(second):
    s = dict(DEFAULT)
    s.update({} if second in (None, True) else second)
    return s


def classes(rows, ok, second):
    """rows (n, 6), ok (n) bool: the valid rows -> (high (n), low (n)) bool; a valid row that is neither is OUT (fp32 compares)"""
    conf = np.asarray(rows, F32).reshape(-1, 6)[:, 4]
    with np.errstate(all="ignore"):
        high = ok & (conf >= F32(second["high_conf"]))
        low = ok & (conf >= F32(second["low_conf"])) & ~high
    return high, low


def _run(match, V, E):
    got = match(V, E)
    return (got[0], got[1]) if isinstance(got, tuple) else (got, None)


def update_stream(st, rows, count, rule, second, motion=None, match=greedy, match_low=None, stats=None):
    """One frame of one stream.  st: (8 + 10 M) int32, or with motion (8 + 32 M), changed in place; rows (R, 6) fp32; rule as in
    track_model; second: dict with high_conf, low_conf, match_thres_low, tracked_only; stats: a dict of counters to add to (below).
    -> (track_id (R), track_hits (R), track_pass (R), track_box (R, 4) (zero in the plain form), fresh rows' indices)"""
    plain = motion is None
    match_low = match if match_low is None else match_low
    M = int(rule["max_tracks"])
    SLOT = tm.SLOT if plain else mm.SLOT
    rows = np.ascontiguousarray(rows, F32).reshape(-1, 6)
    R = rows.shape[0]
    n = min(max(int(count), 0), R)
    head, slots = st[:HEADER], st[HEADER:].reshape(M, SLOT)
    fl = slots[:, :6].view(F32)                                     # a view: writes go to the state
    live = slots[:, 6] != 0
    misses0 = slots[:, 8].copy()                                    # the misses words when the frame begins
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
    # 1 valid, and the classes
    high, low = classes(rows[:n], ok, second)
    # 2 / 3 the first pass: the HIGH rows, match_thres
    V, E = tm.edges(rows[:n], boxes, fl[:, 5], offered, rule["match_thres"], rule["class_aware"])
    E &= high[:, None]
    slot_of_row, rounds1 = _run(match, V, E)
    slot_of_row = np.array(slot_of_row, np.int64)
    taken = np.zeros(M, bool)
    taken[slot_of_row[slot_of_row >= 0]] = True
    # 3b the second pass: the LOW rows, the slots the first pass left unmatched, match_thres_low
    cand = offered & ~taken
    if second["tracked_only"]:
        cand = cand & (misses0 == 0)
    _, E_any = tm.edges(rows[:n], boxes, fl[:, 5], offered, second["match_thres_low"], rule["class_aware"])
    E_any &= low[:, None]                                           # what a LOW row could have had, were nothing in its way
    E2 = E_any & cand[None, :]
    second_slot, rounds2 = _run(match_low, V, E2)
    second_slot = np.array(second_slot, np.int64)
    assert not ((slot_of_row >= 0) & (second_slot >= 0)).any() and not taken[second_slot[second_slot >= 0]].any()
    pass_of_row = np.where(slot_of_row >= 0, 1, np.where(second_slot >= 0, 2, 0)).astype(np.int32)
    slot_of_row = np.where(slot_of_row >= 0, slot_of_row, second_slot)
    if stats is not None:
        stats["second"] = stats.get("second", 0) + int((pass_of_row == 2).sum())
        stats["barred"] = stats.get("barred", 0) + int((E_any & (offered & ~taken & ~cand)[None, :]).any(axis=0).sum())
        lost = 0
        for h in np.nonzero(pass_of_row == 1)[0]:                   # a LOW row with the higher IoU for a slot a HIGH row took
            s = slot_of_row[h]
            lost += int((E_any[:, s] & (tm._bits(V[:, s]) > tm._bits(V[h, s]))).any())
        stats["lost"] = stats.get("lost", 0) + lost
        stats.setdefault("rounds", []).append((rounds1, rounds2))
    box = np.zeros((R, 4), F32)
    rs = np.nonzero(slot_of_row >= 0)[0]                            # 4 matched: identical for both passes (distinct slots: at once)
    ss = slot_of_row[rs]
    if not plain and len(rs):
        filt[ss] = mm.update(filt[ss], z[rs], mm.scales(filt[ss]), motion)
        box[rs] = mm.corners(filt[ss])
    slots[ss, :6] = rows[rs].view(np.int32)
    slots[ss, 7] += 1; slots[ss, 8] = 0; slots[ss, 9] += 1
    unmatched = live.copy()                                         # 5 unmatched: a barred slot is simply unmatched
    unmatched[ss] = False
    slots[unmatched, 8] += 1; slots[unmatched, 9] += 1
    dead = unmatched & (slots[:, 8] > int(rule["max_misses"]))
    slots[dead, :] = 0
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
            head[3] += 1
            slot_of_row[r] = s
            pass_of_row[r] = 1
        else:
            head[5] += 1
    head[2] += 1                                                    # 7 header
    head[1] = int((slots[:, 6] != 0).sum())
    head[6] += int((pass_of_row == 2).sum())
    tid, hits, tpass = np.zeros(R, np.int32), np.zeros(R, np.int32), np.zeros(R, np.int32)
    for r in range(n):
        if slot_of_row[r] >= 0:
            tid[r], hits[r], tpass[r] = slots[slot_of_row[r], 6], slots[slot_of_row[r], 7], pass_of_row[r]
    return tid, hits, tpass, box, np.nonzero(hits == int(rule["confirm_hits"]))[0].astype(np.int32)


class Model(tm.Model):
    """S streams of M slots in the two-pass form: track_model.Model's state (motion=None) or track_motion_model.Model's (motion=True
    or a dict).  update returns track_pass too and, with motion, track_box; self.stats adds up, over every frame: second (second-pass
    matches), barred (slots tracked_only kept from a LOW row that had an edge to them), lost (first-pass matches whose slot a LOW row
    had the higher IoU for) and rounds, a list of (first pass, second pass) round counts where the matching reports them."""

    def __init__(self, streams, second=None, motion=None, **rule):
        super().__init__(streams, **rule)
        self.second = second_of(second)
        if motion is None or motion is False:
            self.motion = None
        else:
            self.motion = dict(mm.DEFAULT)
            self.motion.update({} if motion is True else motion)
            self.state = np.zeros((self.S, mm.state_words(self.M)), np.int32)
        self.stats = {}

    def update(self, dets, count, streams=None, match=greedy, match_low=None):
        dets = np.ascontiguousarray(dets, F32)
        B, R = dets.shape[0], dets.shape[1]
        streams = list(range(B)) if streams is None else [int(s) for s in streams]
        assert len(streams) == B and len(set(streams)) == B and all(0 <= s < self.S for s in streams)
        out = {"track_id": np.zeros((B, R), np.int32), "track_hits": np.zeros((B, R), np.int32), "track_pass": np.zeros((B, R), np.int32),
               "fresh_dets": np.zeros((B, R, 6), F32), "fresh_src": np.zeros((B, R), np.int32), "fresh_count": np.zeros(B, np.int32)}
        if self.motion is not None:
            out["track_box"] = np.zeros((B, R, 4), F32)
        for b, s in enumerate(streams):
            tid, hits, tpass, box, fresh = update_stream(self.state[s], dets[b], count[b], self.rule, self.second, self.motion, match, match_low, self.stats)
            out["track_id"][b], out["track_hits"][b], out["track_pass"][b] = tid, hits, tpass
            if self.motion is not None:
                out["track_box"][b] = box
            out["fresh_count"][b] = len(fresh)
            out["fresh_src"][b, :len(fresh)] = fresh
            out["fresh_dets"][b, :len(fresh)] = dets[b, fresh]
        return out

    def filters(self, stream=0):
        """(M, 4, 5) fp32 view of the stream's filter words (the motion layout only)"""
        return self.state[stream, HEADER:].reshape(self.M, mm.SLOT)[:, mm.FILTER:mm.FILTER + 20].view(F32).reshape(self.M, 4, 5)


def dip_case(high=5, dip=4, after=3, conf_dip=0.3, R=2):
    """One 50 x 50 object moving 5 px / frame (IoU 9 / 11 = 0.818 from frame to frame against its last box): conf 0.9 for `high`
    frames, conf_dip for `dip` frames, 0.9 again for `after`.  -> a list of (dets (1, R, 6), count (1))"""
    out = []
    for t in range(high + dip + after):
        d = np.zeros((1, R, 6), F32)
        x = F32(100.0 + 5.0 * t)
        d[0, 0] = (x, 40.0, x + F32(50.0), 90.0, conf_dip if high <= t < high + dip else 0.9, 0.0)
        out.append((d, np.array([1], np.int32)))
    return out


def walk_case(seed, S, T, R, M, objects=None, dip_rate=0.2, intruder=0.0):
    """Seeded random walks with score dips and dropouts for S streams: each object's conf is high most of the time and dips below
    0.5 for runs of frames; some objects drop out for a frame or two (so tracks carry misses when a LOW row returns on top of them);
    in some frames a HIGH twin overlaps an object less than the object's own LOW row does.  dip_rate: the chance per frame that an
    object at a high score begins a dip of 1 to 4 frames.  intruder: the chance per stream and frame of one more HIGH row far from
    every object - a spurious confident detection, which wants a slot (with more objects than slots, `objects` > M, the objects'
    own rows want them too).  Some counts are 0, negative or beyond R.
    -> a list of T (dets (S, R, 6), count (S)); the rows beyond a frame's count are valid rows that must not be read"""
    rng = np.random.default_rng(seed)
    objects = max(1, min(R, M + M // 4 + 1) * 2 // 3) if objects is None else objects
    pos = rng.uniform(0, 300.0 + 45.0 * np.sqrt(objects), (S, objects, 2))
    vel = rng.uniform(-4, 4, (S, objects, 2))
    size = rng.uniform(30, 70, (S, objects, 2))
    cls = rng.integers(0, 3, (S, objects)).astype(F32)
    dip = np.zeros((S, objects), np.int64)                          # frames of low score left
    out = []
    for t in range(T):
        dets = np.tile(np.array([3000.0, 3000.0, 3040.0, 3040.0, 0.97, 1.0], F32), (S, R, 1))
        count = np.zeros(S, np.int32)
        pos += vel + rng.uniform(-1, 1, pos.shape)
        start = (dip == 0) & (rng.random(dip.shape) < dip_rate)
        dip = np.where(start, rng.integers(1, 5, dip.shape), np.maximum(dip - 1, 0))
        for s in range(S):
            seen = rng.random(objects) >= 0.12                      # the others drop out
            low = dip[s] > 0
            conf = np.where(low, rng.uniform(0.02, 0.5, objects), rng.uniform(0.5, 1.0, objects))
            own = np.concatenate([pos[s], pos[s] + size[s], conf[:, None], cls[s][:, None]], axis=1)
            twin = seen & low & (rng.random(objects) < 0.3)         # a HIGH twin, shifted: a lower IoU with the track than the LOW row's
            shift = np.stack([0.3 * size[s, :, 0], np.zeros(objects)], axis=1)
            other = np.concatenate([pos[s] + shift, pos[s] + shift + size[s], rng.uniform(0.6, 1.0, (objects, 1)), cls[s][:, None]], axis=1)
            rows = np.concatenate([own[seen], other[twin]]).astype(F32)
            if intruder > 0.0 and rng.random() < intruder:
                x, y = rng.uniform(5000.0, 6000.0, 2)
                rows = np.concatenate([rows, np.array([[x, y, x + 40.0, y + 40.0, 0.9, 0.0]], F32)])
            rows = rows[rng.permutation(len(rows))][:R]
            dets[s, :len(rows)] = rows
            count[s] = len(rows)
            u = rng.random()
            if u < 0.04:
                count[s] = 0
            elif u < 0.07:
                count[s] = -3
            elif u < 0.10:
                dets[s, len(rows):] = 0.0                           # beyond the rows: zeros, invalid whatever the count says
                count[s] = R + 5
        out.append((dets, count))
    return out
