"""The numpy statement of the per-stream IoU tracker's rule (include/yfv2.h "identity across frames"; the
library's one function of the IoU is track_iou, csrc/yfv2_track.hip, behind yfv2_track_iou).  Every fp32 operation below is a numpy
float32 operation of its own, which is the whole specification of the arithmetic; everything else is integers.

`greedy` is the rule's walk as written; `mutual_best` is the parallel form the kernel runs (the first edge of the order among the
edges sharing a row or a slot with it is taken, round after round) and also reports its rounds.  The tests pin them to each other."""
import numpy as np

HEADER, SLOT = 8, 10
F32 = np.float32


def state_words(M):
    return HEADER + SLOT * M


def iou(a, b):
    """a (..., 4), b (..., 4) fp32 boxes x1, y1, x2, y2 (broadcast against each other) -> fp32 IoU, as the tile merge computes it"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(all="ignore"):
        aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        ba = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        xx1 = np.where(a[..., 0] > b[..., 0], a[..., 0], b[..., 0])
        yy1 = np.where(a[..., 1] > b[..., 1], a[..., 1], b[..., 1])
        xx2 = np.where(a[..., 2] < b[..., 2], a[..., 2], b[..., 2])
        yy2 = np.where(a[..., 3] < b[..., 3], a[..., 3], b[..., 3])
        dw, dh = xx2 - xx1, yy2 - yy1
        w = np.where(dw > 0, dw, F32(0))
        h = np.where(dh > 0, dh, F32(0))
        inter = w * h
        v = inter / ((aa + ba) - inter)
    assert v.dtype == F32
    return v


def valid_rows(rows):
    """rows (n, 6) fp32 -> bool (n): all six finite, x2 > x1, y2 > y1"""
    rows = np.asarray(rows, F32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        return np.isfinite(rows).all(axis=1) & (rows[:, 2] > rows[:, 0]) & (rows[:, 3] > rows[:, 1])


def edges(rows, slot_box, slot_cls, live, match_thres, class_aware):
    """-> (V (n, M) fp32, E (n, M) bool): the IoU of every row with every slot and which pairs are edges"""
    rows = np.asarray(rows, F32).reshape(-1, 6)
    V = iou(rows[:, None, :4], np.asarray(slot_box, F32)[None, :, :])
    with np.errstate(all="ignore"):
        E = valid_rows(rows)[:, None] & np.asarray(live, bool)[None, :] & (V.astype(np.float64) > float(match_thres))   # NaN: False
        if class_aware:
            E &= rows[:, 5][:, None] == np.asarray(slot_cls, F32)[None, :]
    return V, E


def _bits(V):
    """a positive fp32 orders like its bit pattern"""
    return np.ascontiguousarray(V, F32).view(np.int32).astype(np.int64)


def greedy(V, E):
    """the rule's walk: edges by v descending, row ascending, slot ascending; an edge is taken if both ends are free.
    -> slot_of_row (n) int, -1 = unmatched"""
    n, M = E.shape
    rr, ss = np.nonzero(E)
    vb = _bits(V)[rr, ss]
    order = np.lexsort((ss, rr, -vb))
    slot_of_row = np.full(n, -1, np.int64)
    slot_used = np.zeros(M, bool)
    for k in order:
        r, s = int(rr[k]), int(ss[k])
        if slot_of_row[r] < 0 and not slot_used[s]:
            slot_of_row[r] = s
            slot_used[s] = True
    return slot_of_row


def mutual_best(V, E):
    """the parallel form: every round each free row names its best free slot (highest v, lowest slot), each free slot finds its best
    row over ALL free rows with an edge to it (highest v, lowest row), mutual pairs are taken; until no free row has an edge.
    -> (slot_of_row, rounds)"""
    n, M = E.shape
    K = np.where(E, _bits(V), 0)
    slot_of_row = np.full(n, -1, np.int64)
    free_r, free_s = np.ones(n, bool), np.ones(M, bool)
    rounds = 0
    while n and M:
        Kf = np.where(free_r[:, None] & free_s[None, :], K, 0)
        if not (Kf > 0).any():
            break
        rounds += 1
        row_best = Kf.argmax(axis=1)            # the first maximum: the lowest slot
        slot_best = Kf.argmax(axis=0)           # ... the lowest row
        for r in np.nonzero(Kf.max(axis=1) > 0)[0]:
            s = row_best[r]
            if slot_best[s] == r:
                slot_of_row[r] = s
                free_r[r] = False
                free_s[s] = False
    return slot_of_row, rounds


def update_stream(st, rows, count, rule, match=greedy):
    """One frame of one stream.  st: (8 + 10 M) int32, changed in place; rows (R, 6) fp32; rule: dict with max_tracks, match_thres,
    class_aware, init_conf, max_misses, confirm_hits.  -> (track_id (R), track_hits (R), fresh rows' indices)"""
    M = int(rule["max_tracks"])
    rows = np.ascontiguousarray(rows, F32).reshape(-1, 6)
    R = rows.shape[0]
    n = min(max(int(count), 0), R)
    head, slots = st[:HEADER], st[HEADER:].reshape(M, SLOT)
    fl = slots[:, :6].view(F32)                                     # a view: writes go to the state
    live = slots[:, 6] != 0
    V, E = edges(rows[:n], fl[:, :4], fl[:, 5], live, rule["match_thres"], rule["class_aware"])
    slot_of_row = match(V, E)
    if isinstance(slot_of_row, tuple):
        slot_of_row = slot_of_row[0]
    matched = np.zeros(M, bool)
    for r in range(n):
        s = slot_of_row[r]
        if s >= 0:
            matched[s] = True
            slots[s, :6] = rows[r].view(np.int32)
            slots[s, 7] += 1; slots[s, 8] = 0; slots[s, 9] += 1
    for s in range(M):
        if live[s] and not matched[s]:
            slots[s, 8] += 1; slots[s, 9] += 1
            if slots[s, 8] > int(rule["max_misses"]):
                slots[s, :] = 0
                head[4] += 1
    free = [s for s in range(M) if slots[s, 6] == 0]
    ok = valid_rows(rows[:n])
    k = 0
    for r in range(n):
        if slot_of_row[r] >= 0 or not ok[r] or not rows[r, 4] >= F32(rule["init_conf"]):
            continue
        if k < len(free):
            s = free[k]
            k += 1
            head[0] += 1
            slots[s, :6] = rows[r].view(np.int32)
            slots[s, 6:] = (head[0], 1, 0, 1)
            head[3] += 1
            slot_of_row[r] = s
        else:
            head[5] += 1
    head[2] += 1
    head[1] = int((slots[:, 6] != 0).sum())
    tid, hits = np.zeros(R, np.int32), np.zeros(R, np.int32)
    for r in range(n):
        if slot_of_row[r] >= 0:
            tid[r], hits[r] = slots[slot_of_row[r], 6], slots[slot_of_row[r], 7]
    return tid, hits, np.nonzero(hits == int(rule["confirm_hits"]))[0].astype(np.int32)


class Model:
    """S streams of M slots: the state as the device holds it, and one call's update"""

    def __init__(self, streams, **rule):
        self.rule = dict(max_tracks=64, match_thres=0.3, class_aware=True, init_conf=0.0, max_misses=30, confirm_hits=3)
        self.rule.update(rule)
        self.S, self.M = int(streams), int(self.rule["max_tracks"])
        self.state = np.zeros((self.S, state_words(self.M)), np.int32)

    def update(self, dets, count, streams=None, match=greedy):
        """dets (B, R, 6), count (B), streams: B distinct stream indices (None: 0..B-1) -> dict of track_id (B, R), track_hits (B, R),
        fresh_dets (B, R, 6) / fresh_src (B, R) (zero beyond fresh_count) and fresh_count (B)"""
        dets = np.ascontiguousarray(dets, F32)
        B, R = dets.shape[0], dets.shape[1]
        streams = list(range(B)) if streams is None else [int(s) for s in streams]
        assert len(streams) == B and len(set(streams)) == B and all(0 <= s < self.S for s in streams)
        out = {"track_id": np.zeros((B, R), np.int32), "track_hits": np.zeros((B, R), np.int32), "fresh_dets": np.zeros((B, R, 6), F32),
               "fresh_src": np.zeros((B, R), np.int32), "fresh_count": np.zeros(B, np.int32)}
        for b, s in enumerate(streams):
            tid, hits, fresh = update_stream(self.state[s], dets[b], count[b], self.rule, match)
            out["track_id"][b], out["track_hits"][b] = tid, hits
            out["fresh_count"][b] = len(fresh)
            out["fresh_src"][b, :len(fresh)] = fresh
            out["fresh_dets"][b, :len(fresh)] = dets[b, fresh]
        return out


def chain_case(links=40):
    """The input whose every edge but the last has a heavier neighbour: `links` tracks 16 wide and 10 high, and as many rows of
    the same size; row j overlaps track j by 4 + j / 16 pixels and track j + 1 by 1 / 32 more.  All values are dyadic: exact in
    fp32.  -> (tracks (links, 6), rows (links, 6)): feed `tracks` to an empty table first (they become slots 0 .. links - 1)."""
    tracks, rows = np.zeros((links, 6), F32), np.zeros((links, 6), F32)
    x = 0.0
    for j in range(links):
        ov = 4.0 + j / 16.0
        tracks[j] = (x, 0.0, x + 16.0, 10.0, 0.9, 0.0)
        xr = x + 16.0 - ov                       # row j: overlaps track j by ov
        rows[j] = (xr, 0.0, xr + 16.0, 10.0, 0.9, 0.0)
        x = xr + 16.0 - (ov + 1.0 / 32.0)        # track j + 1: overlaps row j by ov + 1 / 32
    assert np.array_equal(tracks.astype(np.float64), tracks) and float(x) == float(F32(x))
    return tracks, rows
