"""The numpy statement of the tracker's motion form (include/yfv2.h "identity across frames with a motion model"; DESIGN.md 4.19;
the library's one function of the filter is track_filter_step, csrc/yfv2_track.hip, behind yfv2_track_filter_step and
yfv2_track_birth).  Everything that is not the filter - the IoU, the valid rows, the walk and its parallel form - is track_model's.
Every fp32 operation below is a numpy float32 operation of its own, in the order the header writes it."""
import numpy as np

import track_model as tm
from track_model import F32, HEADER, greedy, iou, mutual_best, valid_rows  # noqa: F401  (the rule's shared parts)

SLOT, FILTER = 32, 10                       # a slot's words; its filters: words 10..29, cx, cy, w, h, each x, v, p00, p01, p11
X, V, P00, P01, P11 = range(5)
DEFAULT = dict(std_pos=1.0 / 20, std_vel=1.0 / 160, std_meas=1.0 / 20)


QNAN = np.array([0x7FC00000], np.int32).view(F32)[0]


def canon(a):
    """every NaN becomes THE quiet NaN: which one an invalid operation makes depends on the processor"""
    return np.where(np.isnan(a), QNAN, a).astype(F32)


def state_words(M):
    return HEADER + SLOT * M


def stds(motion):
    m = dict(DEFAULT)
    m.update(motion or {})
    return F32(m["std_pos"]), F32(m["std_vel"]), F32(m["std_meas"])


def predict(f, scale, motion=None):
    """f (..., 5) fp32 filters, scale (...) fp32 -> the filters one time step on"""
    sp, sv, _sm = stds(motion)
    f, l = np.asarray(f, F32), np.asarray(scale, F32)
    out = np.empty_like(f)
    with np.errstate(all="ignore"):
        tp, tv = sp * l, sv * l
        out[..., X] = f[..., X] + f[..., V]
        out[..., V] = f[..., V]
        out[..., P00] = (((f[..., P00] + f[..., P01]) + f[..., P01]) + f[..., P11]) + tp * tp
        out[..., P01] = f[..., P01] + f[..., P11]
        out[..., P11] = f[..., P11] + tv * tv
    assert out.dtype == F32
    return canon(out)


def update(f, z, scale, motion=None):
    """f (..., 5) PREDICTED filters, z (...) measurements, scale (...) -> the posterior filters"""
    _sp, _sv, sm = stds(motion)
    f, z, l = np.asarray(f, F32), np.asarray(z, F32), np.asarray(scale, F32)
    out = np.empty_like(f)
    with np.errstate(all="ignore"):
        tm_ = sm * l
        s = f[..., P00] + tm_ * tm_
        k0, k1 = f[..., P00] / s, f[..., P01] / s
        y = z - f[..., X]
        out[..., X] = f[..., X] + k0 * y
        out[..., V] = f[..., V] + k1 * y
        out[..., P00] = f[..., P00] - k0 * f[..., P00]
        out[..., P01] = f[..., P01] - k0 * f[..., P01]
        out[..., P11] = f[..., P11] - k1 * f[..., P01]
    assert out.dtype == F32
    return canon(out)


def measure(boxes):
    """boxes (..., >= 4) x1, y1, x2, y2 -> (..., 4) cx, cy, w, h"""
    b = np.asarray(boxes, F32)
    with np.errstate(all="ignore"):
        return np.stack([(b[..., 0] + b[..., 2]) * F32(0.5), (b[..., 1] + b[..., 3]) * F32(0.5), b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], axis=-1)


def corners(f):
    """f (..., 4, 5) -> (..., 4) x1, y1, x2, y2 of the filter state"""
    x = np.asarray(f, F32)[..., X]
    with np.errstate(all="ignore"):
        hw, hh = x[..., 2] * F32(0.5), x[..., 3] * F32(0.5)
        return canon(np.stack([x[..., 0] - hw, x[..., 1] - hh, x[..., 0] + hw, x[..., 1] + hh], axis=-1))


def scales(f):
    """f (..., 4, 5) -> (..., 4): the track's w for cx and w, its h for cy and h"""
    x = np.asarray(f, F32)[..., X]
    return np.stack([x[..., 2], x[..., 3], x[..., 2], x[..., 3]], axis=-1)


def birth(box, motion=None):
    """box (..., 4) -> (..., 4, 5): the filters of a track born from a row"""
    sp, sv, _sm = stds(motion)
    z = measure(box)
    l = np.stack([z[..., 2], z[..., 3], z[..., 2], z[..., 3]], axis=-1)
    f = np.zeros(z.shape + (5,), F32)
    with np.errstate(all="ignore"):
        tp, tv = (F32(2.0) * sp) * l, (F32(10.0) * sv) * l
        f[..., X] = z
        f[..., P00] = tp * tp
        f[..., P11] = tv * tv
    return f


def update_stream(st, rows, count, rule, motion=None, match=greedy):
    """One frame of one stream.  st: (8 + 32 M) int32, changed in place; otherwise track_model.update_stream's arguments.
    -> (track_id (R), track_hits (R), track_box (R, 4), fresh rows' indices)"""
    M = int(rule["max_tracks"])
    rows = np.ascontiguousarray(rows, F32).reshape(-1, 6)
    R = rows.shape[0]
    n = min(max(int(count), 0), R)
    head, slots = st[:HEADER], st[HEADER:].reshape(M, SLOT)
    fl = slots[:, :6].view(F32)
    filt = slots[:, FILTER:FILTER + 20].view(F32).reshape(M, 4, 5)   # a view: writes go to the state
    assert np.shares_memory(filt, st)
    live = slots[:, 6] != 0
    # 0 predict
    pred = predict(filt, scales(filt), motion)
    filt[live] = pred[live]
    with np.errstate(all="ignore"):
        blind = ~(np.isfinite(filt).all(axis=(1, 2)) & (filt[:, 2, X] > 0) & (filt[:, 3, X] > 0))
    # 1 valid, 2 edges on the predicted corners, 3 matching
    z = measure(rows[:n])
    ok = valid_rows(rows[:n]) & np.isfinite(z).all(axis=1)
    V, E = tm.edges(rows[:n], corners(filt), fl[:, 5], live & ~blind, rule["match_thres"], rule["class_aware"])
    E &= ok[:, None]
    slot_of_row = match(V, E)
    if isinstance(slot_of_row, tuple):
        slot_of_row = slot_of_row[0]
    box = np.zeros((R, 4), F32)
    matched = np.zeros(M, bool)
    for r in range(n):                                              # 4 matched
        s = slot_of_row[r]
        if s >= 0:
            matched[s] = True
            filt[s] = update(filt[s], z[r], scales(filt[s]), motion)
            box[r] = corners(filt[s])
            slots[s, :6] = rows[r].view(np.int32)
            slots[s, 7] += 1; slots[s, 8] = 0; slots[s, 9] += 1
    for s in range(M):                                              # 5 unmatched: the filter coasts
        if live[s] and not matched[s]:
            slots[s, 8] += 1; slots[s, 9] += 1
            if slots[s, 8] > int(rule["max_misses"]):
                slots[s, :] = 0
                head[4] += 1
    free = [s for s in range(M) if slots[s, 6] == 0]
    k = 0
    for r in range(n):                                              # 6 births
        if slot_of_row[r] >= 0 or not ok[r] or not rows[r, 4] >= F32(rule["init_conf"]):
            continue
        if k < len(free):
            s = free[k]
            k += 1
            head[0] += 1
            slots[s, :6] = rows[r].view(np.int32)
            slots[s, 6:10] = (head[0], 1, 0, 1)
            filt[s] = birth(rows[r, :4], motion)
            box[r] = corners(filt[s])
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
    return tid, hits, box, np.nonzero(hits == int(rule["confirm_hits"]))[0].astype(np.int32)


class Model(tm.Model):
    """track_model.Model with 32-word slots and the filters; update also returns track_box (B, R, 4)"""

    def __init__(self, streams, motion=None, **rule):
        super().__init__(streams, **rule)
        self.motion = dict(DEFAULT)
        self.motion.update({} if motion in (None, True) else motion)
        self.state = np.zeros((self.S, state_words(self.M)), np.int32)

    def update(self, dets, count, streams=None, match=greedy):
        dets = np.ascontiguousarray(dets, F32)
        B, R = dets.shape[0], dets.shape[1]
        streams = list(range(B)) if streams is None else [int(s) for s in streams]
        assert len(streams) == B and len(set(streams)) == B and all(0 <= s < self.S for s in streams)
        out = {"track_id": np.zeros((B, R), np.int32), "track_hits": np.zeros((B, R), np.int32), "track_box": np.zeros((B, R, 4), F32),
               "fresh_dets": np.zeros((B, R, 6), F32), "fresh_src": np.zeros((B, R), np.int32), "fresh_count": np.zeros(B, np.int32)}
        for b, s in enumerate(streams):
            tid, hits, box, fresh = update_stream(self.state[s], dets[b], count[b], self.rule, self.motion, match)
            out["track_id"][b], out["track_hits"][b], out["track_box"][b] = tid, hits, box
            out["fresh_count"][b] = len(fresh)
            out["fresh_src"][b, :len(fresh)] = fresh
            out["fresh_dets"][b, :len(fresh)] = dets[b, fresh]
        return out

    def filters(self, stream=0):
        """(M, 4, 5) fp32 view of the stream's filter words"""
        return self.state[stream, HEADER:].reshape(self.M, SLOT)[:, FILTER:FILTER + 20].view(F32).reshape(self.M, 4, 5)


def occlusion_case(seen=10, hidden=6, speed=8.0, size=64.0, R=2):
    """A size x size box moving `speed` px / frame: seen for `seen` frames, missing for `hidden`, seen again once.
    -> a list of (dets (1, R, 6), count (1))"""
    out = []
    for t in range(seen + hidden + 1):
        d = np.zeros((1, R, 6), F32)
        x = F32(100.0 + speed * t)
        d[0, 0] = (x, 50.0, x + F32(size), 50.0 + size, 0.9, 0.0)
        out.append((d, np.array([0 if seen <= t < seen + hidden else 1], np.int32)))
    return out
