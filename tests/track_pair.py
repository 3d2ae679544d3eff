"""What the GPU tests of the tracker's four forms share (test_gpu_track.py, _motion, _two_pass, _appearance): the fixtures, the
rows' helpers and `Pair` - a device Tracker and the numpy model of its form, stepped together and compared bit for bit after every
call.  The order of the outputs is restated here (`_outputs`), not taken from the package: the tests pin it on their own."""
import os

import numpy as np
import pytest
import torch

import track_appearance_model as ta
import track_model as tm
import track_motion_model as mm
import track_two_pass_model as tp

F32 = np.float32
S_ID, S_HITS, S_DETS, S_SRC, S_CNT, S_BOX, S_PASS, S_COS = -7, -8, -3.0, -9, -10, -5.0, -11, -6.0          # the outputs are pre-filled with these
LAYOUTS = [None, True]                                                                                     # motion: the plain slots, the motion slots
PASSES = [None, True]                                                                                      # second: one pass, two


@pytest.fixture(scope="module")
def yfv2():
    import yolo_fastestv2_amd
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert os.path.exists(yolo_fastestv2_amd.LIB_PATH), "libyfv2.so not built"
    return yolo_fastestv2_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(yfv2, dev):
    """the tracker needs no weights: an engine of the usual size"""
    return yfv2.Engine(dev, 352, 352, max_batch=4, plan={})


def _bits(t):
    return t.contiguous().view(torch.int32)


def _diff(what, got, want):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()[:6].tolist()
        raise AssertionError("%s (index, device, model): %s" % (what, [(i, hex(int(got[tuple(i)]) & 0xFFFFFFFF), hex(int(want[tuple(i)]) & 0xFFFFFFFF)) for i in bad]))


def _frame(rows, R=4):
    """rows: lists of x1, y1, x2, y2, conf, cls -> (1, R, 6) padded with a filler that is itself a valid row, and the count"""
    d = np.tile(np.array([900.0, 900.0, 910.0, 910.0, 0.99, 0.0], F32), (1, R, 1))
    if rows:
        d[0, :len(rows)] = np.array(rows, F32)
    return d, [len(rows)]


def _box(x, y=0.0, w=10.0, h=10.0, conf=0.9, cls=0.0):
    return [x, y, x + w, y + h, conf, cls]


def _outputs(B, R, fresh, box, passes, cos):
    """the tuple an update returns, in order: (name, shape, dtype, the value it is pre-filled with)"""
    i32, f32 = torch.int32, torch.float32
    return ([("track_id", (B, R), i32, S_ID), ("track_hits", (B, R), i32, S_HITS)]
            + ([("fresh_dets", (B, R, 6), f32, S_DETS), ("fresh_src", (B, R), i32, S_SRC), ("fresh_count", (B,), i32, S_CNT)] if fresh else [])
            + ([("track_box", (B, R, 4), f32, S_BOX)] if box else [])
            + ([("track_pass", (B, R), i32, S_PASS)] if passes else [])
            + ([("track_cos", (B, R), f32, S_COS)] if cos else []))


class Pair:
    """a device Tracker of any form and the model of that form, stepped together and compared after every call"""

    def __init__(self, yfv2, eng, streams, motion=None, second=None, appearance=None, **rule):
        self.dev, self.motion, self.second, self.appearance = eng.device, motion, second, appearance
        self.tracker = yfv2.Tracker(eng, streams, motion=motion, two_pass=second, appearance=appearance, **rule)
        if appearance is not None:
            self.model = ta.Model(streams, appearance=appearance, second=second, motion=motion, **rule)
        elif second is not None:
            self.model = tp.Model(streams, second=second, motion=motion, **rule)
        elif motion is not None:
            self.model = mm.Model(streams, motion=motion, **rule)
        else:
            self.model = tm.Model(streams, **rule)

    def step(self, dets, count, streams=None, emb=None, **kw):
        dets = np.ascontiguousarray(dets, F32)
        count = np.asarray(count, np.int32)
        if self.appearance is None:
            want = self.model.update(dets, count, streams)
        else:
            emb = np.ascontiguousarray(emb, F32)
            want = self.model.update(dets, count, emb, streams)
        self.compare(dets, count, streams, want, self.model.state, getattr(self.model, "feat", None), emb, **kw)
        return want

    def compare(self, dets, count, streams, want, wstate, wfeat=None, emb=None, fresh=True, box=None, passes=None, cos=None):
        """box, passes, cos: None - asked for where the form has them"""
        box = (self.motion is not None) if box is None else box
        passes = (self.second is not None) if passes is None else passes
        cos = (self.appearance is not None) if cos is None else cos
        B, R = dets.shape[:2]
        d, c = torch.from_numpy(dets).to(self.dev), torch.from_numpy(np.asarray(count, np.int32)).to(self.dev)
        desc = _outputs(B, R, fresh, box, passes, cos)
        out = tuple(torch.full(shape, fill, device=self.dev, dtype=dtype) for _, shape, dtype, fill in desc)
        app = {} if self.appearance is None else dict(emb=torch.from_numpy(emb).to(self.dev), cos=cos)
        got = self.tracker.update(d, c, streams, fresh=fresh, box=box, passes=passes, out=out, **app)
        assert len(got) == len(out) and all(g is o for g, o in zip(got, out))
        got = {name: g.cpu() for (name, _, _, _), g in zip(desc, got)}
        _diff("state", self.tracker.state.cpu(), torch.from_numpy(wstate))
        if self.appearance is not None:
            _diff("feat", self.tracker.feat.cpu(), torch.from_numpy(wfeat))
        assert torch.equal(got["track_id"], torch.from_numpy(want["track_id"])), "track_id"
        assert torch.equal(got["track_hits"], torch.from_numpy(want["track_hits"])), "track_hits"
        if cos:
            _diff("track_cos", _bits(got["track_cos"]), _bits(torch.from_numpy(want["track_cos"])))
        if passes:
            assert torch.equal(got["track_pass"], torch.from_numpy(want["track_pass"])), "track_pass"
        if box:
            _diff("track_box", _bits(got["track_box"]), _bits(torch.from_numpy(want["track_box"])))
        if fresh:
            assert torch.equal(got["fresh_count"], torch.from_numpy(want["fresh_count"])), "fresh_count"
            for b in range(B):
                k = int(want["fresh_count"][b])
                assert torch.equal(got["fresh_src"][b, :k], torch.from_numpy(want["fresh_src"][b, :k])), "fresh_src"
                assert torch.equal(_bits(got["fresh_dets"][b, :k]), _bits(torch.from_numpy(want["fresh_dets"][b, :k]))), "fresh_dets"
                assert (got["fresh_src"][b, k:] == S_SRC).all() and (got["fresh_dets"][b, k:] == S_DETS).all(), "rows beyond fresh_count were written"

    def header(self, stream=0):
        """issued, live, frames, births, deaths, dropped; with two passes also second; with appearance that and by appearance"""
        return self.model.state[stream, :8 if self.appearance is not None else 7 if self.second is not None else 6].tolist()

    def slots(self, stream=0):
        return self.model.state[stream, tm.HEADER:].reshape(-1, tm.SLOT if self.motion is None else mm.SLOT)
