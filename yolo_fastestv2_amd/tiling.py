"""Tile plans for detection on large frames (include/yfv2.h yfv2_tile_plan).

    tiles = plan_tiles(1080, 1920)                       # 352x352 tiles, 64 pixels of overlap: 4 x 7 = 28 tiles
    dets, src, count = engine.detect_tiled([frame], conf_thres=0.3, iou_thres=0.4)

A tile is ``(frame, x0, y0, width, height)``: a rectangle inside ``frames[frame]``.  The plan itself is host code of
libyfv2.so; nothing here needs a device.
"""
from . import _lib


def _pair(v, what):
    if isinstance(v, int):
        return int(v), int(v)
    v = tuple(v)
    if len(v) != 2:
        raise ValueError("%s must be an int or a (height, width) pair" % what)
    return int(v[0]), int(v[1])


def plan_tiles(frame_h, frame_w, tile=(352, 352), overlap=(64, 64), include_full=False, frame=0):
    """The tiles of one frame as a list of (frame, x0, y0, width, height), row-major, y outer.  Per axis of length L, tile t and
    overlap o (0 <= o < t): L <= t is the single interval [0, L); otherwise n = ceil((L - t) / (t - o)) + 1 tiles of length t
    at min(i * (t - o), L - t), the last one ending on the edge.  ``tile`` / ``overlap``: (height, width) or one int for both.
    ``include_full``: one more tile covering the whole frame comes last when the grid has more than one tile (large objects
    that no tile holds whole).  ``frame``: the index written to every tile."""
    th, tw = _pair(tile, "tile")
    oh, ow = _pair(overlap, "overlap")
    L = _lib.lib()
    args = (int(frame_h), int(frame_w), th, tw, oh, ow, 1 if include_full else 0)
    n = L.yfv2_tile_plan(*args, None, 0)
    if n < 0:
        raise ValueError(_lib.last_error())
    arr = (_lib.Tile * n)()
    if L.yfv2_tile_plan(*args, arr, n) != n:
        raise ValueError(_lib.last_error())
    return [(int(frame), t.x0, t.y0, t.width, t.height) for t in arr]


def tile_table(tiles):
    """list of (frame, x0, y0, width, height) -> a (yfv2_tile * T) array"""
    tiles = list(tiles)
    if not tiles:
        raise ValueError("tiles must not be empty")
    arr = (_lib.Tile * len(tiles))()
    for k, t in enumerate(tiles):
        if len(t) != 5:
            raise ValueError("tile %d: expected (frame, x0, y0, width, height)" % k)
        arr[k].frame, arr[k].x0, arr[k].y0, arr[k].width, arr[k].height = (int(v) for v in t)
    return arr


METRICS = {"iou": 0, "ios": 1, 0: 0, 1: 1}   # "ios": intersection over the smaller box


def metric_code(metric):
    if metric not in METRICS or isinstance(metric, bool):
        raise ValueError("metric must be 'iou' (intersection over union) or 'ios' (intersection over the smaller box), got %r" % (metric,))
    return METRICS[metric]


def crop_views(frames, tiles):
    """The crop of every tile as a view of its frame (no copy): what detect_tiled's tiles are to detect_frames."""
    return [frames[f][y0:y0 + h, x0:x0 + w] for f, x0, y0, w, h in tiles]

