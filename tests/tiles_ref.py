"""Host models of tiled detection (include/yfv2.h yfv2_tile_plan / yfv2_merge_tiles / yfv2_detect_tiled_u8), shared by
tests/test_tiles_host.py (CPU) and tests/test_gpu_tiles.py (GPU).

* plan_axis / plan_tiles: the tile plan, restated.
* merge_model: the merge rule in numpy fp32 with a stable argsort - what the device result is compared with bit for bit.
"""
import numpy as np

MAX_DET = 300


def plan_axis(L, t, o):
    """[(start, length)] of one axis: L <= t is the single interval [0, L); otherwise n = ceil((L - t) / (t - o)) + 1
    intervals of length t at min(i * (t - o), L - t)."""
    assert L >= 1 and t >= 1 and 0 <= o < t
    if L <= t:
        return [(0, L)]
    s = t - o
    n = -(-(L - t) // s) + 1
    return [(min(i * s, L - t), t) for i in range(n)]


def plan_tiles(frame_h, frame_w, tile=(352, 352), overlap=(64, 64), include_full=False, frame=0):
    """[(frame, x0, y0, width, height)] row-major, y outer; the whole frame last if asked for and the grid has > 1 tile"""
    ys, xs = plan_axis(frame_h, tile[0], overlap[0]), plan_axis(frame_w, tile[1], overlap[1])
    out = [(frame, x0, y0, w, h) for y0, h in ys for x0, w in xs]
    if include_full and len(out) > 1:
        out.append((frame, 0, 0, frame_w, frame_h))
    return out


def _match(kb, ka, b, a, metric):
    """fp32 match of the kept boxes kb (n,4) / areas ka (n) with one box b (4) / area a, as torchvision computes IoU"""
    zero = np.float32(0)
    w = np.maximum(zero, np.minimum(kb[:, 2], b[2]) - np.maximum(kb[:, 0], b[0]))
    h = np.maximum(zero, np.minimum(kb[:, 3], b[3]) - np.maximum(kb[:, 1], b[1]))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        m = inter / ((ka + a) - inter) if metric == 0 else inter / np.minimum(ka, a)
    assert m.dtype == np.float32
    return m


def merge_model(tile_dets, tile_count, tiles, F, thres, metric, max_out, fill=0.0, fill_src=0):
    """tile_dets (T,300,6) fp32, tile_count (T), tiles [(frame, x0, y0, w, h)] -> (dets (F,max_out,6) fp32, src (F,max_out)
    int32, count (F) int32); rows beyond count hold `fill` / `fill_src`.  The rule of include/yfv2.h: candidates of a frame =
    its tiles in ascending k, rows r < tile_count[k], x += fp32(x0), y += fp32(y0) in fp32; order = conf descending, stable
    over (k, r); greedy walk, dropping a candidate if a kept one has an equal class and double(match) > thres; stop at max_out."""
    tile_dets = np.asarray(tile_dets, np.float32)
    thres = float(thres)
    dets = np.full((F, max_out, 6), fill, np.float32)
    src = np.full((F, max_out), fill_src, np.int32)
    count = np.zeros(F, np.int32)
    for f in range(F):
        rows, origin = [], []
        for k, (tf, x0, y0, _w, _h) in enumerate(tiles):
            if tf != f:
                continue
            n = int(tile_count[k])
            r = tile_dets[k, :n].copy()
            r[:, 0] = r[:, 0] + np.float32(x0)
            r[:, 2] = r[:, 2] + np.float32(x0)
            r[:, 1] = r[:, 1] + np.float32(y0)
            r[:, 3] = r[:, 3] + np.float32(y0)
            rows.append(r)
            origin.append(k * MAX_DET + np.arange(n, dtype=np.int32))
        if not rows:
            continue
        rows, origin = np.concatenate(rows), np.concatenate(origin)
        order = np.argsort(-rows[:, 4], kind="stable")
        rows, origin = rows[order], origin[order]
        area = (rows[:, 2] - rows[:, 0]) * (rows[:, 3] - rows[:, 1])
        kept = np.zeros(max_out, np.int64)
        nk = 0
        for i in range(len(rows)):
            if nk >= max_out:
                break
            ks = kept[:nk]
            same = rows[ks, 5] == rows[i, 5]
            if same.any():
                ks = ks[same]
                m = _match(rows[ks, :4], area[ks], rows[i, :4], area[i], metric)
                if (m.astype(np.float64) > thres).any():
                    continue
            kept[nk] = i
            nk += 1
        dets[f, :nk] = rows[kept[:nk]]
        src[f, :nk] = origin[kept[:nk]]
        count[f] = nk
    return dets, src, count
