"""The input sizes, batches and class counts at which every training kernel of yfv2_train.hip is checked one layer deep
(tests/train_layers.py): ONE table, as data, read by the golden generator (make_golden.py train_shapes), the CPU test
(tests/test_train_layers_host.py) and the GPU test (tests/test_gpu_train_layers.py).

A case is (H, W, B, classes, T, seed, raises).  Weights, images and labels are make_golden.train_case_inputs' recipe with H and W
as parameters (rebuilt from the seed, never stored); the anchors are loss_cases.anchors_for(H, W).

The four launch formulas of yfv2_train.hip that decide which path a layer takes are restated below as plain arithmetic, each with
the line it restates, and `coverage` derives from them what the table as a whole reaches: the host test asserts every entry of
REQUIRED, so a later edit of the cases cannot silently lose a path.  Pure numpy / torch: no device, no native library."""
import collections

import numpy as np

from loss_cases import anchors_for  # noqa: F401  (re-exported: the cases' anchors)

Case = collections.namedtuple("Case", "H W B classes T seed raises")
LR = 0.001

CASES = (
    Case(32, 32, 2, 3, 3, 41, False),      # maps of 4 and 1 pixel, 2 values per BatchNorm channel, a BatchNorm block spanning hundreds of planes
    Case(32, 64, 5, 255, 6, 42, False),    # a 1-high map, 255 output rows (ragged last MFMA row tile, 4 z-blocks)
    Case(96, 32, 4, 1, 5, 43, False),      # a 1-wide map, pixel counts 3, 12, 48, 192, 768, one class row
    Case(64, 96, 3, 20, 5, 44, False),     # 96 and 1536 pixels (half-filled wave, ragged block)
    Case(128, 128, 1, 80, 4, 45, False),   # batch 1, reduce_segments exactly 2
    Case(160, 128, 2, 80, 6, 46, False),   # a ragged third 4096-pixel chunk (stem weight gradient), 5 BatchNorm segments with one crossing the image boundary, planes longer than BN_EPB
    Case(64, 64, 87, 2, 40, 47, False),    # upw = 2 with a ragged last wave in fpn.conv1x1_2's weight gradient (87 units x 12 tile blocks); ragged chunks in the depthwise weight gradient
    Case(32, 32, 1, 3, 2, 48, True),       # one value per channel: must raise
)
SEQUENCE_SIZES = ((64, 96, 3), (96, 32, 2), (64, 96, 3))   # (H, W, B): one module and one optimizer across input sizes
SEQUENCE_BATCHES = (3, 1, 3)                               # ... and across batch sizes at 64 x 96
SEQUENCE_CLASSES, SEQUENCE_SEED = 20, 44
# The sequence tests compare gradients of two runs, device against device.  yfv2_loss sums the matches of one (image, cell) with float
# atomicAdd, whose order changes from run to run when DIFFERENT labels share a cell (measured at 64 x 96, batch 1, five labels in the one
# image: 2 of 40 iterations returned other last bits in the logit gradients, and every parameter gradient followed; batch 3: none of 40).
# The training kernels themselves repeat bit for bit, and the atomics have their own test (test_gpu_loss_shapes.py), so the sequence steps
# carry ONE label per image: its matches on several anchors or neighbour cells add equal terms or touch different entries, in any order.


def case_id(c):
    return "%dx%d_b%d_c%d" % (c.H, c.W, c.B, c.classes)


def case_inputs(c, B=None):
    """-> (state_dict, x (B, 3, H, W) float32 array, labels (T, 6) float32 array): make_golden.train_case_inputs at H x W"""
    import yolo_fastestv2_amd as yfv2
    B = c.B if B is None else B
    w = yfv2.random_state_dict(c.seed, classes=c.classes)
    rng = np.random.Generator(np.random.PCG64(c.seed))
    x = rng.random((B, 3, c.H, c.W), dtype=np.float32)
    t = np.zeros((c.T, 6), np.float32)
    t[:, 0] = rng.integers(0, B, c.T)
    t[:, 1] = rng.integers(0, c.classes, c.T)
    t[:, 2:4] = rng.random((c.T, 2)) * 0.9 + 0.05
    t[:, 4:6] = rng.random((c.T, 2)) * 0.5 + 0.03
    return w, x, t


def sequence_inputs(H, W, B, step):
    """-> (case, x, labels) of one step of a sequence test: case_inputs' recipe with one label per image (label i in image i), sized
    70 x 110 of 352: within a factor of 2 of the third fine anchor (55.7, 138.3) and of the first coarse one (126.9, 78.2), so that
    both scales have matches"""
    c = Case(H, W, B, SEQUENCE_CLASSES, B, SEQUENCE_SEED + step, False)
    _, x, t = case_inputs(c)
    t[:, 0] = np.arange(B)
    t[:, 4:6] = np.asarray((70.0 / 352.0, 110.0 / 352.0), np.float32)
    return c, x, t


# ---- the launch formulas (yolo_fastestv2_amd/csrc/yfv2_train.hip), restated
BN_EPB = 1024    # `constexpr int BN_EPB = 1024`: elements per block of bn_apply_kernel / bn_bwd_apply_kernel
CHUNK = 4096     # `const long long i0 = (long long)blockIdx.x * 4096`: output pixels per block of stem_wgrad_kernel / dw_wgrad_kernel


def reduce_segments(n, others):
    """`inline unsigned reduce_segments(size_t n, size_t others)`: blocks per channel of bn_stats_part_kernel / bn_bwd_part_kernel"""
    s = 1 if others >= 2048 else 2048 // max(others, 1)
    s = min(s, 64, n // 2048)
    return max(s, 1)


def pw_wgrad_launch(HW, B, cin, cout):
    """`Train::pw_weight_grad`: (seg, nseg, units, upw, tile blocks) of pw_wgrad_kernel"""
    cob, cib = (cout + 47) // 48, (cin + 47) // 48
    seg = 256
    while seg > 64 and ((HW + seg - 1) // seg) * B * cob * cib < 2048:
        seg >>= 1
    nseg = (HW + seg - 1) // seg
    units = nseg * B
    upw = min(max((units * cob * cib) // 512, 1), 16)
    return seg, nseg, units, upw, cob * cib


def wgrad_chunks(B, OHW):
    """`const unsigned chunks = (unsigned)(((size_t)B * HW + 4095) / 4096)` in Train::conv_bn_backward"""
    return (B * OHW + CHUNK - 1) // CHUNK


def pw_gemm_grid(HW, B, rows):
    """`Train::pw_forward` / `pw_data_grad`: `if (out.C <= 32)` two row tiles and one z-block, else four row tiles per z-block"""
    mt = 2 if rows <= 32 else 4
    return mt, (HW + 255) // 256, (1 if rows <= 32 else (rows + 63) // 64)


REQUIRED = ("map_of_1_pixel", "map_of_2_or_3_pixels", "bn_block_spans_100_planes", "two_values_per_bn_channel", "map_1_high", "map_1_wide",
            "reduce_segments_2", "reduce_segment_crosses_image", "plane_longer_than_bn_block", "stem_wgrad_ragged_third_chunk", "dw_wgrad_ragged_chunk",
            "pw_wgrad_upw2_ragged_wave", "rows_not_multiple_of_16", "rows_255_four_z_blocks", "one_class_row", "batch_1", "half_filled_wave",
            "pw_two_row_tiles", "pw_seg_64", "must_raise")
# (seg = 128 / 256 need 2048 waves at that segment length - pixels x batch of the 352 x 352 tests at batch 8 and 64; no small shape reaches them)


def coverage(cases=CASES):
    """{path name: [case ids that reach it]} from the formulas above over every layer of every case"""
    import train_layers as TL
    hit = collections.defaultdict(list)
    for c in cases:
        cid = case_id(c)
        if c.raises:
            if c.B * (c.H // 32) * (c.W // 32) == 1:
                hit["must_raise"].append(cid)
            continue
        if c.B == 1:
            hit["batch_1"].append(cid)
        for op in TL.topology(c.H, c.W, c.classes):
            if op.kind not in ("conv", "head"):
                continue
            HW, C = op.oh * op.ow, op.cout
            mark = lambda k: hit[k].append(cid) if cid not in hit[k] else None  # noqa: E731
            if HW == 1:
                mark("map_of_1_pixel")
            if HW in (2, 3):
                mark("map_of_2_or_3_pixels")
            if op.oh == 1 and op.ow > 1:
                mark("map_1_high")
            if op.ow == 1 and op.oh > 1:
                mark("map_1_wide")
            if op.kind == "conv":
                n = c.B * HW
                if n == 2:
                    mark("two_values_per_bn_channel")
                if min(BN_EPB, c.B * C * HW) // HW >= 100:
                    mark("bn_block_spans_100_planes")
                if HW > BN_EPB:
                    mark("plane_longer_than_bn_block")
                nseg = reduce_segments(n, C)
                if nseg == 2:
                    mark("reduce_segments_2")
                ln = (n + nseg - 1) // nseg
                if nseg > 1 and any((s * ln) // HW != (min(n, (s + 1) * ln) - 1) // HW for s in range(nseg)):
                    mark("reduce_segment_crosses_image")
                chunks = wgrad_chunks(c.B, HW)
                if op.conv == "stem" and chunks == 3 and (c.B * HW) % CHUNK:
                    mark("stem_wgrad_ragged_third_chunk")
                if op.conv.startswith("dw") and chunks >= 2 and (c.B * HW) % CHUNK:
                    mark("dw_wgrad_ragged_chunk")
            if op.conv == "pw":
                seg, nseg, units, upw, _ = pw_wgrad_launch(HW, c.B, op.cin, op.cout)
                mark("pw_seg_%d" % seg)
                if upw >= 2 and units % upw:
                    mark("pw_wgrad_upw2_ragged_wave")
                for rows in (op.cout, op.cin):          # forward rows = output channels, data gradient rows = input channels
                    if rows % 16:
                        mark("rows_not_multiple_of_16")
                    if pw_gemm_grid(HW, c.B, rows)[0] == 2:
                        mark("pw_two_row_tiles")
                if op.cout == 255 and pw_gemm_grid(HW, c.B, 255)[2] == 4:
                    mark("rows_255_four_z_blocks")
                if op.cout == 1:
                    mark("one_class_row")
                if HW % 64 == 32 and HW > 64:
                    mark("half_filled_wave")
    return dict(hit)
