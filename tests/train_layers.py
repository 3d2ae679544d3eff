"""The training kernels of yfv2_train.hip checked ONE LAYER DEEP: every op of the topology of oracle/yfv2_oracle.py (_conv_bn,
_shuffle_block, _tower, backbone, the heads) is evaluated in float64 on the CPU from the operands a run itself recorded, and
compared with what that run recorded as the op's result.  Nothing is amplified through the 79 layers, so the tolerance is a
forward-error bound read from the kernel's source, not a measured number:

    |recorded - float64| <= (k u + d 2^-53) M + floor        elementwise, u = 2^-24

M is the same operation evaluated in float64 on the absolute value of every term, k the number of fp32 roundings on the kernel's
path (table K below, each entry with the source line it counts), d the length of a double-precision sum where the kernel keeps one,
and floor = (k + 1) 2^-120 covers operands a matrix instruction may flush (a value below 2^-126 times a factor below 2^6).

A run record is a dict (oracle.train_step(trace=True)["record"] from the CPU, tests/test_gpu_train_layers.py's read-back through
Engine.debug_train_tensor from the device):
    "x" the image; "logits", "dlogits" six tensors each; "param", "pgrad" {state-dict name: tensor}; "run_before", "run_after"
    {running statistic: tensor}; per conv name "y:" (conv output), "z:" (op output window), "dy:", "dz:" (their gradients),
    "mean:", "invstd:"; per tensor no conv names ("backbone.maxpool", "backbone.stageS.I", "fpn.p2") "v:" and "g:".
Pure torch on the CPU: importable without a device and without the native library."""
import collections

import torch
import torch.nn.functional as F

import train_cases as TC

U = 2.0 ** -24
D = 2.0 ** -53
FLOOR = 2.0 ** -120
BN_EPS = 1e-5
STAGE_REPEATS, STAGE_CHANNELS, OUT_DEPTH = (4, 8, 4), (24, 48, 96, 192), 72

# k: fp32 roundings on each kernel's path (yolo_fastestv2_amd/csrc/yfv2_train.hip)
K = {
    "stem_fwd": 27,         # stem_fwd_kernel: `acc[co] = __builtin_fmaf(a.w[...], v, acc[co])`, 3 x 3 x 3 taps, one rounding each
    "dw_fwd": None,         # dw_fwd_kernel: `acc = __builtin_fmaf(w[ky * K + kx], ip[iy * IW + ix], acc)`: K * K
    "pw_fwd": None,         # pw_gemm_kernel: `acc[t][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(...)` over Cin terms, plus one (the store `acc[t][e][rr] + bi`)
    "head_fwd": None,       # the same with a bias: Cin + 1 + the bias add
    "bn_mean": 1,           # bn_apply_kernel: `const float fm = (float)m` (the sums are double: bn_stats_part_kernel)
    "bn_invstd": 1,         # `fi = (float)(1.0 / sqrt(var + 1e-5))`
    "bn_running": 1,        # `run_mean[c] = (float)(0.9 * (double)run_mean[c] + 0.1 * m)`
    "bn_apply": 4,          # `float v = (y[i] - s_mean[w.k]) * s_inv[w.k] * s_gamma[w.k] + s_beta[w.k]`: four operations, no contraction
    "bn_dbeta": 2,          # bn_bwd_apply_kernel: `s0 = (float)acc[4 * c + 2]` and `dbeta[c] += s0`
    "bn_dgamma": 4,         # bn_bwd_part_kernel: `xh = (y[...] - mc) * ic` (2) inside a double sum; then `s1 = (float)acc[...]`, `dgamma[c] += s1`
    "bn_bwd_dy": 11,        # `dy[i] = s_gamma * s_inv * (g - s_s0 * inv_n - xh * s_s1 * inv_n)`: s0 (1) inv_n (1) product (1); xh (2) s1 (3) inv_n (1) two
                            # products (2); two subtractions, gamma * inv and the last product (4): at most 11 on any term
    "pw_wgrad": None,       # pw_wgrad_kernel: fp32 matrix-instruction sums over at most `seg` pixels, then doubles; wgrad_finish_multi_kernel:
                            # `t.dw[i] += (float)t.scr[i]`: min(seg, pixels) + the cast + the add
    "chunk_wgrad": 24,      # stem_wgrad_kernel / dw_wgrad_kernel: 16 `__builtin_fmaf` per thread, `v += __shfl_down(v, d)` six times, then doubles; the finish: 2
    "head_bias": 3,         # bias_bwd_kernel: `db[co] += (float)red[0]`, once per scale into one tensor: a cast on each part, two adds on the total
    "dw_bwd_data": None,    # dw_bwd_data_kernel: `acc = __builtin_fmaf(w[ky * K + kx], gp[oy * OW + ox], acc)`: K * K (then `+=`: see below)
    "pw_bwd_data": None,    # pw_gemm_kernel<TRANS, ACCUM>: Cout terms plus one (then `*d + acc`)
    "upsample_bwd": 3,      # upsample2_bwd_kernel: three adds of the four children
    "maxpool_bwd": 4,       # maxpool_bwd_kernel: `acc += dout[...]` for at most four windows
    "copy": 0,              # view_copy_kernel
    "accumulate": 1,        # every `+=` into a gradient tensor: one rounding of the running total per consumer
}

# The CPU record comes from ATen's kernels, whose paths differ from the device's in a few places; check(..., aten=True) ADDS these
# roundings for such a record (the device is always held to K alone).  "n": ATen keeps the sum over the n = B * OH * OW values of a
# channel (or the n products of a weight gradient) in fp32 in an order it does not document, where the device kernel keeps it in
# double (or in fp32 runs of `seg` / 16 terms): any order of an n-term fp32 sum is within (n - 1) u of the absolute sum.
K_ATEN_EXTRA = {
    "bn_running": 3,        # the batch statistic rounded to fp32, two fp32 products and an fp32 sum, where the kernel rounds once
    "bn_apply": 4,          # y * alpha + (beta - mean * alpha) with alpha = gamma * invstd in fp32, from ATen's own rounded mean / invstd
    "bn_dbeta": "n", "bn_dgamma": "n", "bn_bwd_dy": "n", "head_bias": "n", "pw_wgrad": "n", "chunk_wgrad": "n",
}

Ref = collections.namedtuple("Ref", "key coff cstride C")   # channels coff, coff + cstride, ... (C of them) of the tensor `key`
Op = collections.namedtuple("Op", "kind name bn conv src dst src2 cin cout k stride pad groups relu oh ow slot")


def _op(kind, name, src, dst, oh, ow, **kw):
    d = dict(bn=None, conv="", src2=None, cin=src.C, cout=dst.C if dst else 0, k=1, stride=1, pad=0, groups=1, relu=False, slot=None)
    d.update(kw)
    return Op(kind=kind, name=name, src=src, dst=dst, oh=oh, ow=ow, **d)


def topology(H, W, classes, anchor_num=3):
    """the ops of one training forward at H x W in the oracle's order.  kinds: conv (conv + BatchNorm [+ ReLU]), maxpool, window (a
    conv's output IS a channel window of a block's output), pass (even channels copied), upcat, head"""
    ops = []

    def conv(kind, prefix, i, src, cout, ih, iw, relu):
        name, bn = "%s.%d" % (prefix, i), "%s.%d" % (prefix, i + 1)
        k, stride, pad, dw = {"pw": (1, 1, 0, 0), "dw3s1": (3, 1, 1, 1), "dw3s2": (3, 2, 1, 1), "dw5s1": (5, 1, 2, 1), "stem": (3, 2, 1, 0)}[kind]
        oh, ow = (ih + 2 * pad - k) // stride + 1, (iw + 2 * pad - k) // stride + 1
        ops.append(_op("conv", name, src, Ref("z:" + name, 0, 1, cout), oh, ow, bn=bn, conv=kind, k=k, stride=stride, pad=pad, groups=cout if dw else 1, relu=relu))
        return Ref("z:" + name, 0, 1, cout), oh, ow

    cur, h, w = conv("stem", "backbone.first_conv", 0, Ref("x", 0, 1, 3), 24, H, W, True)
    h, w = h // 2, w // 2
    ops.append(_op("maxpool", "backbone.maxpool", cur, Ref("v:backbone.maxpool", 0, 1, 24), h, w))
    cur, c2 = Ref("v:backbone.maxpool", 0, 1, 24), None
    for si in range(3):
        cin, cout = STAGE_CHANNELS[si], STAGE_CHANNELS[si + 1]
        mid = cout // 2
        for i in range(STAGE_REPEATS[si]):
            p = "backbone.stage%d.%d" % (si + 2, i)
            out = "v:" + p
            if i == 0:
                pd, oh, ow = conv("dw3s2", p + ".branch_proj", 0, cur, cin, h, w, False)
                pr, _, _ = conv("pw", p + ".branch_proj", 2, pd, cin, oh, ow, True)
                ops.append(_op("window", pr.key[2:], pr, Ref(out, 0, 1, cin), oh, ow))
                m1, _, _ = conv("pw", p + ".branch_main", 0, cur, mid, h, w, True)
                m2, _, _ = conv("dw3s2", p + ".branch_main", 3, m1, mid, h, w, False)
                m3, _, _ = conv("pw", p + ".branch_main", 5, m2, cout - cin, oh, ow, True)
                ops.append(_op("window", m3.key[2:], m3, Ref(out, cin, 1, cout - cin), oh, ow))
                h, w = oh, ow
            else:
                ops.append(_op("pass", p + ".pass", Ref(cur.key, 0, 2, mid), Ref(out, 0, 1, mid), h, w))
                m1, _, _ = conv("pw", p + ".branch_main", 0, Ref(cur.key, 1, 2, mid), mid, h, w, True)
                m2, _, _ = conv("dw3s1", p + ".branch_main", 3, m1, mid, h, w, False)
                m3, _, _ = conv("pw", p + ".branch_main", 5, m2, mid, h, w, True)
                ops.append(_op("window", m3.key[2:], m3, Ref(out, mid, 1, mid), h, w))
            cur = Ref(out, 0, 1, cout)
        if si == 1:
            c2, h2, w2 = cur, h, w
    c3 = cur

    def tower(p, src, th, tw):
        a, _, _ = conv("dw5s1", p, 0, src, OUT_DEPTH, th, tw, True)
        b, _, _ = conv("pw", p, 3, a, OUT_DEPTH, th, tw, False)
        c, _, _ = conv("dw5s1", p, 5, b, OUT_DEPTH, th, tw, True)
        return conv("pw", p, 8, c, OUT_DEPTH, th, tw, False)[0]

    s3, _, _ = conv("pw", "fpn.conv1x1_3", 0, c3, OUT_DEPTH, h, w, True)
    cls3, reg3 = tower("fpn.cls_head_3.block", s3, h, w), tower("fpn.reg_head_3.block", s3, h, w)
    p2 = Ref("v:fpn.p2", 0, 1, c3.C + c2.C)
    ops.append(_op("upcat", "fpn.p2", c3, p2, h2, w2, src2=c2))
    s2, _, _ = conv("pw", "fpn.conv1x1_2", 0, p2, OUT_DEPTH, h2, w2, True)
    cls2, reg2 = tower("fpn.cls_head_2.block", s2, h2, w2), tower("fpn.reg_head_2.block", s2, h2, w2)
    A = anchor_num
    for slot, (src, name, co, hh, ww) in enumerate(((reg2, "output_reg_layers", 4 * A, h2, w2), (cls2, "output_obj_layers", A, h2, w2),
                                                    (cls2, "output_cls_layers", classes, h2, w2), (reg3, "output_reg_layers", 4 * A, h, w),
                                                    (cls3, "output_obj_layers", A, h, w), (cls3, "output_cls_layers", classes, h, w))):
        ops.append(_op("head", name, src, None, hh, ww, conv="pw", cout=co, slot=slot))
    return ops


def conv_names(H=64, W=64, classes=1):
    return [o.name for o in topology(H, W, classes) if o.kind == "conv"]


def named_tensors():
    return ["backbone.maxpool"] + ["backbone.stage%d.%d" % (si + 2, i) for si in range(3) for i in range(STAGE_REPEATS[si])] + ["fpn.p2"]


# ---- reading the record
def _gkey(key):
    return {"z": "dz:", "v": "g:", "y": "dy:"}[key[0]] + key.split(":", 1)[1]


def _view(rec, ref, grad=False):
    t = rec["x"] if ref.key == "x" else rec[_gkey(ref.key) if grad else ref.key]
    return t[:, ref.coff:ref.coff + ref.cstride * ref.C:ref.cstride].double()


class Report:
    """per kernel kind: the worst error / bound and where it occurred"""

    def __init__(self):
        self.worst = {}

    def add(self, kind, where, got, want, M=None, k=0, d=0, extra=None):
        got = got.double()
        assert got.shape == want.shape, (kind, where, got.shape, want.shape)
        err = (got - want).abs()
        if M is None:                       # an exact comparison
            ratio = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
        else:
            bound = (k * U + d * D) * M + (k + 1) * FLOOR
            if extra is not None:
                bound = bound + extra
            ratio = err / bound
        ratio = torch.where(torch.isnan(got) | torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        r = float(ratio.max()) if ratio.numel() else 0.0
        if kind not in self.worst or r > self.worst[kind][0]:
            idx = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape)) if ratio.numel() else ()
            self.worst[kind] = (r, "%s%s" % (where, list(idx)))

    def ratios(self):
        return {k: v[0] for k, v in self.worst.items()}

    def max(self):
        return max(v[0] for v in self.worst.values())

    def as_json(self):
        return {k: {"ratio": (round(v[0], 4) if v[0] != float("inf") else "inf"), "where": v[1]} for k, v in sorted(self.worst.items())}


def _conv(x, w, op, bias=None):
    return F.conv2d(x, w, bias, op.stride, op.pad, 1, op.groups)


def _conv_input_grad(shape, w, g, op):
    return torch.nn.grad.conv2d_input(shape, w, g, op.stride, op.pad, 1, op.groups)


def _conv_weight_grad(x, wshape, g, op):
    return torch.nn.grad.conv2d_weight(x, wshape, g, op.stride, op.pad, 1, op.groups)


def bn_backward64(y, z, dz, mean, invstd, gamma, relu):
    """BatchNorm's backward in float64 from recorded operands -> (dy, d gamma, d beta) and the abs-value sums of the three bounds"""
    n = y.shape[0] * y.shape[2] * y.shape[3]
    c = lambda v: v[None, :, None, None]  # noqa: E731
    g = dz * (z > 0) if relu else dz
    xh, xh_abs = (y - c(mean)) * c(invstd), (y.abs() + c(mean.abs())) * c(invstd)
    s0, s1 = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    a0, a1 = g.abs().sum((0, 2, 3)), (g.abs() * xh_abs).sum((0, 2, 3))
    dy = c(gamma * invstd) * (g - c(s0) / n - xh * c(s1) / n)
    m_dy = c((gamma * invstd).abs()) * (g.abs() + c(a0) / n + xh_abs * c(a1) / n)
    return dy, s1, s0, m_dy, a1, a0


def _pw_k(HW, B, cin, cout):
    return min(TC.pw_wgrad_launch(HW, B, cin, cout)[0], HW) + 2


def check(rec, H, W, classes, only=None, aten=False):
    """-> Report.  only: a set of op names / tensor keys to restrict the walk to (the mutant tests); aten: the record is ATen's (K_ATEN_EXTRA)"""
    rep = Report()

    def kk(kind, n, k=None):
        k = K[kind] if k is None else k
        extra = K_ATEN_EXTRA.get(kind, 0) if aten else 0
        return k + (n if extra == "n" else extra)

    ops = topology(H, W, classes)
    P = {k: v.double() for k, v in rec["param"].items()}
    G = rec["pgrad"]
    B = rec["x"].shape[0]
    want_op = lambda name: only is None or name in only  # noqa: E731
    c4 = lambda v: v[None, :, None, None]  # noqa: E731
    for op in ops:
        if op.kind == "head" or not want_op(op.name):
            continue
        if op.kind == "conv":
            x, w = _view(rec, op.src), P[op.name + ".weight"]
            y, z, dy, dz = (rec[p + op.name].double() for p in ("y:", "z:", "dy:", "dz:"))
            n = B * op.oh * op.ow
            # forward: the conv
            kind, k = {"stem": ("stem_fwd", K["stem_fwd"]), "pw": ("pw_fwd", op.cin + 1)}.get(op.conv, ("dw_fwd", op.k * op.k))
            rep.add(kind, "y:" + op.name, y, _conv(x, w, op), _conv(x.abs(), w.abs(), op), k)
            # forward: BatchNorm on the recorded y
            mean = y.mean((0, 2, 3))
            ey2 = (y * y).mean((0, 2, 3))
            var = ((y - c4(mean)) ** 2).mean((0, 2, 3))
            inv = 1.0 / torch.sqrt(var + BN_EPS)
            var_m = ey2 + mean * mean                       # E[y^2] - mean^2 on absolute values: what the kernel's double cancellation is relative to
            mean_r, inv_r = rec["mean:" + op.name].double(), rec["invstd:" + op.name].double()
            gam, bet = P[op.bn + ".weight"], P[op.bn + ".bias"]
            rep.add("bn_mean", "mean:" + op.name, mean_r, mean, y.abs().mean((0, 2, 3)), K["bn_mean"], n)
            rep.add("bn_invstd", "invstd:" + op.name, inv_r, inv, inv, K["bn_invstd"], extra=(n + 4) * D * 0.5 * inv * var_m / (var + BN_EPS))
            z64 = (y - c4(mean_r)) * c4(inv_r) * c4(gam) + c4(bet)
            rep.add("bn_apply", "z:" + op.name, z, z64.clamp(min=0) if op.relu else z64, (y.abs() + c4(mean_r.abs())) * c4((inv_r * gam).abs()) + c4(bet.abs()), kk("bn_apply", n))
            rm0, rv0 = rec["run_before"][op.bn + ".running_mean"].double(), rec["run_before"][op.bn + ".running_var"].double()
            unb = n / (n - 1.0)
            rep.add("bn_running_mean", op.bn + ".running_mean", rec["run_after"][op.bn + ".running_mean"], 0.9 * rm0 + 0.1 * mean,
                    0.9 * rm0.abs() + 0.1 * y.abs().mean((0, 2, 3)), kk("bn_running", n), n)
            rep.add("bn_running_var", op.bn + ".running_var", rec["run_after"][op.bn + ".running_var"], 0.9 * rv0 + 0.1 * var * unb,
                    0.9 * rv0.abs() + 0.1 * var_m * unb, kk("bn_running", n), n + 4)
            # backward: BatchNorm from the recorded y, output gradient and ReLU mask
            dy64, dgam, dbet, m_dy, m_dgam, m_dbet = bn_backward64(y, z, dz, mean_r, inv_r, gam, op.relu)
            rep.add("bn_bwd_dy", "dy:" + op.name, dy, dy64, m_dy, kk("bn_bwd_dy", n), n)
            rep.add("bn_dgamma", op.bn + ".weight", G[op.bn + ".weight"], dgam, m_dgam, kk("bn_dgamma", n), n)
            rep.add("bn_dbeta", op.bn + ".bias", G[op.bn + ".bias"], dbet, m_dbet, kk("bn_dbeta", n), n)
            # backward: the weight gradient from the recorded input and dy
            kind, k = (("pw_wgrad", kk("pw_wgrad", n, _pw_k(op.oh * op.ow, B, op.cin, op.cout))) if op.conv == "pw" else
                       (("stem_wgrad" if op.conv == "stem" else "dw_wgrad"), kk("chunk_wgrad", n)))
            rep.add(kind, op.name + ".weight", G[op.name + ".weight"], _conv_weight_grad(x, w.shape, dy, op), _conv_weight_grad(x.abs(), w.shape, dy.abs(), op), k, n)
        elif op.kind == "maxpool":
            rep.add("maxpool_fwd", op.dst.key, _view(rec, op.dst), F.max_pool2d(_view(rec, op.src), 3, 2, 1))
        elif op.kind in ("window", "pass"):
            rep.add("copy", "%s -> %s" % (op.src.key, op.dst.key), _view(rec, op.dst), _view(rec, op.src))
            if op.kind == "window":
                rep.add("copy", "%s <- %s" % (_gkey(op.src.key), _gkey(op.dst.key)), _view(rec, op.src, True), _view(rec, op.dst, True))
        elif op.kind == "upcat":
            c = op.src.C
            rep.add("copy", "upsample -> fpn.p2", rec["v:fpn.p2"][:, :c].double(), F.interpolate(_view(rec, op.src), scale_factor=2))
            rep.add("copy", "c2 -> fpn.p2", rec["v:fpn.p2"][:, c:].double(), _view(rec, op.src2))
    # the heads: logits per scale; bias and weight gradients summed over both scales, as the library does
    for name in ("output_reg_layers", "output_obj_layers", "output_cls_layers"):
        if not want_op(name):
            continue
        w, b = P[name + ".weight"], P[name + ".bias"]
        gw, gw_m, gb, gb_m, k, n = 0.0, 0.0, 0.0, 0.0, 0, 0
        for op in ops:
            if op.kind != "head" or op.name != name:
                continue
            x, g = _view(rec, op.src), rec["dlogits"][op.slot].double()
            rep.add("head_fwd", "logits[%d]" % op.slot, rec["logits"][op.slot], _conv(x, w, op, b), _conv(x.abs(), w.abs(), op, b.abs()), op.cin + 2)
            gw, gw_m = gw + _conv_weight_grad(x, w.shape, g, op), gw_m + _conv_weight_grad(x.abs(), w.shape, g.abs(), op)
            gb, gb_m = gb + g.sum((0, 2, 3)), gb_m + g.abs().sum((0, 2, 3))
            k, n = max(k, _pw_k(op.oh * op.ow, B, op.cin, op.cout)), n + B * op.oh * op.ow
        rep.add("head_wgrad", name + ".weight", G[name + ".weight"], gw, gw_m, kk("pw_wgrad", n, k), n)
        rep.add("head_bias_grad", name + ".bias", G[name + ".bias"], gb, gb_m, kk("head_bias", n), n)
    # the gradient of every tensor with consumers: the float64 sum of its consumers' contributions, each from that consumer's recorded
    # output gradient; bound = the consumers' bounds plus one rounding of the running total per accumulation
    consumers = collections.OrderedDict()
    for op in ops:
        if op.kind != "window" and op.src.key != "x":
            consumers.setdefault(op.src.key, []).append((op, op.src))
        if op.kind == "upcat":
            consumers.setdefault(op.src2.key, []).append((op, op.src2))
    for key, users in consumers.items():
        if not want_op(key):
            continue
        got = rec[_gkey(key)].double()
        total, bound_km, m_sum, kinds = torch.zeros_like(got), torch.zeros_like(got), torch.zeros_like(got), set()
        for op, ref in users:
            sl = (slice(None), slice(ref.coff, ref.coff + ref.cstride * ref.C, ref.cstride))
            shape = got[sl].shape
            if op.kind in ("conv", "head"):
                w = P[op.name + ".weight"]
                g = rec["dlogits"][op.slot].double() if op.kind == "head" else rec["dy:" + op.name].double()
                c, m = _conv_input_grad(shape, w, g, op), _conv_input_grad(shape, w.abs(), g.abs(), op)
                k = op.cout + 1 if op.conv == "pw" else op.k * op.k
                kinds.add("pw" if op.conv == "pw" else "dw")
            elif op.kind == "pass":
                c = _view(rec, op.dst, True)
                m, k = c.abs(), K["copy"]
                kinds.add("pass")
            elif op.kind == "upcat":
                gp2 = rec["g:fpn.p2"].double()
                if ref is op.src:
                    c, m, k = 4 * F.avg_pool2d(gp2[:, :ref.C], 2), 4 * F.avg_pool2d(gp2[:, :ref.C].abs(), 2), K["upsample_bwd"]
                else:
                    c, k = gp2[:, op.src.C:], K["copy"]
                    m = c.abs()
                kinds.add("upcat")
            else:                                           # maxpool: the FIRST maximum of each window keeps the gradient (ATen's scan order)
                gout = _view(rec, op.dst, True)
                _, idx = F.max_pool2d(_view(rec, op.src), 3, 2, 1, return_indices=True)
                flat = lambda v: v.reshape(v.shape[0], v.shape[1], -1)  # noqa: E731
                c = torch.zeros(shape, dtype=torch.float64)
                m = torch.zeros(shape, dtype=torch.float64)
                flat(c).scatter_add_(2, flat(idx), flat(gout))
                flat(m).scatter_add_(2, flat(idx), flat(gout.abs()))
                k = K["maxpool_bwd"]
                kinds.add("maxpool")
            total[sl] += c
            bound_km[sl] += k * m
            m_sum[sl] += m
        # (k_c u M_c summed) + (accumulations) u (sum of M_c): expressed as k = 1 on a combined M
        rep.add("dgrad:" + "+".join(sorted(kinds)), _gkey(key), got, total, bound_km + K["accumulate"] * len(users) * m_sum, 1)
    return rep


def device_record(model, eng, x, logits, dlogits, run_before, H, W, classes):
    """the run record of one device iteration: `model` after forward + backward (its .grad = what the caller sees), the arenas read
    back through Engine.debug_train_tensor"""
    B = x.shape[0]
    rec = {"x": x.detach().cpu(), "logits": [p.detach().cpu() for p in logits], "dlogits": [g.detach().cpu() for g in dlogits],
           "param": {k: p.detach().cpu() for k, p in model.named_parameters()}, "pgrad": {k: p.grad.detach().cpu() for k, p in model.named_parameters()},
           "run_before": run_before, "run_after": {k: v.detach().cpu() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}}
    for op in topology(H, W, classes):
        if op.kind == "conv":
            shape = (B, op.cout, op.oh, op.ow)
            for key, which in (("y:", "y"), ("z:", "out"), ("dy:", "grad_y"), ("dz:", "grad_out")):
                rec[key + op.name] = eng.debug_train_tensor(op.name, which).reshape(shape)
            rec["mean:" + op.name], rec["invstd:" + op.name] = eng.debug_train_tensor(op.name, "mean"), eng.debug_train_tensor(op.name, "invstd")
        elif op.kind in ("maxpool", "upcat") or (op.kind == "window" and op.dst.coff > 0):
            name = op.dst.key[2:]
            shape = (B, {"maxpool": 24, "upcat": op.dst.C}.get(op.kind, op.dst.coff + op.dst.C), op.oh, op.ow)
            rec["v:" + name], rec["g:" + name] = eng.debug_train_tensor(name, "out").reshape(shape), eng.debug_train_tensor(name, "grad_out").reshape(shape)
    return rec
