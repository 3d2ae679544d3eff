"""torch.optim.SGD as train.py:81-85 builds it (momentum 0.949, weight_decay 0.0005, dampening 0, no Nesterov), stepping the
parameters with libyfv2's SGD kernel: d = g + wd p; buf = d (first step) | momentum buf + d; p -= lr buf.
A ``torch.optim.Optimizer`` subclass, so ``param_groups`` (train.py:113-117 rewrites ``lr`` during the warm-up) and
``torch.optim.lr_scheduler.MultiStepLR`` (train.py:88-90) work on it unchanged.  All tensors of a parameter group travel in one
table (``yfv2_sgd_step_multi``): three launches for the network's 225 tensors instead of 225."""
import torch

from .. import _lib
from ..engine import get_engine


def _order(t):
    """(stride, size) of the dimensions that move the address (size > 1), innermost first"""
    return sorted((st, n) for n, st in zip(t.shape, t.stride()) if n > 1)


def _dense(t):
    """True if the elements of ``t`` fill numel() consecutive addresses from data_ptr(), each exactly once"""
    expect = 1
    for st, n in _order(t):
        if st != expect:
            return False
        expect *= n
    return True


def _same_order(a, b):
    """True if element [i, j, ...] of ``a`` and of ``b`` sit at the same offset from their data_ptr()"""
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _laid_out_like(p):
    return torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device)


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("lr, momentum and weight_decay must be >= 0")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        # kernel-argument tables, one per parameter group, keyed by the group's position.  Kept OFF param_groups: state_dict()
        # copies every non-'params' key of a group, and a ctypes array of pointers can be neither pickled (torch.save of the
        # optimizer state) nor deep-copied
        self._yfv2_tables = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            todo = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda" or p.dtype != torch.float32:
                    raise RuntimeError("yolo_fastestv2_amd.SGD steps fp32 parameters on the MI355X only")
                st = self.state[p]
                first = "momentum_buffer" not in st
                # the kernel walks numel() elements from each data_ptr(): parameter, gradient and buffer must share ONE memory
                # order.  A contiguous parameter (every tensor of the Detector) takes the row-major one; a dense parameter in
                # another order (a channels_last conv weight, a transposed matrix) lends its own strides to the other two
                if p.is_contiguous():
                    if first:
                        st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    elif not st["momentum_buffer"].is_contiguous():
                        st["momentum_buffer"] = st["momentum_buffer"].contiguous()
                    g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                else:
                    if not _dense(p):
                        raise RuntimeError("yolo_fastestv2_amd.SGD steps dense parameters only: shape %s with strides %s leaves gaps or overlaps"
                                           % (tuple(p.shape), tuple(p.stride())))
                    if first:
                        st["momentum_buffer"] = _laid_out_like(p).zero_()
                    elif not _same_order(st["momentum_buffer"], p):
                        st["momentum_buffer"] = _laid_out_like(p).copy_(st["momentum_buffer"])
                    g = p.grad if _same_order(p.grad, p) else _laid_out_like(p).copy_(p.grad)
                todo.append((p, g, st["momentum_buffer"], first))
            if not todo:
                continue
            # the table is rebuilt only when a pointer in it changed (gradients that are views of the Detector's persistent
            # bucket keep their addresses from step to step)
            key = tuple((p.data_ptr(), g.data_ptr(), b.data_ptr(), first) for p, g, b, first in todo)
            cache = self.__dict__.setdefault("_yfv2_tables", {}).setdefault(gi, {})
            if cache.get("key") != key:
                items = (_lib.SgdItem * len(todo))()
                for i, (p, g, b, first) in enumerate(todo):
                    items[i].param, items[i].grad, items[i].momentum_buf = p.data_ptr(), g.data_ptr(), b.data_ptr()
                    items[i].n, items[i].first_step = p.numel(), 1 if first else 0
                cache["key"], cache["items"] = key, items
            dev = todo[0][0].device
            eng = get_engine(dev, 32, 32, 1, 3)          # any handle of the device: the kernel only needs its error slot
            eng.sgd_step_multi(cache["items"], group["lr"], group["momentum"], group["weight_decay"])
            # the kernel wrote through the raw pointers: move the autograd version counters as an in-place torch op would, so
            # that Detector.engine_for() sees the change and re-packs the inference weights on the next eval forward.  The call
            # takes an ITERABLE of tensors: handed one tensor it walks that tensor's rows (a Python-level view per row - seconds
            # for a long vector - and a RuntimeError for a 0-d parameter)
            torch._C._increment_version([p for p, _, _, _ in todo])
        return loss
