"""``optim.Adam`` / ``optim.SGD`` as one multi-tensor launch per parameter group (``csrc/step.hip``).

    opt = FusedAdam(net.parameters(), lr=1e-3)       # drop-in for optim.Adam (PLTrainer.py:171-174)

There is no CPU fallback: parameters and gradients must be contiguous fp32 on a ROCm device.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Dict, List, Optional

import torch

from . import _lib
from ._args import _p, _require_cuda, _stream
from .engine import bump_param_epoch


def _ptr_array(ts: List[Optional[torch.Tensor]]):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (amsgrad/maximize off -- the reference uses the
    defaults, PLTrainer.py:171-174) with every parameter tensor of a group updated by ONE kernel launch.
    ``grad_scale``: optional device scalar multiplied into the gradients (e.g. 1/world_size)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("FusedAdam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                _require_cuda(p, "parameter")
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or not p.is_contiguous():
                    raise RuntimeError("FusedAdam: parameters and gradients must be contiguous fp32")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            by_step: Dict[int, List[torch.Tensor]] = OrderedDict()
            for p in ps:
                self.state[p]["step"] += 1
                by_step.setdefault(self.state[p]["step"], []).append(p)
            b1, b2 = group["betas"]
            for step, plist in by_step.items():
                with torch.cuda.device(plist[0].device):
                    n = (ctypes.c_longlong * len(plist))(*[p.numel() for p in plist])
                    _lib.call("hpri_adam_step", _ptr_array(plist), _ptr_array([p.grad for p in plist]),
                              _ptr_array([self.state[p]["exp_avg"] for p in plist]),
                              _ptr_array([self.state[p]["exp_avg_sq"] for p in plist]), n, len(plist),
                              float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                              int(step), _p(grad_scale), _stream())
        bump_param_epoch()      # parameters were written through raw pointers: packed-weight caches are stale
        return loss


class FusedSGD(torch.optim.Optimizer):
    """``torch.optim.SGD(params, lr, momentum, weight_decay)`` (dampening 0, no Nesterov; PLTrainer.py:176-180)."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, weight_decay: float = 0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("FusedSGD: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            mom = float(group["momentum"])
            fresh, old = [], []
            for p in ps:
                _require_cuda(p, "parameter")
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or not p.is_contiguous():
                    raise RuntimeError("FusedSGD: parameters and gradients must be contiguous fp32")
                st = self.state[p]
                if mom != 0.0 and "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)
                    fresh.append(p)
                else:
                    old.append(p)
            for first, plist in ((1, fresh), (0, old)):
                if not plist:
                    continue
                with torch.cuda.device(plist[0].device):
                    n = (ctypes.c_longlong * len(plist))(*[p.numel() for p in plist])
                    bufs = _ptr_array([self.state[p]["momentum_buffer"] for p in plist]) if mom != 0.0 else None
                    _lib.call("hpri_sgd_step", _ptr_array(plist), _ptr_array([p.grad for p in plist]), bufs, n, len(plist),
                              float(group["lr"]), mom, float(group["weight_decay"]), first, _p(grad_scale), _stream())
        bump_param_epoch()
        return loss
