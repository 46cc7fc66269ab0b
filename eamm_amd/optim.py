"""``eamm_amd.Adam``: the optimiser of every stage of the reference's ``train.py`` (``torch.optim.Adam(params, lr=..., betas=(0.5, 0.999))``)
with its step on the multi-tensor HIP kernel (csrc/optim.hip through ``optim_ops.adam_step``): per param group and device ONE library
call over every parameter that has a gradient, which reads p, g, m, v once and writes p, m, v once.

It IS a ``torch.optim.Adam``: the constructor's checks, ``state_dict`` / ``load_state_dict``, ``add_param_group``, ``zero_grad`` and the
hooks are torch's, so every learning-rate scheduler works unchanged (``lr`` is read from the group at each step).  The state is torch's
default layout -- per parameter ``step`` (a float32 scalar on the CPU), ``exp_avg`` and ``exp_avg_sq`` in the parameter's memory format
-- so a ``state_dict`` moves between the two classes in both directions and training continues on either.

Parameters on the CPU take torch's own single-tensor Adam (bit-identical to ``torch.optim.Adam(foreach=False)``); on a GPU only float32
parameters are served.  What the kernel does not do is refused by name: ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``,
``decoupled_weight_decay``, a tensor ``lr``, sparse gradients.  ``foreach`` and ``fused`` select among torch's implementations; this is
another one, and they are accepted and ignored.  ``weight_decay`` is torch.optim.Adam's L2 term (not AdamW)."""
from __future__ import annotations

import inspect

import torch
from torch.optim import adam as _torch_adam

from . import optim_ops

_REFUSED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")
_ADAM_TAKES = frozenset(inspect.signature(_torch_adam.adam).parameters)


def _refuse(group: dict):
    for flag in _REFUSED_FLAGS:
        if group.get(flag, False):
            raise ValueError(f"eamm_amd.Adam: {flag}=True is not supported (the HIP step is plain Adam; use torch.optim.Adam for it)")
    if isinstance(group["lr"], torch.Tensor):
        raise ValueError("eamm_amd.Adam: lr as a tensor is not supported: the step size is computed on the host, pass a Python float")


def _refuse_dtype(p: torch.Tensor):
    raise ValueError(f"eamm_amd.Adam: a parameter of dtype {p.dtype} on {p.device}: on a GPU only float32 parameters are supported")


_OTHER_DEVICES = {}      # the CPU and whatever else is not a GPU -> a bucket number (those parameters take torch's own Adam)


class Adam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _refuse(dict(lr=lr, amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable,
                     decoupled_weight_decay=decoupled_weight_decay))
        del foreach, fused            # torch's own implementations; the groups keep torch's defaults for both
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._step_buffers = {}

    def __setstate__(self, state):
        super().__setstate__(state)   # (also what load_state_dict ends with: the state tensors are new ones)
        self._step_buffers = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        states = self.state
        for group in self.param_groups:
            _refuse(group)
            beta1, beta2 = (float(b) for b in group["betas"])
            buckets, last, bucket = {}, None, None      # device index (-1: the CPU) -> [(parameter, gradient, state)]
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue          # as torch: no update, and its step does not advance
                state = states[p]
                if not state:
                    if p.is_cuda and p.dtype != torch.float32:
                        _refuse_dtype(p)
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                index = p.get_device() if p.is_cuda else -1 - _OTHER_DEVICES.setdefault(p.device, len(_OTHER_DEVICES))
                if index != last:
                    last, bucket = index, buckets.setdefault(index, [])
                bucket.append((p, g, state))
            for index, bucket in buckets.items():
                params, grads = [b[0] for b in bucket], [b[1] for b in bucket]
                if any(g.is_sparse for g in grads):
                    raise ValueError("eamm_amd.Adam: sparse gradients are not supported (torch.optim.SparseAdam serves them)")
                if index >= 0:
                    self._hip_step(group, index, params, grads, [b[2] for b in bucket], beta1, beta2)
                else:
                    extra = {"decoupled_weight_decay": False} if "decoupled_weight_decay" in _ADAM_TAKES else {}
                    _torch_adam.adam(params, grads, [b[2]["exp_avg"] for b in bucket], [b[2]["exp_avg_sq"] for b in bucket], [],
                                     [b[2]["step"] for b in bucket], foreach=False, capturable=False, differentiable=False, fused=False,
                                     grad_scale=None, found_inf=None, has_complex=any(torch.is_complex(p) for p in params), amsgrad=False,
                                     beta1=beta1, beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"],
                                     maximize=False, **extra)
        return loss

    def _hip_step(self, group, index, params, grads, states, beta1, beta2):
        """One library call for the group's parameters on GPU ``index``.  Their ``step`` scalars are views of ONE CPU buffer per group
        and device, so that a step advances them with one addition; the buffer is made (and the states are looked at: dtype, layout,
        where ``step`` lives) whenever the set of step tensors is not the one of the last call -- the first step, a state that
        ``load_state_dict`` replaced, a parameter that joins or sits out."""
        steps = [st["step"] for st in states]
        ids = [id(s) for s in steps]
        cached = self._step_buffers.get((id(group), index))
        if cached is None or cached[0] != ids:
            for p, st in zip(params, states):
                if p.dtype != torch.float32:
                    _refuse_dtype(p)
                for key in ("exp_avg", "exp_avg_sq"):        # a state loaded in another layout or from another device
                    t = st[key]
                    if t.device != p.device or t.dtype != p.dtype or (t.stride() != p.stride() and not (t.is_contiguous() and p.is_contiguous())):
                        st[key] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(t)
            buffer = torch.tensor([float(s) for s in steps], dtype=torch.float32)
            views = list(buffer.unbind(0))
            for st, view in zip(states, views):
                st["step"] = view
            cached = self._step_buffers[(id(group), index)] = ([id(v) for v in views], buffer, views)
        buffer = cached[1]
        buffer += 1
        optim_ops.adam_step(params, grads, [st["exp_avg"] for st in states], [st["exp_avg_sq"] for st in states], buffer.tolist(),
                            lr=group["lr"], betas=(beta1, beta2), eps=group["eps"], weight_decay=group["weight_decay"])
