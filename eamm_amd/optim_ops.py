"""The optimiser step as an operator on libeamm_hip.so (csrc/optim.hip; C ABI ``eamm_optim_adam``): Adam over LISTS of float32 tensors
on one GPU, the whole list in a few launches (one per ``table_capacity()`` tensors).

* ``adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, *, lr, betas, eps, weight_decay)``  the functional form, as
  ``torch.optim.adam.adam`` for the default arguments of ``torch.optim.Adam``: ``params``, ``exp_avgs`` and ``exp_avg_sqs`` are updated
  in place, ``grads`` are only read.  ``steps`` are the step numbers AFTER this step's increment, one per tensor (parameters that
  received gradients in different steps carry different ones); ``lr / (1 - beta1**step)`` and ``sqrt(1 - beta2**step)`` are computed
  here in Python floats, as torch computes them, and handed over as fp32.

A parameter may be any non-overlapping dense tensor (contiguous, ``channels_last``, a transposed weight): it is updated in storage order,
so its two moments must share its strides (``torch.zeros_like(p, memory_format=torch.preserve_format)`` does); a gradient laid out
differently is copied once into the parameter's layout.  Addresses need 4-byte alignment only: a view that starts off a 16-byte boundary
is updated where it is, one float at a time.  Enqueues on the current stream; allocates only those gradient copies.  GPU only: no CPU
fallback (``eamm_amd.Adam`` hands CPU parameters to torch)."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import torch

from . import _lib, _op

_MODULE = "optim_ops"
_FAMILY = "optim"


def table_capacity() -> int:
    """Tensors per launch (csrc/kernels.h ADAM_TABLE)."""
    return _lib.lib().eamm_optim_adam_table_capacity()


def block_elems() -> int:
    """E, the elements of one workgroup's chunk (csrc/kernels.h ADAM_BLOCK_ELEMS); a launch of very many chunks uses a multiple."""
    return _lib.lib().eamm_optim_adam_block_elems()


def plan(numels: Sequence[int]) -> Tuple[List[Tuple[int, int, int]], List[int]]:
    """How ``eamm_optim_adam`` cuts a list of lengths into launches (host only, no GPU): ``([(first tensor, tensor count, workgroups)],
    [elements per workgroup of every tensor])``."""
    n = len(numels)
    lengths = (C.c_longlong * max(1, n))(*numels)
    per_block = (C.c_longlong * max(1, n))()
    cap = n // table_capacity() + 1
    first, count, blocks = ((C.c_int * cap)() for _ in range(3))
    made = _lib.lib().eamm_optim_adam_plan(n, lengths, cap, first, count, blocks, per_block)
    if made < 0:
        _lib.check(made, None)
    assert made <= cap, (made, cap)
    return [(first[i], count[i], blocks[i]) for i in range(made)], list(per_block[:n])


def _dense(t: torch.Tensor) -> bool:
    """Non-overlapping and dense: the tensor's elements fill ``numel`` consecutive floats of its storage, in some order of its dimensions."""
    expect = 1
    for stride, size in sorted((t.stride(d), t.shape[d]) for d in range(t.dim()) if t.shape[d] != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def _in_the_parameters_layout(params, grads, exp_avgs, exp_avg_sqs) -> list:
    """The per-tensor checks behind ``adam_step``'s fast path: shapes equal, parameters dense, moments in the parameter's strides.
    Returns the gradients, those laid out differently copied into their parameter's layout."""
    grads = list(grads)
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        if not (g.shape == p.shape and m.shape == p.shape and v.shape == p.shape):
            raise ValueError(f"adam_step: tensor {i}: grads / exp_avgs / exp_avg_sqs must have the parameter's shape {tuple(p.shape)}, got "
                             f"{tuple(g.shape)}, {tuple(m.shape)}, {tuple(v.shape)}")
        if p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous():
            continue
        if not _dense(p):
            raise ValueError(f"adam_step: params[{i}] is not a dense tensor (shape {tuple(p.shape)}, strides {p.stride()}): it is updated "
                             "in storage order")
        if m.stride() != p.stride() or v.stride() != p.stride():
            raise ValueError(f"adam_step: exp_avgs[{i}] / exp_avg_sqs[{i}] must share the strides {p.stride()} of params[{i}], got "
                             f"{m.stride()} and {v.stride()}")
        if g.stride() != p.stride():
            grads[i] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
    return grads


def adam_step(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
              exp_avg_sqs: Sequence[torch.Tensor], steps: Sequence[float], *, lr: float, betas: Tuple[float, float] = (0.9, 0.999),
              eps: float = 1e-8, weight_decay: float = 0.0) -> None:
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(steps) == n):
        raise ValueError(f"adam_step: params, grads, exp_avgs, exp_avg_sqs and steps must be lists of one length, got {n}, {len(grads)}, "
                         f"{len(exp_avgs)}, {len(exp_avg_sqs)}, {len(steps)}")
    if n == 0:
        return
    if isinstance(lr, torch.Tensor):
        raise ValueError("adam_step: lr must be a Python number, not a tensor")
    beta1, beta2 = float(betas[0]), float(betas[1])
    lists = (params, grads, exp_avgs, exp_avg_sqs)
    # one pass per property over the 4 n tensors: the common case -- float32, one GPU, contiguous, equal lengths -- costs a few method
    # calls per tensor; anything else goes through the checks that name what they refuse
    index = params[0].get_device()
    numels = [t.numel() for t in params]
    float32 = torch.float32
    if index < 0 or not all(t.dtype is float32 and t.get_device() == index for ts in lists for t in ts):
        _op.operands(_MODULE, "adam_step", *params, *grads, *exp_avgs, *exp_avg_sqs)
    if not all(t.is_contiguous() for ts in lists for t in ts) or any([t.numel() for t in ts] != numels for ts in lists[1:]):
        grads = _in_the_parameters_layout(*lists)
    factors = {}
    step_size, bc2_sqrt = (C.c_float * n)(), (C.c_float * n)()
    for i, step in enumerate(steps):
        f = factors.get(step)
        if f is None:
            step = float(step)
            if not step >= 1:
                raise ValueError(f"adam_step: steps[{i}] = {step}: the step number after this step's increment is at least 1")
            f = factors[step] = (lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5)     # torch's Python-float expressions
        step_size[i], bc2_sqrt[i] = f
    addresses = C.c_void_p * n
    _op.call("adam", params[0].device, n, addresses(*[t.data_ptr() for t in params]), addresses(*[t.data_ptr() for t in grads]),
             addresses(*[t.data_ptr() for t in exp_avgs]), addresses(*[t.data_ptr() for t in exp_avg_sqs]),
             (C.c_longlong * n)(*numels), step_size, bc2_sqrt, beta1, beta2, float(eps), float(weight_decay),
             family=_FAMILY)
    # the kernel wrote behind torch's back: what is keyed on a tensor's version counter (a module's inference engine caches its folded
    # weights on it, autograd checks saved tensors against it) has to see an in-place write
    for tensors in (params, exp_avgs, exp_avg_sqs):
        torch.autograd.graph.increment_version(tensors)
