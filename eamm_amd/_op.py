"""The one way Python calls a handle-less operator entry (``eamm_op_*``, or ``eamm_disc_*`` / ``eamm_equi_*`` with ``family="disc"`` / ``"equi"``;
include/eamm_hip.h): every entry takes the device index
first and the stream last, a workspace-taking one its ``(workspace, workspace_floats)`` pair in front of the stream, and reports
through ``eamm_last_error(NULL)``.  The handle families go through ``_handle.Handle`` instead.

What a public wrapper does with its tensor operands before they get here: ``operands`` refuses a wrong dtype or device by name,
``dense`` copies what is strided or starts off a 16-byte boundary ("The calling contract of the operators")."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _handle, _lib
from ._handle import ptr, stream_ptr   # noqa: F401  (importable from here)

CHANNEL_GRANULE = 32   # channel granule of the convolution kernels (conv_common.h CONV_BK)
ALIGN = 16             # bytes: the alignment include/eamm_hip.h documents for every tensor (the kernels access four floats at a time)
_PLAIN = frozenset((int, float, type(None)))   # most arguments: passed on without the (slower) tensor test


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def need_gpu(t: torch.Tensor, module: str, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"eamm_amd.{module}.{what} runs only on a ROCm GPU (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: float32 tensors only, got {t.dtype}")


def operands(module: str, what: str, *tensors: Optional[torch.Tensor]):
    """Every tensor operand of operator ``what`` (None: an absent one) is float32 on one GPU, or the call is refused by name: a
    kernel reads an address as float32 whatever the tensor behind it holds."""
    first = None
    for t in tensors:
        if t is None:
            continue
        need_gpu(t, module, what)
        if first is None:
            first = t
        elif t.device != first.device:
            raise RuntimeError(f"{what}: every tensor operand must be on one device, got {first.device} and {t.device}")


def dense(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """``t`` as the library takes a tensor: contiguous and starting on a 16-byte boundary.  ``t`` itself where it is both (every
    tensor that owns its allocation), else a copy -- ``.contiguous()`` alone returns a contiguous view as it is, wherever it starts."""
    if t is None:
        return None
    t = t.contiguous()
    return t if t.data_ptr() % ALIGN == 0 else t.clone(memory_format=torch.contiguous_format)


def call(name: str, dev: torch.device, *args, work: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
         family: str = "op"):
    """``eamm_<family>_<name>(dev.index, *args[, work, work.numel()], stream)`` on ``dev``: tensors (and None) among ``args`` are passed
    by address, everything else as it is; ``stream`` defaults to the current stream of ``dev``.  Enqueues only; a non-zero return
    raises ``EammError`` with the library's message."""
    entry = f"eamm_{family}_{name}"
    to_address = _handle.ptr      # (looked up per call: the one conversion point, which tests/calling.py replaces)
    argv = [a if type(a) in _PLAIN else to_address(a, entry, i + 1) if isinstance(a, torch.Tensor) else a for i, a in enumerate(args)]
    if work is not None:
        argv += (to_address(work, entry, len(args) + 1), work.numel())
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), entry)(dev.index, *argv, stream_ptr(dev, stream)), None)


def workspace(name: str, dev: torch.device, *dims: int, family: str = "op") -> torch.Tensor:
    """An uninitialised workspace of ``eamm_<family>_<name>_workspace_floats(*dims)`` floats on ``dev`` (one float where that is 0: the
    entry then refuses the shape itself)."""
    n = getattr(_lib.lib(), f"eamm_{family}_{name}_workspace_floats")(*dims)
    return torch.empty(max(1, n), dtype=torch.float32, device=dev)
