"""The one way Python calls a handle-less operator entry (``eamm_op_*``, or ``eamm_disc_*`` / ``eamm_equi_*`` with ``family="disc"`` / ``"equi"``;
include/eamm_hip.h): every entry takes the device index
first and the stream last, a workspace-taking one its ``(workspace, workspace_floats)`` pair in front of the stream, and reports
through ``eamm_last_error(NULL)``.  The handle families go through ``_handle.Handle`` instead."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._handle import ptr, stream_ptr

CHANNEL_GRANULE = 32   # channel granule of the convolution kernels (conv_common.h CONV_BK)
_PLAIN = frozenset((int, float, type(None)))   # most arguments: passed on without the (slower) tensor test


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def need_gpu(t: torch.Tensor, module: str, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"eamm_amd.{module}.{what} runs only on a ROCm GPU (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: float32 tensors only, got {t.dtype}")


def call(name: str, dev: torch.device, *args, work: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
         family: str = "op"):
    """``eamm_<family>_<name>(dev.index, *args[, work, work.numel()], stream)`` on ``dev``: tensors (and None) among ``args`` are passed
    by address, everything else as it is; ``stream`` defaults to the current stream of ``dev``.  Enqueues only; a non-zero return
    raises ``EammError`` with the library's message."""
    argv = [a if type(a) in _PLAIN else C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    if work is not None:
        argv += (ptr(work), work.numel())
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), f"eamm_{family}_{name}")(dev.index, *argv, stream_ptr(dev, stream)), None)


def workspace(name: str, dev: torch.device, *dims: int, family: str = "op") -> torch.Tensor:
    """An uninitialised workspace of ``eamm_<family>_<name>_workspace_floats(*dims)`` floats on ``dev`` (one float where that is 0: the
    entry then refuses the shape itself)."""
    n = getattr(_lib.lib(), f"eamm_{family}_{name}_workspace_floats")(*dims)
    return torch.empty(max(1, n), dtype=torch.float32, device=dev)
