"""The Python owner of one C-ABI handle, and the small ctypes helpers every module of the binding shares.

The five handle families of include/eamm_hip.h (``_lib.FAMILIES``: generator, key-point detector, emotion detector, audio
network, deconvolution tail) share one lifecycle -- create, load every tensor, finalise, then last_error and destroy -- which
api_common.h writes once for the library and ``Handle`` writes once for Python.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Tuple

import torch

from . import _lib


def ptr(t: Optional[torch.Tensor], entry: Optional[str] = None, operand: Optional[int] = None):
    """Tensor or None -> its address as a ``c_void_p``, or None (a NULL argument).  The ONE place where the binding turns a tensor
    into an address: ``_op.call`` and the BatchNorm calls convert here and say which ``entry`` and which of its C arguments
    (``operand``, counted from 0) the address is for.  Nothing is checked here -- the public wrappers refuse a wrong dtype or device
    and copy what is strided or off a 16-byte boundary (``_op.operands``, ``_op.dense``) -- but tests/calling.py replaces this
    function to look at every tensor before the library does."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None, stream: Optional[torch.cuda.Stream] = None) -> C.c_void_p:
    """The hipStream_t of ``stream``, by default the current stream of ``device`` (None: of the current device)."""
    return C.c_void_p((torch.cuda.current_stream(device) if stream is None else stream).cuda_stream)


def weights_key(tensors: Iterable[torch.Tensor]) -> tuple:
    """Identity AND version counter of every tensor: what a handle's loaded weights are keyed on.  An in-place write bumps the
    counter; a replaced tensor may carry the same counter as the one it replaces, but not its identity."""
    return tuple((id(t), t._version) for t in tensors)


def refuse_silent_detach(mod: torch.nn.Module, x: torch.Tensor):
    """For the modules that are inference-only (no backward kernels: SURVEY.md 8f N1 / N3 are forward rows; their parameters are
    frozen at construction).  If the caller nevertheless asks for a gradient -- gradients enabled and the input or a
    re-enabled parameter requires one -- the reference would return a differentiable tensor; returning a detached one
    would silently train nothing, so refuse instead."""
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in mod.parameters())):
        raise RuntimeError(f"eamm_amd.{type(mod).__name__} is inference-only (forward kernels, no backward): call it under "
                           "torch.no_grad() / with frozen parameters and an input that does not require grad; it never "
                           "returns a silently detached tensor")


class Handle:
    """One handle of the family named by its symbol prefix (``"eamm_kp_"``: eamm_kp_create, eamm_kp_load_tensor, ...).

    ``Handle(prefix, config_struct, device)`` creates it, ``load`` gives it its weights (two steps: the generator switches a
    fresh handle to training mode in between), ``call`` runs one of the family's entries on it, ``close`` destroys it.  ``ptr``
    is the raw ``c_void_p`` (None once closed) for callers that bind the entry themselves."""

    def __init__(self, prefix: str, config: C.Structure, device):
        self.prefix = prefix
        self.device = torch.device(device)
        self.ptr: Optional[C.c_void_p] = None
        self._L = _lib.lib()
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        ctx = C.c_void_p()
        self._check(self._fn("create")(C.byref(config), index, C.byref(ctx)))   # (no handle yet: the family's last_error(NULL))
        self.ptr = ctx

    def _fn(self, name: str):
        return getattr(self._L, self.prefix + name)

    def _check(self, code: int):
        if code != _lib.EAMM_OK:
            msg = self._fn("last_error")(self.ptr)
            raise _lib.EammError(code, msg.decode() if msg else "?")

    def load(self, named_tensors: Iterable[Tuple[str, torch.Tensor]]):
        """``(name, tensor)`` pairs (a state dict's items) -> host float32 copies -> load_tensor, then finalize_weights on the
        handle's device.  A handle whose load failed is destroyed before the error propagates."""
        try:
            load_tensor = self._fn("load_tensor")
            for name, t in named_tensors:
                if name.endswith("num_batches_tracked"):
                    continue
                host = t.detach().to("cpu", torch.float32).contiguous()
                shape = (C.c_int64 * max(1, host.dim()))(*host.shape)
                self._check(load_tensor(self.ptr, name.encode(), C.c_void_p(host.data_ptr()), shape, host.dim()))
            with torch.cuda.device(self.device):
                self._check(self._fn("finalize_weights")(self.ptr))
        except BaseException:
            self.close()
            raise

    def call(self, name: str, *args):
        """``<prefix><name>(handle, *args)`` on the handle's device; a non-zero return raises with the family's last error."""
        with torch.cuda.device(self.device):
            self._check(self._fn(name)(self.ptr, *args))

    def close(self):
        if self.ptr is not None:
            ctx, self.ptr = self.ptr, None
            self._fn("destroy")(ctx)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HandleOwner:
    """Mixin of the inference-only modules: the cached ``Handle`` their forward runs on, rebuilt when its key (device, geometry,
    ``weights_key`` of the tensors the module loads) changes or a batch outgrows its capacity."""
    _prefix = ""
    _handle: Optional[Handle] = None
    _key = None
    _cap = 0

    def _inference_device(self, param: torch.Tensor) -> torch.device:
        if param.device.type != "cuda":
            raise RuntimeError(f"eamm_amd.{type(self).__name__} runs only on a ROCm GPU (no CPU fallback): call .cuda()")
        if self.training:
            raise RuntimeError("inference-only: call .eval() (BatchNorm uses running statistics)")
        return param.device

    def _has_handle(self, key, batch: int = 0) -> bool:
        return self._handle is not None and self._handle.ptr is not None and self._key == key and batch <= self._cap

    def _rebuild_handle(self, key, cap: int, config: C.Structure, device, named_tensors):
        if self._handle is not None:
            self._handle.close()
            self._handle = None
        h = Handle(self._prefix, config, device)
        h.load(named_tensors)
        self._handle, self._key, self._cap = h, key, cap
