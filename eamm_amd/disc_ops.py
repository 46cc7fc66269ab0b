"""The discriminator's operators (reference modules/discriminator.py:7-33) -- ``torch.autograd.Function``s whose forward AND backward
are libeamm_hip.so kernels (csrc/disc_conv4.hip, csrc/disc_norm.hip; C ABI ``eamm_disc_conv4``, ``eamm_disc_conv4_wgrad``,
``eamm_disc_norm_act_pool`` and ``eamm_disc_norm_act_pool_backward``), on NHWC fp32 tensors.

* ``conv4_valid(x, weight, bias)``                 ``F.conv2d(x, weight, bias)`` with a 4x4 filter, no padding, stride 1: x [B,H,W,C]
  -> [B,H-3,W-3,Cout].  ``weight.shape[1] <= 16`` selects the thin form: x then has 4, 8 or 16 floats per pixel (``thin_channels``)
  with exact zeros above the filter's channels.
* ``norm_act_pool(x, gamma, beta, pool)``          ``F.avg_pool2d(F.leaky_relu(F.instance_norm(x, weight=gamma, bias=beta), 0.2), 2)``;
  ``gamma = beta = None``: no normalisation (block 0); ``pool=False``: no pooling (the last block).

Each backward computes only the gradients ``needs_input_grad`` asks for: a frozen discriminator in the generator's step runs no
weight gradient.  GPU only: no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch

from . import _op
from ._op import CHANNEL_GRANULE

_MODULE = "disc_ops"
THIN_MAX = 16   # up to this many real channels a map is kept thin; above, padded to a multiple of 32


def thin_channels(real: int) -> int:
    """Floats per pixel of a map with ``real`` channels in front of ``conv4_valid``: the smallest of 4, 8, 16 that holds them, or the
    next multiple of 32 from 17 channels on."""
    if real < 1:
        raise ValueError(f"thin_channels: {real} channels")
    for cp in (4, 8, 16):
        if real <= cp:
            return cp
    return _op.round_up(real, CHANNEL_GRANULE)


class _Conv4Function(torch.autograd.Function):
    """x NHWC [B,H,W,Cx], OIHW weight [Cout,Cw,4,4], bias -> NHWC [B,H-3,W-3,Cout]; thin = Cx where Cx <= 16, else 0 (Cw == Cx)."""

    @staticmethod
    def forward(ctx, x, weight, bias, thin):
        b, h, w, _ = x.shape
        cout, cw = weight.shape[:2]
        out = torch.empty(b, h - 3, w - 3, cout, dtype=torch.float32, device=x.device)
        work = _op.workspace("conv4", x.device, b, h, w, cw, cout, 0, 0, thin, family="disc")
        _op.call("conv4", x.device, x, b, h, w, cw, _op.dense(weight.detach()), None if bias is None else _op.dense(bias.detach()),
                 cout, 0, 0, thin, out, work=work, family="disc")
        ctx.save_for_backward(x, weight)
        ctx.thin, ctx.has_bias = thin, bias is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        thin = ctx.thin
        grad_out = _op.dense(grad_out)
        b, h, w, cx = x.shape
        cout, cw = weight.shape[:2]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # dX = valid 4x4 correlation of dY zero-padded by 3 with the filter transposed over (out, in) and flipped over (y, x)
            gx = torch.empty_like(x)
            work = _op.workspace("conv4", x.device, b, h - 3, w - 3, cout, cw, 3, 1, thin, family="disc")
            _op.call("conv4", x.device, grad_out, b, h - 3, w - 3, cout, _op.dense(weight.detach()), None, cw, 3, 1, thin, gx,
                     work=work, family="disc")
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            gwx = torch.empty(cout, cx, 4, 4, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[1] else None
            gb = torch.empty(cout, dtype=torch.float32, device=x.device) if want_b else None
            work = _op.workspace("conv4_wgrad", x.device, b, h, w, cx, cout, family="disc")
            _op.call("conv4_wgrad", x.device, x, grad_out, b, h, w, cx, cout, gwx, gb, work=work, family="disc")
            if ctx.needs_input_grad[1]:
                gw = gwx if cw == cx else gwx[:, :cw].contiguous()
        return gx, gw, gb, None


def conv4_valid(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """``F.conv2d`` with a 4x4 filter, no padding, stride 1, on NHWC x [B,H,W,Cx] -> [B,H-3,W-3,Cout]; weight OIHW [Cout,Cw,4,4].
    ``Cw`` and ``Cout`` multiples of 32 with ``Cx == Cw`` -- or ``Cw <= 16`` with ``Cx == thin_channels(Cw)`` and exact zeros in x's
    channels ``Cw .. Cx-1`` (the thin first layer: K = 16 Cx instead of 16 x 32).  Differentiable in x, weight and bias."""
    _op.operands(_MODULE, "conv4_valid", x, weight, bias)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4) or x.dim() != 4:
        raise ValueError(f"conv4_valid: a [Cout,Cin,4,4] filter and an NHWC input are required, got {tuple(weight.shape)} / {tuple(x.shape)}")
    cout, cw = weight.shape[:2]
    cx = x.shape[3]
    thin = cx if cw <= THIN_MAX else 0
    if cout % CHANNEL_GRANULE or (thin and cx != thin_channels(cw)) or (not thin and (cw % CHANNEL_GRANULE or cx != cw)):
        raise ValueError(f"conv4_valid: weight {tuple(weight.shape)} / input {tuple(x.shape)} unsupported (Cout a multiple of "
                         f"{CHANNEL_GRANULE}; Cin a multiple of {CHANNEL_GRANULE} with as many input channels, or Cin <= {THIN_MAX} with "
                         f"thin_channels(Cin) floats per input pixel)")
    if x.shape[1] < 4 or x.shape[2] < 4:
        raise ValueError(f"conv4_valid: a {x.shape[1]} x {x.shape[2]} map is smaller than the 4 x 4 filter")
    return _Conv4Function.apply(_op.dense(x), weight, bias, thin)


class _NormActPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, pool):
        b, h, w, c = x.shape
        norm = int(gamma is not None)
        out = torch.empty((b, h // 2, w // 2, c) if pool else (b, h, w, c), dtype=torch.float32, device=x.device)
        stats = torch.empty(b, c, 2, dtype=torch.float64, device=x.device) if norm else None
        work = _op.workspace("norm_act_pool", x.device, b, h, w, c, norm, family="disc") if norm else None
        g = _op.dense(gamma.detach()) if norm else None
        be = _op.dense(beta.detach()) if norm else None
        _op.call("norm_act_pool", x.device, x, g, be, b, h, w, c, norm, int(pool), stats, out, work, 0 if work is None else work.numel(),
                 family="disc")
        ctx.save_for_backward(x, stats, gamma, beta)
        ctx.norm, ctx.pool = norm, int(pool)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, stats, gamma, beta = ctx.saved_tensors
        norm, pool = ctx.norm, ctx.pool
        need_x, need_g, need_b = ctx.needs_input_grad[0], norm and ctx.needs_input_grad[1], norm and ctx.needs_input_grad[2]
        if not (need_x or need_g or need_b):
            return None, None, None, None
        b, h, w, c = x.shape
        grad_out = _op.dense(grad_out)
        gx = torch.empty_like(x) if need_x else None
        gg = torch.empty(c, dtype=torch.float32, device=x.device) if need_g else None
        gb = torch.empty(c, dtype=torch.float32, device=x.device) if need_b else None
        work = _op.workspace("norm_act_pool_backward", x.device, b, h, w, c, norm, family="disc") if norm else None
        g = _op.dense(gamma.detach()) if norm else None
        be = _op.dense(beta.detach()) if norm else None
        _op.call("norm_act_pool_backward", x.device, x, stats, g, be, grad_out, b, h, w, c, norm, pool, gx, gg, gb, work,
                 0 if work is None else work.numel(), family="disc")
        return gx, gg, gb, None


def norm_act_pool(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], pool: bool) -> torch.Tensor:
    """NHWC x [B,H,W,C] -> ``leaky_relu(instance_norm(x) * gamma + beta, 0.2)`` (InstanceNorm2d: eps 1e-5, biased variance, no running
    statistics; ``gamma = beta = None``: no normalisation), then with ``pool`` ``avg_pool2d(., 2)`` -> [B,H//2,W//2,C] (an odd last row
    or column feeds no window).  One apply pass over x; differentiable in x, gamma and beta (recomputed from x and the saved
    statistics).  C a multiple of 4."""
    _op.operands(_MODULE, "norm_act_pool", x, gamma, beta)
    if (gamma is None) != (beta is None):
        raise ValueError("norm_act_pool: gamma and beta come together")
    if x.dim() != 4 or x.shape[3] % 4 or (gamma is not None and (tuple(gamma.shape) != (x.shape[3],) or tuple(beta.shape) != (x.shape[3],))):
        raise ValueError(f"norm_act_pool: an NHWC input with channels a multiple of 4 and [C] parameters are required, got {tuple(x.shape)}")
    if gamma is not None and x.shape[1] * x.shape[2] < 2:
        raise ValueError("norm_act_pool: InstanceNorm needs more than one value per channel")
    if pool and (x.shape[1] < 2 or x.shape[2] < 2):
        raise ValueError(f"norm_act_pool: a {x.shape[1]} x {x.shape[2]} map has no 2 x 2 pooling window")
    return _NormActPoolFunction.apply(_op.dense(x), gamma, beta, bool(pool))
