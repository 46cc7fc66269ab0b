"""The equivariance constraint's transform as operators (reference modules/model.py:71-152, class ``Transform``) on libeamm_hip.so
kernels (csrc/equivariance.hip; C ABI ``eamm_equi_tps_warp_frame``, ``eamm_equi_tps_warp_points`` and its ``_backward``).

* ``tps_warp_frame(frame, theta, control_params, points)``  ``F.grid_sample(frame, warp(grid), padding_mode='reflection')`` in one
  pass: every output pixel warps its own grid point and samples there; no grid and no distance tensor exist.  No gradient.
* ``tps_warp_points(coords, theta, control_params, points, want_jacobian)``  the warp of given points and, where asked, its
  jacobian; a ``torch.autograd.Function`` whose backward is a kernel too and differentiates BOTH outputs in the coordinates.

``warp(c) = theta[:, :, :2] c + theta[:, :, 2] + sum_p w_p U(|c - c_p|_1)``, ``U(d) = d^2 log(d + 1e-6)``, control points on the
``points x points`` coordinate grid; ``points = 0``: the affine part alone.  ``theta`` and ``control_params`` are data: the reference
draws them and trains neither, so they get no gradient.  GPU only: no CPU fallback."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _op

_MODULE = "equivariance_ops"
_FAMILY = "equi"
MAX_POINTS = 16      # control points per side (csrc/eamm_equi_api.hip)


def _check_params(theta: torch.Tensor, control_params: Optional[torch.Tensor], points: int, what: str) -> Tuple[torch.Tensor, Optional[torch.Tensor], int]:
    """theta [B,2,3]; control_params (or None with points 0) of B * points^2 values.  Returns them detached and contiguous."""
    points = int(points or 0)
    if theta.dim() != 3 or tuple(theta.shape[1:]) != (2, 3):
        raise ValueError(f"{what}: theta must be [B,2,3], got {tuple(theta.shape)}")
    if points != 0 and not 2 <= points <= MAX_POINTS:
        raise ValueError(f"{what}: points must be 0 (affine only) or 2..{MAX_POINTS}, got {points}")
    _op.need_gpu(theta, _MODULE, what)
    if points == 0:
        return _op.dense(theta.detach()), None, 0
    if control_params is None or control_params.numel() != theta.shape[0] * points * points:
        raise ValueError(f"{what}: control_params must hold {theta.shape[0]} x {points * points} weights, got "
                         f"{None if control_params is None else tuple(control_params.shape)}")
    _op.need_gpu(control_params, _MODULE, what)
    if control_params.device != theta.device:
        raise RuntimeError(f"{what}: theta and control_params are on different devices")
    return _op.dense(theta.detach()), _op.dense(control_params.detach().reshape(theta.shape[0], points * points)), points


def tps_warp_frame(frame: torch.Tensor, theta: torch.Tensor, control_params: Optional[torch.Tensor], points: int) -> torch.Tensor:
    """``frame`` NCHW [B,C,H,W] (C 1..6, H and W at least 2) seen through the transform: the reference's ``transform_frame``, bilinear
    with reflection padding.  Not differentiable: a frame that requires a gradient is refused."""
    _op.need_gpu(frame, _MODULE, "tps_warp_frame")
    if frame.dim() != 4 or not 1 <= frame.shape[1] <= 6 or frame.shape[2] < 2 or frame.shape[3] < 2:
        raise ValueError(f"tps_warp_frame: an NCHW batch [B,1..6,H>=2,W>=2] is required, got {tuple(frame.shape)}")
    if frame.requires_grad and torch.is_grad_enabled():
        raise ValueError("tps_warp_frame: the frame requires a gradient, and the frame warp has none (frames are data)")
    theta, params, points = _check_params(theta, control_params, points, "tps_warp_frame")
    if theta.shape[0] != frame.shape[0]:
        raise ValueError(f"tps_warp_frame: the frame batch {frame.shape[0]} is not the transform's {theta.shape[0]}")
    if theta.device != frame.device:
        raise RuntimeError("tps_warp_frame: frame and theta are on different devices")
    frame = _op.dense(frame.detach())
    b, c, h, w = frame.shape
    out = torch.empty_like(frame)
    _op.call("tps_warp_frame", frame.device, frame, theta, params, points, b, c, h, w, out, family=_FAMILY)
    return out


class _TpsWarpPointsFunction(torch.autograd.Function):
    """coords [Bc,N,2] (Bc 1 or B) -> (out [B,N,2], jacobian [B,N,2,2] or None)."""

    @staticmethod
    def forward(ctx, coords, theta, params, points, want_jacobian):
        bc, n, _ = coords.shape
        b = theta.shape[0]
        out = torch.empty(b, n, 2, dtype=torch.float32, device=coords.device)
        jac = torch.empty(b, n, 2, 2, dtype=torch.float32, device=coords.device) if want_jacobian else None
        _op.call("tps_warp_points", coords.device, coords, bc, theta, params, points, b, n, out, jac, family=_FAMILY)
        ctx.save_for_backward(coords, theta, params)
        ctx.points = points
        ctx.set_materialize_grads(False)
        return out, jac

    @staticmethod
    def backward(ctx, grad_out, grad_jac):
        if not ctx.needs_input_grad[0] or (grad_out is None and grad_jac is None):
            return (None,) * 5
        coords, theta, params = ctx.saved_tensors
        bc, n, _ = coords.shape
        grad_out = None if grad_out is None else _op.dense(grad_out)
        grad_jac = None if grad_jac is None else _op.dense(grad_jac)
        grad = torch.empty_like(coords)
        _op.call("tps_warp_points_backward", coords.device, coords, bc, theta, params, ctx.points, theta.shape[0], n, grad_out, grad_jac,
                 grad, family=_FAMILY)
        return (grad,) + (None,) * 4


def tps_warp_points(coords: torch.Tensor, theta: torch.Tensor, control_params: Optional[torch.Tensor], points: int,
                    want_jacobian: bool = False):
    """``(warp(coords), jacobian or None)``: ``coords`` [Bc,N,2] with Bc = 1 (one set for every image) or B -> [B,N,2] and
    ``d warp / d coords`` [B,N,2,2].  Both are differentiable in ``coords`` (the jacobian's derivative is the thin-plate term's second
    derivative); with Bc = 1 the images' gradients are added in index order.  The same bits on every run."""
    _op.need_gpu(coords, _MODULE, "tps_warp_points")
    theta, params, points = _check_params(theta, control_params, points, "tps_warp_points")
    if coords.dim() != 3 or coords.shape[2] != 2 or coords.shape[1] < 1:
        raise ValueError(f"tps_warp_points: coordinates must be [B,N,2], got {tuple(coords.shape)}")
    if coords.shape[0] not in (1, theta.shape[0]):
        raise ValueError(f"tps_warp_points: the coordinate batch {coords.shape[0]} is neither 1 nor the transform's {theta.shape[0]}")
    if theta.device != coords.device:
        raise RuntimeError("tps_warp_points: coordinates and theta are on different devices")
    return _TpsWarpPointsFunction.apply(_op.dense(coords), theta, params, points, bool(want_jacobian))
