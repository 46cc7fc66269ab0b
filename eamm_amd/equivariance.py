"""The equivariance constraint of the reference's ``GeneratorFullModel`` (modules/model.py:71-152 ``Transform``, :526-552 the two loss
terms): a random affine + thin-plate transform of the driving frames, the key points detected on the transformed frames warped back,
and the L1 distances that tie both detections together.  The transform's kernels are ``eamm_amd.equivariance_ops``; the 2x2 products
of the jacobian term are element-wise torch on [B,K,2,2]; both means are the deterministic ``perceptual_ops.l1_pair``.
GPU only: no CPU fallback (a ``Transform`` can be BUILT anywhere -- its noise is drawn on the CPU, as the reference's)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import equivariance_ops as ops
from .perceptual_ops import l1_pair


def _coordinate_grid(h: int, w: int) -> torch.Tensor:
    """make_coordinate_grid (reference modules/util.py): [h,w,2] of (x, y) in [-1, 1], fp32."""
    x = 2 * (torch.arange(w, dtype=torch.float32) / (w - 1)) - 1
    y = 2 * (torch.arange(h, dtype=torch.float32) / (h - 1)) - 1
    return torch.stack([x.view(1, -1).repeat(h, 1), y.view(-1, 1).repeat(1, w)], dim=2)


def _inverse_theta(theta: torch.Tensor) -> torch.Tensor:
    """The first two rows of inv([theta; 0 0 1]) in closed form (computed in float64, rounded once): [B,2,3]."""
    t = theta.double()
    a, b, tx, c, d, ty = t[:, 0, 0], t[:, 0, 1], t[:, 0, 2], t[:, 1, 0], t[:, 1, 1], t[:, 1, 2]
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    rows = [ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty)]
    return torch.stack(rows, dim=1).view(-1, 2, 3).to(theta.dtype)


class Transform:
    """The reference's ``Transform``: ``theta`` [bs,2,3] = identity + N(0, sigma_affine^2) and, with ``sigma_tps`` and ``points_tps``
    both given, ``control_params`` [bs,1,P^2] ~ N(0, sigma_tps^2) on the ``control_points`` [1,P^2,2] of the P x P coordinate grid.
    The noise is drawn on the CPU by the reference's two ``torch.normal`` calls in the reference's order (the same draws under the
    same ``torch.manual_seed``; ``generator``: a CPU generator to draw from instead), then moved to ``device``."""

    def __init__(self, bs: int, sigma_affine: float, sigma_tps: Optional[float] = None, points_tps: Optional[int] = None, *,
                 device=None, generator: Optional[torch.Generator] = None):
        if (sigma_tps is None) != (points_tps is None):
            raise ValueError("Transform: sigma_tps and points_tps go together, got only one of them")
        if points_tps is not None and (int(points_tps) != points_tps or not 2 <= points_tps <= ops.MAX_POINTS):
            raise ValueError(f"Transform: points_tps must be an integer 2..{ops.MAX_POINTS}, got {points_tps}")
        if int(bs) != bs or bs < 1:
            raise ValueError(f"Transform: bs must be a positive integer, got {bs}")
        noise = torch.normal(mean=0, std=sigma_affine * torch.ones([bs, 2, 3]), generator=generator)
        theta = noise + torch.eye(2, 3).view(1, 2, 3)
        params = None
        if points_tps is not None:
            params = torch.normal(mean=0, std=sigma_tps * torch.ones([bs, 1, points_tps ** 2]), generator=generator)
        self._set(theta, params, points_tps, device)

    def _set(self, theta, params, points, device):
        dev = None if device is None else torch.device(device)
        self.bs = int(theta.shape[0])
        self.theta = theta if dev is None else theta.to(dev)
        self.tps = params is not None
        self.points = int(points) if self.tps else 0
        if self.tps:
            self.control_points = _coordinate_grid(self.points, self.points).view(1, self.points ** 2, 2)
            self.control_params = params if dev is None else params.to(dev)
            if dev is not None:
                self.control_points = self.control_points.to(dev)
        self._cache = {}

    @classmethod
    def from_params(cls, theta: torch.Tensor, control_params: Optional[torch.Tensor] = None, points_tps: Optional[int] = None) -> "Transform":
        """A transform with GIVEN parameters: ``theta`` [bs,2,3]; ``control_params`` of bs * P^2 weights (``points_tps``: P, taken from
        the weights' count where omitted), or None for the affine part alone.  It lives where ``theta`` lies."""
        if theta.dim() != 3 or tuple(theta.shape[1:]) != (2, 3) or theta.shape[0] < 1:
            raise ValueError(f"Transform.from_params: theta must be [bs,2,3], got {tuple(theta.shape)}")
        bs = theta.shape[0]
        if control_params is None:
            if points_tps is not None:
                raise ValueError("Transform.from_params: points_tps without control_params")
        else:
            if points_tps is None:
                points_tps = math.isqrt(control_params.numel() // bs)
            if int(points_tps) != points_tps or not 2 <= points_tps <= ops.MAX_POINTS:
                raise ValueError(f"Transform.from_params: points_tps must be an integer 2..{ops.MAX_POINTS}, got {points_tps}")
            if control_params.numel() != bs * points_tps ** 2:
                raise ValueError(f"Transform.from_params: control_params must hold {bs} x {points_tps ** 2} weights, got "
                                 f"{tuple(control_params.shape)}")
            control_params = control_params.detach().to(torch.float32).reshape(bs, 1, points_tps ** 2)
        self = cls.__new__(cls)
        self._set(theta.detach().to(torch.float32), control_params, points_tps, None)
        return self

    def _on(self, device: torch.device, inverse: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(theta or its inverse, control_params) on ``device``, moved once."""
        key = (device, inverse)
        if key not in self._cache:
            theta = _inverse_theta(self.theta) if inverse else self.theta
            self._cache[key] = (theta.to(device), self.control_params.to(device) if self.tps else None)
        return self._cache[key]

    def _frame(self, frame, inverse, what):
        ops._op.need_gpu(frame, "equivariance", f"Transform.{what}")
        if frame.dim() != 4 or frame.shape[0] != self.bs:
            raise ValueError(f"Transform.{what}: the frame batch {tuple(frame.shape)} is not [bs = {self.bs},C,H,W]")
        if frame.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"Transform.{what}: the frame requires a gradient, and the frame warp has none (frames are data)")
        theta, params = self._on(frame.device, inverse)
        return ops.tps_warp_frame(frame, theta, params, self.points)

    def _points(self, coordinates, inverse, jacobian, what):
        ops._op.need_gpu(coordinates, "equivariance", f"Transform.{what}")
        if coordinates.dim() != 3 or coordinates.shape[2] != 2 or coordinates.shape[0] not in (1, self.bs):
            raise ValueError(f"Transform.{what}: the coordinate batch {tuple(coordinates.shape)} is neither [1,N,2] nor [bs = {self.bs},N,2]")
        theta, params = self._on(coordinates.device, inverse)
        return ops.tps_warp_points(coordinates, theta, params, self.points, jacobian)

    def transform_frame(self, frame: torch.Tensor) -> torch.Tensor:
        """``F.grid_sample(frame, warp_coordinates(grid), padding_mode='reflection')`` for frame [bs,C,H,W]."""
        return self._frame(frame, False, "transform_frame")

    def inverse_transform_frame(self, frame: torch.Tensor) -> torch.Tensor:
        """The same with ``inverse_warp_coordinates``."""
        return self._frame(frame, True, "inverse_transform_frame")

    def warp_coordinates(self, coordinates: torch.Tensor) -> torch.Tensor:
        """[1 or bs,N,2] -> [bs,N,2]; differentiable in the coordinates."""
        return self._points(coordinates, False, False, "warp_coordinates")[0]

    def inverse_warp_coordinates(self, coordinates: torch.Tensor) -> torch.Tensor:
        """The reference's: the affine part inverted, the thin-plate term added as it is."""
        return self._points(coordinates, True, False, "inverse_warp_coordinates")[0]

    def jacobian(self, coordinates: torch.Tensor) -> torch.Tensor:
        """``d warp_coordinates / d coordinates`` [bs,N,2,2], itself differentiable in the coordinates.  The argument's
        ``requires_grad`` is left as it is."""
        return self._points(coordinates, False, True, "jacobian")[1]


def _matmul2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[...,2,2] x [...,2,2], element-wise: c[i][j] = a[i][0] b[0][j] + a[i][1] b[1][j]."""
    return a[..., :, 0:1] * b[..., 0:1, :] + a[..., :, 1:2] * b[..., 1:2, :]


def _inverse2(m: torch.Tensor) -> torch.Tensor:
    a, b, c, d = m[..., 0, 0], m[..., 0, 1], m[..., 1, 0], m[..., 1, 1]
    det = a * d - b * c
    return torch.stack([d / det, -b / det, -c / det, a / det], dim=-1).view(*m.shape[:-2], 2, 2)


def equivariance_loss(kp_extractor, driving: torch.Tensor, kp_driving: Dict[str, torch.Tensor], transform: Transform,
                      equivariance_value: float, equivariance_jacobian: float) -> Tuple[Dict[str, torch.Tensor], Dict[str, object]]:
    """modules/model.py:526-552: ``(loss_values, extras)``.  ``kp_extractor`` detects on ``transform.transform_frame(driving)``;
    ``'equivariance_value' = w mean|kp_driving.value - warp(transformed_kp.value)|`` and ``'equivariance_jacobian' =
    w mean|I - inv(kp_driving.jacobian) jacobian(transformed_kp.value) transformed_kp.jacobian|``.  A term whose weight is 0 is absent;
    with both 0 nothing runs and both dicts are empty.  ``extras``: ``transformed_frame`` and ``transformed_kp``."""
    if equivariance_value == 0 and equivariance_jacobian == 0:
        return {}, {}
    if equivariance_jacobian != 0 and "jacobian" not in kp_driving:
        raise ValueError("equivariance_loss: equivariance_jacobian is set, but kp_driving has no 'jacobian' (a detector without jacobians)")
    transformed_frame = transform.transform_frame(driving)
    transformed_kp = kp_extractor(transformed_frame)
    extras = {"transformed_frame": transformed_frame, "transformed_kp": transformed_kp}
    values = {}
    if equivariance_value != 0:
        values["equivariance_value"] = l1_pair(kp_driving["value"], transform.warp_coordinates(transformed_kp["value"]),
                                               float(equivariance_value))
    if equivariance_jacobian != 0:
        if "jacobian" not in transformed_kp:
            raise ValueError("equivariance_loss: equivariance_jacobian is set, but the detector returned no 'jacobian'")
        product = _matmul2(_inverse2(kp_driving["jacobian"]), _matmul2(transform.jacobian(transformed_kp["value"]), transformed_kp["jacobian"]))
        eye = torch.eye(2, dtype=product.dtype, device=product.device).view(1, 1, 2, 2).expand_as(product)
        values["equivariance_jacobian"] = l1_pair(eye, product, float(equivariance_jacobian))
    return values, extras
