"""What the equivariance tests share: a plain-torch oracle of the transform (reference modules/model.py:71-152) and of
``F.grid_sample(mode='bilinear', padding_mode='reflection', align_corners=False)``, written from the formulas and differentiated by
autograd -- twice for the jacobian's gradient, as the reference does -- on the CPU, in any dtype; the seeded parameters and planted
cases; the fixture's loader.  The tests run it in float64 and in float32 from identical fp32-rounded inputs (the coordinate grids
included: they are fp32 values in both runs, as the kernels build them) and compare with ``closeness.close``:
no element beyond max(4 |fp32 - fp64|_max, OP_FLOOR x scale)."""
import os

import numpy as np
import torch

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "equivariance_tiny.npz")
EPS = 1e-6
SHIPPED = (0.05, 0.005)      # sigma_affine, sigma_tps of every shipped configuration (points_tps 5)
WIDE = (0.3, 0.02)           # a third of the grid points leave the frame
# every pixel takes several reflections, and the y axis is mirrored
THETA_MANY_REFLECTIONS = [[3.2, 0.0, 2.7], [0.0, -3.2, -2.7]]


def coordinate_grid(h, w, dtype=torch.float32, grid_dtype=torch.float32):
    """make_coordinate_grid: [h,w,2] of (x, y); computed in ``grid_dtype``, handed on in ``dtype``."""
    x = 2 * (torch.arange(w, dtype=grid_dtype) / (w - 1)) - 1
    y = 2 * (torch.arange(h, dtype=grid_dtype) / (h - 1)) - 1
    return torch.stack([x.view(1, -1).repeat(h, 1), y.view(-1, 1).repeat(1, w)], dim=2).to(dtype)


def draw_params(bs, points, sigmas=SHIPPED, seed=0):
    """(theta [bs,2,3], control_params [bs,P^2] or None), fp32: the constructor's recipe from a generator of its own."""
    g = torch.Generator().manual_seed(seed)
    theta = torch.normal(mean=0, std=sigmas[0] * torch.ones(bs, 2, 3), generator=g) + torch.eye(2, 3).view(1, 2, 3)
    params = torch.normal(mean=0, std=sigmas[1] * torch.ones(bs, points * points), generator=g) if points else None
    return theta, params


def inverse_theta(theta):
    """The first two rows of inv([theta; 0 0 1]), in theta's dtype (torch.linalg on the CPU)."""
    bottom = torch.tensor([0, 0, 1], dtype=theta.dtype).view(1, 1, 3).expand(theta.shape[0], 1, 3)
    return torch.linalg.inv(torch.cat([theta, bottom], dim=1))[:, :2]


def warp(coords, theta, params, points, grid_dtype=torch.float32):
    """warp_coordinates: coords [Bc,N,2] (Bc 1 or B) -> [B,N,2] in coords' dtype."""
    dt = coords.dtype
    theta = theta.to(dt).unsqueeze(1)
    out = (torch.matmul(theta[:, :, :, :2], coords.unsqueeze(-1)) + theta[:, :, :, 2:]).squeeze(-1)
    if points:
        cp = coordinate_grid(points, points, dt, grid_dtype).view(1, 1, -1, 2)
        d = (coords.view(coords.shape[0], -1, 1, 2) - cp).abs().sum(-1)
        r = (d ** 2 * torch.log(d + EPS) * params.to(dt).view(theta.shape[0], 1, -1)).sum(dim=2)
        out = out + r.unsqueeze(-1)
    return out


def warp_with_jacobian(coords, theta, params, points):
    """(coords as the leaf to differentiate in, out [B,N,2], jacobian [B,N,2,2]) with the jacobian by autograd, ``create_graph=True``."""
    leaf = coords.detach().clone().requires_grad_()
    each = leaf.expand(theta.shape[0], -1, -1)          # one row per image: the jacobian of image b alone
    out = warp(each, theta, params, points)
    gx, = torch.autograd.grad(out[..., 0].sum(), each, create_graph=True)
    gy, = torch.autograd.grad(out[..., 1].sum(), each, create_graph=True)
    return leaf, out, torch.stack([gx, gy], dim=-2)


def points_reference(coords, theta, params, points, a=None, b=None, dtype=torch.float64):
    """out, jacobian and (where ``a`` / ``b`` are given) the coordinate gradient of ``(out a).sum() + (jacobian b).sum()``."""
    leaf, out, jac = warp_with_jacobian(coords.to(dtype), theta, params, points)
    grad = None
    if a is not None or b is not None:
        loss = 0
        if a is not None:
            loss = loss + (out * a.to(dtype)).sum()
        if b is not None:
            loss = loss + (jac * b.to(dtype)).sum()
        if loss.requires_grad:
            grad, = torch.autograd.grad(loss, leaf, allow_unused=True)
        if grad is None:
            grad = torch.zeros_like(leaf)
    return out.detach(), jac.detach(), grad


def reflect_clip(i, size):
    a = (i + 0.5).abs()
    extra = torch.fmod(a, size)
    flips = torch.floor(a / size)
    r = torch.where(torch.fmod(flips, 2) == 0, extra - 0.5, size - extra - 0.5)
    return r.clamp(0, size - 1)


def grid_sample_reflection(frame, grid):
    """frame [B,C,H,W], grid [B,h,w,2] -> [B,C,h,w]."""
    B, C, H, W = frame.shape
    ix = reflect_clip(((grid[..., 0] + 1) * W - 1) / 2, W)
    iy = reflect_clip(((grid[..., 1] + 1) * H - 1) / 2, H)
    x0, y0 = ix.floor(), iy.floor()
    ax, ay = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    flat = frame.reshape(B, C, H * W)

    def tap(yy, xx, wgt):
        inside = ((xx < W) & (yy < H)).to(frame.dtype)
        idx = (yy.clamp(max=H - 1) * W + xx.clamp(max=W - 1)).view(B, 1, -1).expand(B, C, -1)
        return flat.gather(2, idx).view(B, C, *yy.shape[1:]) * (wgt * inside).unsqueeze(1)

    return tap(y0, x0, (1 - ax) * (1 - ay)) + tap(y0, x0 + 1, ax * (1 - ay)) + tap(y0 + 1, x0, (1 - ax) * ay) + tap(y0 + 1, x0 + 1, ax * ay)


def transform_frame(frame, theta, params, points, grid_dtype=torch.float32):
    """transform_frame in frame's dtype."""
    B, C, H, W = frame.shape
    grid = coordinate_grid(H, W, frame.dtype, grid_dtype).view(1, H * W, 2)
    return grid_sample_reflection(frame, warp(grid, theta, params, points, grid_dtype).view(B, H, W, 2))


def frame_reference(frame, theta, params, points):
    """(float64, float32) of the oracle from the same fp32 values."""
    return transform_frame(frame.double(), theta, params, points), transform_frame(frame.float(), theta, params, points)


def planted_coords(points, n, seed=3):
    """[n,2] coordinates, the first ones planted: on a control point, sharing x with one, sharing y with one (bit-equal fp32 values,
    so that sign(0) = 0 is met exactly), two outside [-1, 1]; the rest uniform in [-1.3, 1.3]."""
    c = torch.rand(n, 2, generator=torch.Generator().manual_seed(seed)) * 2.6 - 1.3
    if points:
        cp = coordinate_grid(points, points).view(-1, 2)
        planted = [cp[points + 1].clone(), torch.stack([cp[1, 0], torch.tensor(0.137)]), torch.stack([torch.tensor(-0.411), cp[points, 1]])]
    else:
        planted = [torch.tensor([0.0, 0.0])]
    planted += [torch.tensor([1.7, -0.2]), torch.tensor([-1.25, 2.4])]
    for i, p in enumerate(planted[:n]):
        c[i] = p
    return c


def load_fixture():
    with np.load(FIXTURE) as f:
        return {k: (torch.from_numpy(f[k]) if f[k].ndim else f[k].item()) for k in f.files}


def jacobian_of(coords, theta, params, points):
    """``Transform.jacobian`` for coordinates [B,N,2] that are part of a graph: autograd with ``create_graph=True``, as the reference."""
    out = warp(coords, theta, params, points)
    gx, = torch.autograd.grad(out[..., 0].sum(), coords, create_graph=True)
    gy, = torch.autograd.grad(out[..., 1].sum(), coords, create_graph=True)
    return torch.stack([gx, gy], dim=-2)


def loss_reference(kp_driving, transformed_kp, theta, params, points, weight_value, weight_jacobian):
    """modules/model.py:535-552 in the key points' dtype: {'equivariance_value', 'equivariance_jacobian'} (a zero weight: absent)."""
    values = {}
    if weight_value:
        values["equivariance_value"] = weight_value * (kp_driving["value"] - warp(transformed_kp["value"], theta, params, points)).abs().mean()
    if weight_jacobian:
        jt = torch.matmul(jacobian_of(transformed_kp["value"], theta, params, points), transformed_kp["jacobian"])
        value = torch.matmul(torch.inverse(kp_driving["jacobian"]), jt)
        eye = torch.eye(2, dtype=value.dtype).view(1, 1, 2, 2)
        values["equivariance_jacobian"] = weight_jacobian * (eye - value).abs().mean()
    return values


def kp_leaves(sd, dtype):
    """The detector's state dict in ``dtype`` with its trainable tensors as leaves (tests/test_gpu_kp_backward.py)."""
    leaf = lambda k, v: v.is_floating_point() and "running" not in k and k != "down.weight"
    return {k: (v.detach().clone().to(dtype).requires_grad_() if leaf(k, v) else v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
