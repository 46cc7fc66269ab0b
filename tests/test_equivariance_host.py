"""The equivariance transform without a GPU: the constructor's draws are the reference's to the bit, attributes and shapes, every
refusal by name, the binding's table, and the oracle of tests/equivariance_common.py against the reference's recorded results and
against ATen's own grid_sample (this guards the oracle, not the kernels)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import equivariance_common as ec
from conftest import ROOT
from eamm_amd import Transform, _lib, equivariance_loss, tps_warp_frame, tps_warp_points

ENTRIES = ["eamm_equi_tps_warp_frame", "eamm_equi_tps_warp_points", "eamm_equi_tps_warp_points_backward"]


@pytest.mark.parametrize("seed", [0, 5])
@pytest.mark.parametrize("bs", [1, 4])
def test_the_draws_are_the_references_two_normal_calls_to_the_bit(seed, bs):
    torch.manual_seed(seed)
    noise = torch.normal(mean=0, std=0.05 * torch.ones([bs, 2, 3]))
    params = torch.normal(mean=0, std=0.005 * torch.ones([bs, 1, 25]))
    torch.manual_seed(seed)
    t = Transform(bs, sigma_affine=0.05, sigma_tps=0.005, points_tps=5)
    assert t.tps is True and t.bs == bs
    assert torch.equal(t.theta, noise + torch.eye(2, 3).view(1, 2, 3)) and torch.equal(t.control_params, params)
    assert tuple(t.theta.shape) == (bs, 2, 3) and tuple(t.control_params.shape) == (bs, 1, 25)
    assert tuple(t.control_points.shape) == (1, 25, 2)
    assert torch.equal(t.control_points, ec.coordinate_grid(5, 5).view(1, 25, 2))
    # without TPS: one draw, and no thin-plate attributes (as the reference)
    torch.manual_seed(seed)
    t = Transform(bs, sigma_affine=0.05)
    assert t.tps is False and torch.equal(t.theta, noise + torch.eye(2, 3).view(1, 2, 3))
    assert not hasattr(t, "control_params") and not hasattr(t, "control_points")
    # a generator of its own leaves the global stream alone
    torch.manual_seed(seed)
    t = Transform(bs, 0.05, 0.005, 5, generator=torch.Generator().manual_seed(seed + 1))
    assert not torch.equal(t.theta, noise + torch.eye(2, 3).view(1, 2, 3))
    assert torch.equal(torch.normal(mean=0, std=0.05 * torch.ones([bs, 2, 3])), noise)


def test_from_params_keeps_the_given_values():
    theta, params = ec.draw_params(3, 4, seed=2)
    t = Transform.from_params(theta, params)
    assert t.bs == 3 and t.tps and t.points == 4 and torch.equal(t.theta, theta)
    assert tuple(t.control_params.shape) == (3, 1, 16) and torch.equal(t.control_params.view(3, 16), params)
    assert torch.equal(t.control_points, ec.coordinate_grid(4, 4).view(1, 16, 2))
    t = Transform.from_params(theta)
    assert not t.tps and t.points == 0
    with pytest.raises(ValueError, match="Transform.from_params: theta must be"):
        Transform.from_params(theta[0])
    with pytest.raises(ValueError, match="Transform.from_params: control_params must hold"):
        Transform.from_params(theta, params, points_tps=5)
    with pytest.raises(ValueError, match="Transform.from_params: points_tps without control_params"):
        Transform.from_params(theta, None, points_tps=5)


def test_constructor_refusals_by_name():
    with pytest.raises(ValueError, match="Transform: sigma_tps and points_tps go together"):
        Transform(2, 0.05, sigma_tps=0.005)
    with pytest.raises(ValueError, match="Transform: sigma_tps and points_tps go together"):
        Transform(2, 0.05, points_tps=5)
    for points in (1, 0, -3, 17, 2.5):
        with pytest.raises(ValueError, match="Transform: points_tps must be an integer 2..16"):
            Transform(2, 0.05, 0.005, points)
    with pytest.raises(ValueError, match="Transform: bs must be a positive integer"):
        Transform(0, 0.05)


def test_cpu_tensors_are_refused_with_the_librarys_message():
    t = Transform(2, 0.05, 0.005, 5)
    frame, coords = torch.zeros(2, 3, 8, 8), torch.zeros(2, 4, 2)
    for call in (lambda: t.transform_frame(frame), lambda: t.inverse_transform_frame(frame), lambda: t.warp_coordinates(coords),
                 lambda: t.inverse_warp_coordinates(coords), lambda: t.jacobian(coords),
                 lambda: tps_warp_frame(frame, t.theta, t.control_params, 5), lambda: tps_warp_points(coords, t.theta, t.control_params, 5)):
        with pytest.raises(RuntimeError, match=r"runs only on a ROCm GPU \(there is no CPU fallback\)"):
            call()
    assert coords.requires_grad is False


def _gpu_like(*shape, requires_grad=False):
    """Shape checks come before anything touches a device: a tensor without storage stands for one on the GPU."""
    return torch.empty(*shape, device="meta", requires_grad=requires_grad)


def test_shape_refusals_by_name(monkeypatch):
    from eamm_amd import _op
    monkeypatch.setattr(_op, "need_gpu", lambda t, module, what: None)          # the shape checks are host code
    t = Transform(3, 0.05, 0.005, 5)
    with pytest.raises(ValueError, match=r"Transform.transform_frame: the frame batch .* is not \[bs = 3,C,H,W\]"):
        t.transform_frame(_gpu_like(2, 3, 8, 8))
    with pytest.raises(ValueError, match=r"Transform.inverse_transform_frame: the frame batch"):
        t.inverse_transform_frame(_gpu_like(4, 3, 8, 8))
    with pytest.raises(ValueError, match="Transform.transform_frame: the frame requires a gradient"):
        t.transform_frame(_gpu_like(3, 3, 8, 8, requires_grad=True))
    for method in ("warp_coordinates", "inverse_warp_coordinates", "jacobian"):
        with pytest.raises(ValueError, match=rf"Transform.{method}: the coordinate batch .* is neither \[1,N,2\] nor \[bs = 3,N,2\]"):
            getattr(t, method)(_gpu_like(2, 10, 2))
        with pytest.raises(ValueError, match=rf"Transform.{method}: the coordinate batch"):
            getattr(t, method)(_gpu_like(3, 10, 3))
    theta, params = _gpu_like(3, 2, 3), _gpu_like(3, 25)
    with pytest.raises(ValueError, match="tps_warp_frame: an NCHW batch"):
        tps_warp_frame(_gpu_like(3, 7, 8, 8), theta, params, 5)
    with pytest.raises(ValueError, match="tps_warp_frame: an NCHW batch"):
        tps_warp_frame(_gpu_like(3, 3, 1, 8), theta, params, 5)
    with pytest.raises(ValueError, match="tps_warp_frame: points must be 0"):
        tps_warp_frame(_gpu_like(3, 3, 8, 8), theta, params, 1)
    with pytest.raises(ValueError, match="tps_warp_frame: control_params must hold 3 x 16 weights"):
        tps_warp_frame(_gpu_like(3, 3, 8, 8), theta, params, 4)
    with pytest.raises(ValueError, match="tps_warp_frame: the frame batch 2 is not the transform's 3"):
        tps_warp_frame(_gpu_like(2, 3, 8, 8), theta, params, 5)
    with pytest.raises(ValueError, match="tps_warp_points: the coordinate batch 2 is neither 1 nor the transform's 3"):
        tps_warp_points(_gpu_like(2, 10, 2), theta, params, 5)
    with pytest.raises(ValueError, match="tps_warp_points: theta must be"):
        tps_warp_points(_gpu_like(3, 10, 2), _gpu_like(3, 3, 3), params, 5)


def test_loss_refusals_and_the_empty_case():
    def never(_):
        raise AssertionError("with both weights 0 nothing runs")

    assert equivariance_loss(never, None, {}, None, 0, 0) == ({}, {})
    with pytest.raises(ValueError, match="equivariance_loss: equivariance_jacobian is set, but kp_driving has no 'jacobian'"):
        equivariance_loss(never, None, {"value": torch.zeros(1, 2, 2)}, None, 10, 10)


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_the_entries_are_bound_as_the_header_declares_them():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == m.group(1).count(",") + 1, name
        assert args[0] is ctypes.c_int and args[-1] is ctypes.c_void_p            # device first, stream last
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("eamm_equi_")) == sorted(ENTRIES)
    assert _lib.ABI_VERSION == 6


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def test_the_oracle_reproduces_the_references_recorded_results():
    fx = ec.load_fixture()
    theta, params, P = fx["theta"], fx["control_params"].view(2, -1), fx["points_tps"]
    torch.manual_seed(fx["transform_seed"])
    t = Transform(2, fx["sigma_affine"], fx["sigma_tps"], P)
    assert torch.equal(t.theta, theta) and torch.equal(t.control_params, fx["control_params"])
    assert fx["frame"].dtype == torch.float32 and fx["frame_out"].dtype == torch.float64
    out, jac, grad = ec.points_reference(fx["coords"], theta, params, P, fx["a"], fx["b"])
    for got, key in ((out, "coords_out"), (jac, "jacobian"), (grad, "coords_grad")):
        assert float((got - fx[key]).abs().max()) <= 1e-12 * float(fx[key].abs().max()), key
    # the reference builds the frame's grid in the frame's dtype: float64 there, fp32 values in the tests' runs
    frame = ec.transform_frame(fx["frame"].double(), theta, params, P, grid_dtype=torch.float64)
    assert float((frame - fx["frame_out"]).abs().max()) <= 1e-12
    near = ec.transform_frame(fx["frame"].double(), theta, params, P)
    assert float((near - fx["frame_out"]).abs().max()) <= 1e-5


@pytest.mark.parametrize("theta", [ec.THETA_MANY_REFLECTIONS, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [[0.9, 0.3, 0.8], [-0.2, 1.1, -1.4]]])
def test_the_oracles_sampling_is_atens_grid_sample(theta):
    frame = torch.rand(1, 2, 9, 14, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    theta = torch.tensor([theta])
    grid = ec.warp(ec.coordinate_grid(9, 14, torch.float64).view(1, -1, 2), theta, None, 0).view(1, 9, 14, 2)
    want = F.grid_sample(frame, grid, mode="bilinear", padding_mode="reflection", align_corners=False)
    assert float((ec.grid_sample_reflection(frame, grid) - want).abs().max()) <= 1e-12


def test_the_closed_forms_are_the_double_autograd():
    """U', U'' as the kernels use them (include/eamm_hip.h) against the oracle's autograd, float64."""
    P = 5
    theta, params = ec.draw_params(2, P, ec.WIDE, seed=4)
    coords = ec.planted_coords(P, 12).view(1, 12, 2).expand(2, -1, -1).contiguous()
    g = torch.Generator().manual_seed(6)
    a, b = torch.randn(2, 12, 2, generator=g), torch.randn(2, 12, 2, 2, generator=g)
    out, jac, grad = ec.points_reference(coords, theta, params, P, a, b)
    c, w, th = coords.double(), params.double(), theta.double()
    e = c.view(2, 12, 1, 2) - ec.coordinate_grid(P, P, torch.float64).view(1, 1, -1, 2)
    d, s = e.abs().sum(-1), torch.sign(e)
    l, de = torch.log(d + ec.EPS), d + ec.EPS
    u1 = 2 * d * l + d * d / de
    u2 = 2 * l + 2 * d / de + (d * d + 2 * d * ec.EPS) / (de * de)
    gvec = (w.view(2, 1, -1, 1) * u1.unsqueeze(-1) * s).sum(2)
    jac_closed = th[:, None, :, :2] + gvec.unsqueeze(-2)
    hs = (w.view(2, 1, -1, 1, 1) * u2[..., None, None] * s.unsqueeze(-1) * s.unsqueeze(-2)).sum(2)
    grad_closed = torch.einsum("bni,bnik->bnk", a.double(), jac_closed) + torch.einsum("bnij,bnjk->bnk", b.double(), hs)
    assert float((jac_closed - jac).abs().max()) <= 1e-13 and float((grad_closed - grad).abs().max()) <= 1e-12
