"""The equivariance transform's entries (eamm_equi_*, csrc/equivariance.hip) against the plain-torch oracle of
tests/equivariance_common.py, float64 on the CPU, at ``closeness.close``'s bar: no element beyond
max(4 |oracle fp32 - fp64|_max, OP_FLOOR x scale).

A case is a function of ``place`` (tests/guarded.py): it calls the C entries on placed operands and compares.  Every case runs
twice on plain tensors (identical bits); the cases registered at the end of this file as ``equi-<name>`` -- every entry, shapes
whose last workgroup is partial -- run again between poisoned guard bands at skew 0 and 16 (``guarded.run_three``: tests/test_gpu_guarded_ops.py),
and must leave the bands intact and give the plain run's bits.

The smallest shapes at which the kernels can go wrong: (16,24) non-square with a partial second workgroup, (33,17) odd sizes,
(64,64) sixteen full workgroups per image; 1 / 10 / 257 points (257: a second, partial workgroup); P = 0 affine only, 2 the smallest
grid, 5 the shipped one."""
import pytest
import torch

import equivariance_common as ec
from eamm_amd import _op, tps_warp_frame, tps_warp_points
from closeness import close
from guarded import CASES, Plain, case, run_three, same_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = [(16, 24), (33, 17), (64, 64)]
SIGMAS = {"shipped": ec.SHIPPED, "wide": ec.WIDE}


def _call(name, *args):
    _op.call(name, torch.device(DEV), *args, family="equi")


def _frame(B, C, H, W, seed=1):
    return torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(seed + 7 * B + 13 * C + H + 3 * W))


def frame_case(place, frame, theta, params, P, what):
    B, C, H, W = frame.shape
    f, t = place(frame, "in", name="frame"), place(theta, "in", name="theta")
    w = place(params, "in", name="control_params") if P else None
    out = place((B, C, H, W), "out", name="out")
    _call("tps_warp_frame", f, t, w, P, B, C, H, W, out)
    want, want32 = ec.frame_reference(frame, theta, params, P)
    close(out, want, want32, what)
    return want


def points_case(place, coords, theta, params, P, what):
    """Forward with and without the jacobian, then the backward with grad_out alone, grad_jac alone and both."""
    Bc, N, _ = coords.shape
    B = theta.shape[0]
    g = torch.Generator().manual_seed(17 + N + B)
    a, b = torch.randn(B, N, 2, generator=g), torch.randn(B, N, 2, 2, generator=g)
    c, t = place(coords, "in", name="coords"), place(theta, "in", name="theta")
    w = place(params, "in", name="control_params") if P else None
    ga, gb = place(a, "in", name="grad_out"), place(b, "in", name="grad_jac")
    out, jac, alone = place((B, N, 2), "out", name="out"), place((B, N, 2, 2), "out", name="jac"), place((B, N, 2), "out", name="out alone")
    _call("tps_warp_points", c, Bc, t, w, P, B, N, out, jac)
    _call("tps_warp_points", c, Bc, t, w, P, B, N, alone, None)
    assert torch.equal(out, alone), (what, "the forward without a jacobian differs")
    ref = {}
    for dtype in (torch.float64, torch.float32):
        o, j, _ = ec.points_reference(coords, theta, params, P, dtype=dtype)
        ref[dtype] = {"out": o, "jac": j}
        for key, (ua, ub) in (("grad a", (a, None)), ("grad b", (None, b)), ("grad ab", (a, b))):
            ref[dtype][key] = ec.points_reference(coords, theta, params, P, ua, ub, dtype=dtype)[2]
    close(out, ref[torch.float64]["out"], ref[torch.float32]["out"], what + " out")
    close(jac, ref[torch.float64]["jac"], ref[torch.float32]["jac"], what + " jacobian")
    for key, (pa, pb) in (("grad a", (ga, None)), ("grad b", (None, gb)), ("grad ab", (ga, gb))):
        grad = place((Bc, N, 2), "out", name=key)
        _call("tps_warp_points_backward", c, Bc, t, w, P, B, N, pa, pb, grad)
        if P == 0 and key == "grad b":            # the affine map's jacobian is constant
            assert bool((grad == 0).all()), what
            continue
        close(grad, ref[torch.float64][key], ref[torch.float32][key], f"{what} {key}")


def twice(fn):
    """Two runs of one case on plain tensors: the same bits."""
    first, second = Plain(DEV), Plain(DEV)
    fn(first)
    fn(second)
    torch.cuda.synchronize()
    assert same_outputs(first, second) == []


# ---- the frame warp --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigmas", sorted(SIGMAS))
@pytest.mark.parametrize("P", [0, 2, 5])
@pytest.mark.parametrize("C", [1, 3, 6])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_tps_warp_frame_against_the_oracle(H, W, B, C, P, sigmas):
    theta, params = ec.draw_params(B, P, SIGMAS[sigmas], seed=H + B + C + P)
    frame = _frame(B, C, H, W)
    twice(lambda place: frame_case(place, frame, theta, params, P, f"frame {H}x{W} B{B} C{C} P{P} {sigmas}"))


def test_the_wide_sigmas_leave_the_frame():
    """What the 'wide' cases are for, stated on the oracle: a good part of the grid points fall outside [-1, 1] in x or in y."""
    theta, params = ec.draw_params(3, 5, ec.WIDE, seed=64 + 3 + 3 + 5)
    g = ec.warp(ec.coordinate_grid(64, 64).view(1, -1, 2), theta, params, 5)
    outside = float((g.abs() > 1).any(-1).float().mean())
    assert outside >= 0.25, outside


def planted_reflections(B):
    return torch.tensor([ec.THETA_MANY_REFLECTIONS]).repeat(B, 1, 1)


def planted_translations(H, W):
    """Three images.  With theta00 = (W - 1) / W the grid point j lands on pixel centre j; a shift of 2 k / W moves it k pixels.
    0: the centres themselves.  1: x half a pixel left (column 0 samples -0.5), y half a pixel down (the last row samples H - 0.5).
    2: three pixels right and five up: whole-pixel positions beyond both edges, reflected."""
    sx, sy = (W - 1) / W, (H - 1) / H
    return torch.tensor([[[sx, 0, 0], [0, sy, 0]], [[sx, 0, -1 / W], [0, sy, 1 / H]], [[sx, 0, 6 / W], [0, sy, -10 / H]]], dtype=torch.float32)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("P", [0, 5])
def test_tps_warp_frame_with_many_reflections(H, W, P):
    theta = planted_reflections(2)
    _, params = ec.draw_params(2, P, ec.SHIPPED, seed=9)
    frame = _frame(2, 3, H, W)
    flips = (ec.warp(ec.coordinate_grid(H, W).view(1, -1, 2), theta, params, P).abs() - 1) / 2      # how many times a coordinate is reflected
    assert float((flips > 0).any(-1).float().mean()) > 0.8 and float(flips.max()) > 2.2
    twice(lambda place: frame_case(place, frame, theta, params, P, f"reflections {H}x{W} P{P}"))


@pytest.mark.parametrize("H,W", SIZES)
def test_tps_warp_frame_on_edges_and_pixel_centres(H, W):
    theta = planted_translations(H, W)
    frame = _frame(3, 3, H, W)
    want = []
    twice(lambda place: want.append(frame_case(place, frame, theta, None, 0, f"edges {H}x{W}")))
    # on pixel centres the warp is the identity (up to the rounding of the positions)
    assert float((want[0][0] - frame[0].double()).abs().max()) <= 1e-4


# ---- the coordinate warp, its jacobian and its backward --------------------------------------------------------------------------
def _coords(P, N, B, Bc):
    c = ec.planted_coords(P, N, seed=3 + N)
    if Bc == 1:
        return c.view(1, N, 2)
    return torch.stack([c if b == 0 else ec.planted_coords(P, N, seed=40 + b + N) for b in range(B)])


@pytest.mark.parametrize("sigmas", sorted(SIGMAS))
@pytest.mark.parametrize("P", [0, 2, 5])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("N", [1, 10, 257])
def test_tps_warp_points_forward_jacobian_and_backward(N, B, shared, P, sigmas):
    theta, params = ec.draw_params(B, P, SIGMAS[sigmas], seed=N + B + P)
    coords = _coords(P, N, B, 1 if shared else B)
    if N >= 10:
        assert float(coords.abs().max()) > 1.0                      # points outside [-1, 1]
        if P:
            cp = ec.coordinate_grid(P, P).view(-1, 2)
            e = coords.view(-1, 1, 2) - cp.view(1, -1, 2)
            assert bool(((e[..., 0] == 0) & (e[..., 1] == 0)).any()) and bool(((e[..., 0] == 0) ^ (e[..., 1] == 0)).any())
    twice(lambda place: points_case(place, coords, theta, params, P, f"points N{N} B{B} Bc{coords.shape[0]} P{P} {sigmas}"))


@pytest.mark.parametrize("shared", [False, True])
def test_the_autograd_function_asks_for_what_is_needed(shared):
    """``tps_warp_points`` as a node: a None gradient for an unused output, no backward without a coordinate that requires one,
    and the gradient of both outputs equal to the entry's."""
    B, N, P = 4, 10, 5
    theta, params = ec.draw_params(B, P, ec.WIDE, seed=1)
    coords = _coords(P, N, B, 1 if shared else B)
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(B, N, 2, generator=g), torch.randn(B, N, 2, 2, generator=g)
    th, w = theta.to(DEV), params.to(DEV)
    out, jac = tps_warp_points(coords.to(DEV), th, w, P, True)
    assert not out.requires_grad and not jac.requires_grad
    assert tps_warp_points(coords.to(DEV), th, w, P)[1] is None
    for ua, ub in ((a, None), (None, b), (a, b)):
        x = coords.to(DEV).requires_grad_()
        out, jac = tps_warp_points(x, th, w, P, True)
        loss = 0
        if ua is not None:
            loss = loss + (out * ua.to(DEV)).sum()
        if ub is not None:
            loss = loss + (jac * ub.to(DEV)).sum()
        loss.backward()
        want = ec.points_reference(coords, theta, params, P, ua, ub)[2]
        want32 = ec.points_reference(coords, theta, params, P, ua, ub, dtype=torch.float32)[2]
        close(x.grad, want, want32, f"autograd shared={shared} a={ua is not None} b={ub is not None}")
    assert x.requires_grad and not coords.requires_grad


def test_tps_warp_frame_through_the_python_operator():
    theta, params = ec.draw_params(3, 5, ec.WIDE, seed=8)
    frame = _frame(3, 3, 33, 17)
    got = tps_warp_frame(frame.to(DEV), theta.to(DEV), params.to(DEV).view(3, 1, 25), 5)
    want, want32 = ec.frame_reference(frame, theta, params, 5)
    close(got, want, want32, "tps_warp_frame")
    with pytest.raises(ValueError, match="tps_warp_frame: the frame requires a gradient"):
        tps_warp_frame(frame.to(DEV).requires_grad_(), theta.to(DEV), params.to(DEV), 5)


# ---- between guard bands ---------------------------------------------------------------------------------------------------------
def _frame_guarded(H, W, B, C, P, sigmas, seed):
    theta, params = ec.draw_params(B, P, sigmas, seed=seed)
    frame = _frame(B, C, H, W)
    return lambda place: frame_case(place, frame, theta, params, P, f"guarded frame {H}x{W} B{B} C{C} P{P}")


def _points_guarded(N, B, Bc, P):
    theta, params = ec.draw_params(B, P, ec.WIDE, seed=N + B)
    coords = _coords(P, N, B, Bc)
    return lambda place: points_case(place, coords, theta, params, P, f"guarded points N{N} B{B} Bc{Bc} P{P}")


_FRAME, _POINTS = ["eamm_equi_tps_warp_frame"], ["eamm_equi_tps_warp_points", "eamm_equi_tps_warp_points_backward"]
case("equi-frame-16x24", _FRAME, _frame_guarded(16, 24, 3, 3, 5, ec.WIDE, 1))        # 384 pixels: the second workgroup is half full
case("equi-frame-33x17-c6", _FRAME, _frame_guarded(33, 17, 1, 6, 2, ec.WIDE, 2))     # 561 pixels: three workgroups
case("equi-frame-33x17-affine", _FRAME, _frame_guarded(33, 17, 3, 1, 0, ec.WIDE, 3))
case("equi-frame-reflections", _FRAME,
     lambda place: frame_case(place, _frame(2, 3, 33, 17), planted_reflections(2), ec.draw_params(2, 5, seed=9)[1], 5, "guarded reflections"))
case("equi-frame-edges", _FRAME,
     lambda place: frame_case(place, _frame(3, 3, 16, 24), planted_translations(16, 24), None, 0, "guarded edges"))
case("equi-points-257", _POINTS, _points_guarded(257, 4, 4, 5))      # 1028: five workgroups, the last of 4
case("equi-points-257-shared", _POINTS, _points_guarded(257, 4, 1, 5))
case("equi-points-10-affine", _POINTS, _points_guarded(10, 1, 1, 0))
case("equi-points-1", _POINTS, _points_guarded(1, 4, 4, 2))


# the ids these nine runs have always had, kept beside tests/test_gpu_guarded_ops.py's test_guarded[equi-*], which makes the same call
@pytest.mark.parametrize("cid", sorted(c[len("equi-"):] for c in CASES if c.startswith("equi-")))
def test_case_between_guard_bands(cid):
    run_three("equi-" + cid, DEV)
