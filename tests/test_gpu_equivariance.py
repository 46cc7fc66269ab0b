"""``eamm_amd.equivariance``: ``Transform`` against the reference's own recorded results (tests/golden/equivariance_tiny.npz,
tools/record_equivariance_fixture.py), its inverse forms against the float64 oracle (the reference's cannot run without a GPU and
are not recorded), and ``equivariance_loss`` through the tiny KPDetector against the float64 composition of the oracle detector
(oracle/eamm_oracle.py) and tests/equivariance_common.py -- the loss values at ``closeness.close``'s bar, the detector's
parameter gradients at tests/test_gpu_kp_backward.py's rule and floors."""
import pytest
import torch

import equivariance_common as ec
from eamm_amd import KPDetector, KPDetector_a, Transform, equivariance_loss, tiny_kp_config
from eamm_amd.weights import kp_state_dict_spec, synthetic_source, synthetic_state_dict
from closeness import GRAD_FLOOR, OP_FLOOR, close, kp_close
from oracle import eamm_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KP_SEED, KP_IMAGE_SEED = 77, 3          # tests/test_gpu_kp_backward.py's


@pytest.fixture(scope="module")
def fx():
    return ec.load_fixture()


def _transform(fx, tps=True):
    return Transform.from_params(fx["theta"].to(DEV), fx["control_params"].to(DEV) if tps else None)


def test_transform_reproduces_the_references_recorded_results(fx):
    t = _transform(fx)
    assert t.bs == 2 and t.points == fx["points_tps"] and t.theta.device.type == "cuda"
    close(t.transform_frame(fx["frame"].to(DEV)), fx["frame_out"], fx["frame_out_fp32"], "transform_frame")
    c = fx["coords"].to(DEV).requires_grad_()
    out, jac = t.warp_coordinates(c), t.jacobian(c)
    close(out, fx["coords_out"], fx["coords_out_fp32"], "warp_coordinates")
    close(jac, fx["jacobian"], fx["jacobian_fp32"], "jacobian")
    ((out * fx["a"].to(DEV)).sum() + (jac * fx["b"].to(DEV)).sum()).backward()
    close(c.grad, fx["coords_grad"], fx["coords_grad_fp32"], "coordinate gradient")
    # jacobian() leaves its argument's requires_grad alone, and needs none
    plain = fx["coords"].to(DEV)
    again = t.jacobian(plain)
    assert not plain.requires_grad and not again.requires_grad and torch.equal(again, jac.detach())


@pytest.mark.parametrize("tps", [True, False])
def test_the_inverse_forms_against_the_float64_oracle(fx, tps):
    t = _transform(fx, tps)
    theta, params, P = fx["theta"], (fx["control_params"].view(2, -1) if tps else None), (fx["points_tps"] if tps else 0)
    inv64, inv32 = ec.inverse_theta(theta.double()), ec.inverse_theta(theta)
    close(t.inverse_warp_coordinates(fx["coords"].to(DEV)), ec.warp(fx["coords"].double(), inv64, params, P), ec.warp(fx["coords"], inv32, params, P),
          "inverse_warp_coordinates")
    close(t.inverse_transform_frame(fx["frame"].to(DEV)), ec.transform_frame(fx["frame"].double(), inv64, params, P),
          ec.transform_frame(fx["frame"], inv32, params, P), "inverse_transform_frame")
    if not tps:
        c = fx["coords"]
        close(t.warp_coordinates(t.inverse_warp_coordinates(c.to(DEV))), c.double(), ec.warp(ec.warp(c, inv32, None, 0), theta, None, 0),
              "warp(inverse_warp(c))")
    one = fx["coords"][:1].to(DEV)                                             # the broadcast form: [1,N,2] -> [bs,N,2]
    assert tuple(t.warp_coordinates(one).shape) == (2, 10, 2)
    assert torch.equal(t.warp_coordinates(one)[0], t.warp_coordinates(fx["coords"].to(DEV))[0])


def test_the_constructor_places_its_draws_on_the_device():
    torch.manual_seed(4)
    host = Transform(3, 0.05, 0.005, 5)
    torch.manual_seed(4)
    t = Transform(3, 0.05, 0.005, 5, device=DEV)
    assert t.theta.device.type == t.control_params.device.type == t.control_points.device.type == "cuda"
    assert torch.equal(t.theta.cpu(), host.theta) and torch.equal(t.control_params.cpu(), host.control_params)
    frame = synthetic_source(64, seed=1, batch=3).to(DEV)
    assert torch.equal(t.transform_frame(frame), host.transform_frame(frame))        # a host-built transform follows its argument


# ---- the loss ---------------------------------------------------------------------------------------------------------------------
def _detector(cfg, cls=KPDetector, seed=KP_SEED):
    sd = synthetic_state_dict(cfg, seed=seed, spec=kp_state_dict_spec(cfg))
    det = cls(**cfg)
    det.load_state_dict(sd)
    return det.to(DEV), sd


def _oracle_loss(cfg, sd, driving, theta, params, P, wv, wj, dtype):
    sdd = ec.kp_leaves(sd, dtype)
    x = driving.to(dtype)
    kp_d = orc.kp_detector_forward(sdd, cfg, x)
    kp_t = orc.kp_detector_forward(sdd, cfg, ec.transform_frame(x, theta, params, P))
    values = ec.loss_reference(kp_d, kp_t, theta, params, P, wv, wj)
    sum(values.values()).backward()
    return {k: v.detach() for k, v in values.items()}, {k: v.grad for k, v in sdd.items() if v.requires_grad}


@pytest.fixture(scope="module")
def loss_case():
    """The tiny detector, three 64 x 64 frames, a transform at the wide sigmas; the oracle's float64 and fp32 runs, computed once."""
    cfg = tiny_kp_config()
    det, sd = _detector(cfg)
    det.requires_grad_(True).eval()
    driving = synthetic_source(64, seed=KP_IMAGE_SEED, batch=3)
    theta, params = ec.draw_params(3, 5, ec.WIDE, seed=12)
    ref = {dt: _oracle_loss(cfg, sd, driving, theta, params, 5, 10.0, 10.0, dt) for dt in (torch.float64, torch.float32)}
    return dict(cfg=cfg, det=det, driving=driving, theta=theta, params=params, ref=ref)


def test_equivariance_loss_values_and_detector_gradients(loss_case):
    det, driving = loss_case["det"], loss_case["driving"].to(DEV)
    t = Transform.from_params(loss_case["theta"], loss_case["params"])                 # host-held parameters follow the frames' device
    det.zero_grad(set_to_none=True)
    values, extras = equivariance_loss(det, driving, det(driving), t, 10.0, 10.0)
    assert sorted(values) == ["equivariance_jacobian", "equivariance_value"] and sorted(extras) == ["transformed_frame", "transformed_kp"]
    assert torch.equal(extras["transformed_frame"], t.transform_frame(driving)) and "value" in extras["transformed_kp"]
    (v64, g64), (v32, g32) = loss_case["ref"][torch.float64], loss_case["ref"][torch.float32]
    for k in values:
        close(values[k], v64[k], v32[k], k)
    sum(values.values()).backward()
    gmax = max(float(v.abs().max()) for v in g64.values())
    for name, p in det.named_parameters():
        assert p.grad is not None, name
        head = name.startswith(("kp.", "jacobian."))
        kp_close(p.grad, g64[name], g32[name], "loss " + name, OP_FLOOR if head else GRAD_FLOOR, relu=not head, gmax=gmax)


def test_both_sides_receive_their_gradient_and_a_zero_weight_leaves_its_key_out(loss_case):
    det, driving = loss_case["det"], loss_case["driving"].to(DEV)
    t = Transform.from_params(loss_case["theta"].to(DEV), loss_case["params"].to(DEV))
    with torch.no_grad():
        kp = det(driving)
    kp_driving = {k: kp[k].clone().requires_grad_() for k in ("value", "jacobian")}     # leaves: the driving side alone
    for wv, wj, keys in ((10.0, 0, ["equivariance_value"]), (0, 10.0, ["equivariance_jacobian"])):
        det.zero_grad(set_to_none=True)
        for v in kp_driving.values():
            v.grad = None
        values, extras = equivariance_loss(det, driving, kp_driving, t, wv, wj)
        assert sorted(values) == keys and sorted(extras) == ["transformed_frame", "transformed_kp"]
        sum(values.values()).backward()
        side = kp_driving["value" if wv else "jacobian"].grad
        assert side is not None and bool(torch.isfinite(side).all()) and float(side.abs().max()) > 0
        assert kp_driving["jacobian" if wv else "value"].grad is None
        assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in det.parameters())
    assert equivariance_loss(det, driving, kp_driving, t, 0, 0) == ({}, {})


def test_a_detector_without_jacobians_is_refused_by_name(loss_case):
    cfg = dict(tiny_kp_config(), estimate_jacobian=False)
    det, _ = _detector(cfg)
    det.requires_grad_(True).eval()
    driving = loss_case["driving"].to(DEV)
    t = Transform.from_params(loss_case["theta"], loss_case["params"])
    with pytest.raises(ValueError, match="equivariance_loss: equivariance_jacobian is set, but kp_driving has no 'jacobian'"):
        equivariance_loss(det, driving, det(driving), t, 10.0, 10.0)
    with pytest.raises(ValueError, match="equivariance_loss: equivariance_jacobian is set, but the detector returned no 'jacobian'"):
        equivariance_loss(det, driving, loss_case["det"](driving), t, 10.0, 10.0)
    values, _ = equivariance_loss(det, driving, det(driving), t, 10.0, 0)              # the value term needs none
    assert sorted(values) == ["equivariance_value"]


def test_the_audio_detectors_output_can_stand_in_for_kp_driving(loss_case):
    cfg = tiny_kp_config(audio=True)
    det_a, _ = _detector(cfg, KPDetector_a, seed=78)
    det_a.requires_grad_(True).eval()
    fmap = (0.05 * torch.randn(3, det_a.out_filters, 16, 16, generator=torch.Generator().manual_seed(4))).to(DEV)
    det, driving = loss_case["det"], loss_case["driving"].to(DEV)
    det.zero_grad(set_to_none=True)
    t = Transform.from_params(loss_case["theta"], loss_case["params"])
    values, _ = equivariance_loss(det, driving, det_a(fmap), t, 10.0, 10.0)
    assert sorted(values) == ["equivariance_jacobian", "equivariance_value"] and all(bool(torch.isfinite(v)) for v in values.values())
    sum(values.values()).backward()
    got = [n for n, p in det_a.named_parameters() if p.grad is not None and float(p.grad.abs().max()) > 0]
    assert got and not any(n.startswith("predictor.") for n in got)
    assert any(p.grad is not None for p in det.parameters())
