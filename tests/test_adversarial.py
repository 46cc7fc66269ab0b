"""Badly conditioned statistics: every other fixture uses He-scaled weights with BatchNorm variance and gain in
[0.75, 1.25]; a trained checkpoint has dead channels, variances over five decades and gains well away from 1, and Winograd
F(4x4,3x3) in fp32 amplifies rounding with the operands' dynamic range.  Fixtures `*_adversarial.npz` (oracle/make_golden.py::
adversarial_case) hold the REFERENCE's outputs on such a network -- BatchNorm variances 1e-4 .. 10 calibrated to the network's
own activations, gains 0.25 .. 4 of either sign, 3 % dead channels, convolution gain x 4, a saturated 0 / 1 source, key points on
the frame border -- together with the reference's own fp32-vs-fp64 distance per output (`*_floor`).

On that network the reference ITSELF is 1e-3 away from its double-precision evaluation at 256x256 (prediction; SURVEY.md 8c's
benign-network tolerance is 1e-4), so the bar per key is max(TOL, 4 x floor) and every test prints error / floor.
CPU: the oracle against the fixtures.  GPU: the three bottleneck forms -- F(4x4), F(2x2), direct -- against the fixtures."""
import numpy as np
import pytest
import torch

from conftest import TOL
from eamm_amd import OcclusionAwareGenerator, hot_path_config, tiny_config
from eamm_amd.weights import adversarial_inputs, adversarial_state_dict
from oracle import eamm_oracle as orc
from test_oracle_golden import load_case, sample

KEYS = ("prediction", "mask", "sparse_deformed", "occlusion_map", "deformed", "deformation")
CASES = [("tiny64_adversarial", tiny_config), ("full256_adversarial", hot_path_config)]


def rebuild(name, cfg):
    """(fixture, state_dict, source, kp_driving, kp_source) -- the weights from the seed + the fixture's calibrated statistics."""
    fx = load_case(name)
    bn = {k[len("bn_mean/"):]: (fx[k], fx["bn_var/" + k[len("bn_mean/"):]]) for k in fx if k.startswith("bn_mean/")}
    sd = adversarial_state_dict(cfg, int(fx["weight_seed"]), bn_stats=bn)
    src, kp_s, kp_d = adversarial_inputs(int(fx["size"]), int(fx["frames"]), cfg["num_kp"], cfg["num_channels"])
    return fx, sd, src, kp_d, kp_s


def compare(tag, out, fx, keys=KEYS):
    rows, bad = [], []
    for k in keys:
        got = sample(out[k].cpu(), k, fx)
        want = torch.from_numpy(fx[k])
        assert got.shape == want.shape, (k, got.shape, want.shape)
        err, floor = float((got - want).abs().max()), float(fx[k + "_floor"])
        bar = max(TOL[k], 4 * floor)
        rows.append(f"{k} {err:.2e} = {err / floor:.2f} x floor {floor:.1e}")
        if not err <= bar:
            bad.append((k, err, bar))
    print("\n" + tag + ":  " + ";  ".join(rows))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("name,cfg_fn", CASES)
def test_fixture_is_adversarial_and_the_oracle_reproduces_it(name, cfg_fn):
    cfg = cfg_fn()
    fx, sd, src, kp_d, kp_s = rebuild(name, cfg)
    lo, med, hi = fx["running_var_range"]
    assert lo < 2e-4 and hi > 5.0 and 1e-3 < med < 1.0          # BatchNorm variances over >= 4.5 decades
    gammas = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("norm.weight") or k.endswith("norm1.weight") or k.endswith("norm2.weight")])
    assert float(gammas.abs().max()) > 3.5 and float(gammas.abs().min()) < 0.3 and float((gammas < 0).float().mean()) > 0.05
    assert set(np.unique(src.numpy())) == {0.0, 1.0} and float(kp_d["value"].abs().max()) == 1.0
    n = kp_d["value"].shape[0]
    with torch.no_grad():
        out = orc.generator_forward(sd, cfg, src.expand(n, -1, -1, -1).contiguous(), kp_d,
                                    {k: v.expand(n, *v.shape[1:]).contiguous() for k, v in kp_s.items()})
    compare(f"oracle vs reference, {name}", out, fx)


@pytest.mark.gpu
@pytest.mark.parametrize("form,env", [(4, {}), (2, {"EAMM_WINO_TILE": "2", "EAMM_WINO_MIN_M": "1"}), (0, {"EAMM_WINO_MIN_M": "-1"})])
@pytest.mark.parametrize("name,cfg_fn", CASES)
def test_hip_forms_on_the_adversarial_network(name, cfg_fn, form, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if form == 4:
        monkeypatch.setenv("EAMM_WINO4_MIN_M", "1")
    cfg = cfg_fn()
    fx, sd, src, kp_d, kp_s = rebuild(name, cfg)
    with torch.no_grad():
        gen = OcclusionAwareGenerator(**cfg)
        gen.load_state_dict(sd, strict=True)
        gen = gen.to("cuda:0").eval()
        n = kp_d["value"].shape[0]
        e = gen.encode_source(src.to("cuda:0"), max_frames=n)
        assert e.bottleneck_form(n) == form
        out = e.forward_frames({k: v.to("cuda:0") for k, v in kp_d.items()}, {k: v.to("cuda:0") for k, v in kp_s.items()},
                               outputs=KEYS)
        e.check_numeric()
    compare(f"HIP form {form} vs reference, {name}", out, fx)


@pytest.mark.gpu
def test_adversarial_network_at_the_timed_16_frame_plan():
    """The forms above run the fixture's two frames in a two-frame call; the benchmark times 16 frames per call at 256x256 (other
    tiles, split-K and chain plans).  Here the fixture's frames are rows 0 .. of a 16-frame call whose remaining rows repeat the
    fixture's driving key points; the fixture's rows are held to the same max(TOL, 4 x floor)."""
    cfg = hot_path_config()
    fx, sd, src, kp_d, kp_s = rebuild("full256_adversarial", cfg)
    n = kp_d["value"].shape[0]
    rows = torch.arange(16) % n
    with torch.no_grad():
        gen = OcclusionAwareGenerator(**cfg)
        gen.load_state_dict(sd, strict=True)
        gen = gen.to("cuda:0").eval()
        e = gen.encode_source(src.to("cuda:0"), max_frames=16)
        assert e.bottleneck_form(16) == 4
        out = e.forward_frames({k: v[rows].to("cuda:0") for k, v in kp_d.items()}, {k: v.to("cuda:0") for k, v in kp_s.items()},
                               outputs=KEYS)
        e.check_numeric()
    assert out["prediction"].shape[0] == 16
    compare("HIP 16-frame plan vs reference, full256_adversarial", {k: v[:n] for k, v in out.items()}, fx)
