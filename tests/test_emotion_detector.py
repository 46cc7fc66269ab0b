"""Emotion detector Emotion_k (reference modules/util.py:1223-1527): the module's checkpoint layout and argument checks on the
host, and the HIP forward against fixtures captured from the reference on the CPU (tools/make_emotion_golden.py) on the GPU."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from eamm_amd import EmotionDetector, animate_from_features, emotion_detector_config
from eamm_amd import _lib
from eamm_amd.weights import emotion_state_dict_spec, synthetic_keypoints, synthetic_source, synthetic_state_dict

DEV = "cuda:0"
CASES = ["emotion_tiny128", "emotion_full256", "emotion_full256_wide"]
OUTPUTS = ("value", "jacobian", "fake", "feature")


def make(cfg, seed, **kw):
    m = EmotionDetector(**cfg, **kw)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed, spec=emotion_state_dict_spec(cfg)), strict=True)
    return m


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    fx = {k: z[k] for k in z.files}
    cfg = json.loads(str(fx["config"]))
    n, size = int(fx["frames"]), int(fx["size"])
    x = synthetic_source(size, seed=int(fx["image_seed"]), batch=n)
    kp = synthetic_keypoints(n, 10, seed=int(fx["kp_seed"]))
    if float(fx["jac_scale"]) > 0:
        rs = np.random.RandomState(int(fx["kp_seed"]) + 1000)
        s = float(fx["jac_scale"])
        kp["jacobian"] = torch.from_numpy(rs.uniform(-s, s, (n, 10, 2, 2)).astype(np.float32))
    return fx, cfg, x, kp


# ---- host ----------------------------------------------------------------------------------------------------------------
def test_state_dict_matches_the_reference_layout():
    with open(os.path.join(GOLDEN, "emotion_keys.json")) as f:
        ref = [(k, tuple(s)) for k, s in json.load(f)]
    m = EmotionDetector(**emotion_detector_config())
    mine = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert len(ref) == 223 and mine == ref
    spec = emotion_state_dict_spec(emotion_detector_config())
    assert [(k, tuple(s)) for k, s, *_ in spec] == ref


def test_strict_load_round_trip():
    cfg = emotion_detector_config()
    sd = synthetic_state_dict(cfg, seed=5, spec=emotion_state_dict_spec(cfg))
    m = EmotionDetector(**cfg)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "fc_p.0.weight"}, strict=True)


def test_refusals():
    cfg = emotion_detector_config()
    with pytest.raises(ValueError, match="scale_factor"):
        EmotionDetector(**{**cfg, "scale_factor": 0.3})
    m = EmotionDetector(**cfg).eval()
    x = torch.zeros(2, 3, 256, 256)
    kp5 = synthetic_keypoints(2, 5, seed=1)
    with pytest.raises(ValueError, match="num_kp 10"):
        m._check_inputs(x, kp5["value"], kp5["jacobian"])
    m.conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        m.feature(x)


def test_public_interface():
    assert {"forward", "feature", "detect"} <= set(dir(EmotionDetector))
    params = inspect.signature(animate_from_features).parameters
    assert "emo_detector" in params and "emotion_frames" in params
    assert _lib.ABI_VERSION == 6
    for name in ("eamm_emo_create", "eamm_emo_destroy", "eamm_emo_last_error", "eamm_emo_load_tensor", "eamm_emo_finalize_weights",
                 "eamm_emo_detect"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "eamm_hip.h")).read()
    assert "#define EAMM_ABI_VERSION 6" in header and "eamm_emo_detect(" in header
    assert [f for f, _ in _lib.EammEmoOutputs._fields_] == list(OUTPUTS)


def test_animate_from_features_refuses_both_emotion_sources():
    with pytest.raises(ValueError, match="either emo_driving"):
        animate_from_features(None, None, None, None, None, None, emo_driving={"value": torch.zeros(1, 4, 2)},
                              emo_detector=object(), emotion_frames=torch.zeros(1, 3, 8, 8),
                              backend=type("B", (), {"device": torch.device("cpu")})())


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def errors(out, fx):
    return {k: float((out[k].cpu() - torch.from_numpy(fx[k])).abs().max()) for k in OUTPUTS}


def tolerance(fx, k):
    return max(1e-4, 4.0 * float(fx["floor_" + k]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_detector_matches_reference_fixture(name):
    fx, cfg, x, kp = load(name)
    m = make(cfg, int(fx["weight_seed"]), max_batch=8).to(DEV).eval()
    out = m.detect(x.to(DEV), kp["value"].to(DEV), kp["jacobian"].to(DEV))
    err = errors(out, fx)
    tol = {k: tolerance(fx, k) for k in OUTPUTS}
    assert all(err[k] <= tol[k] for k in OUTPUTS), f"{name}: max|hip - reference| {err}, tolerance {tol}"
    # forward / feature are the same pass
    kpo, fake = m(x.to(DEV), kp["value"].to(DEV), kp["jacobian"].to(DEV))
    assert torch.equal(fake, out["fake"]) and torch.equal(kpo["value"], out["value"]) and torch.equal(kpo["jacobian"], out["jacobian"])
    assert torch.equal(m.feature(x.to(DEV)), out["feature"])


@pytest.mark.gpu
def test_batch_invariance_and_determinism():
    fx, cfg, x, kp = load("emotion_full256")
    m = make(cfg, int(fx["weight_seed"]), max_batch=64).to(DEV).eval()
    n = 64
    xb = synthetic_source(256, seed=int(fx["image_seed"]), batch=n).to(DEV)
    kpb = synthetic_keypoints(n, 10, seed=int(fx["kp_seed"]))
    kpb = {k: v.to(DEV) for k, v in kpb.items()}
    big = m.detect(xb, kpb["value"], kpb["jacobian"])
    small = m.detect(xb[:4], kpb["value"][:4], kpb["jacobian"][:4])
    err = {k: float((big[k][:4] - small[k]).abs().max()) for k in OUTPUTS}
    assert all(err[k] <= tolerance(fx, k) for k in OUTPUTS), f"frames 0-3 alone vs in a batch of 64: {err}"
    again = m.detect(xb, kpb["value"], kpb["jacobian"])
    assert all(torch.equal(big[k], again[k]) for k in OUTPUTS)
    # batches beyond max_batch are chunked
    m.max_batch = 16
    chunked = m.detect(xb[:40], kpb["value"][:40], kpb["jacobian"][:40])
    err = {k: float((big[k][:40] - chunked[k]).abs().max()) for k in OUTPUTS}
    assert all(err[k] <= tolerance(fx, k) for k in OUTPUTS), err
