"""Audio network AT_net2 (reference modules/util.py:514-612) on the host: the module's checkpoint layout, its refusals, the
pipeline's refusals of mixed inputs, and that the fixtures (tools/make_audio_golden.py) exercise a live recurrence."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from eamm_amd import AudioFeatureNet, animate_from_features
from eamm_amd import _lib
from eamm_amd.weights import audio_feature_state_dict_spec, synthetic_audio_inputs, synthetic_state_dict

FIXTURES = ["audio_small", "audio_batch2", "audio_long"]
CPU_BACKEND = type("B", (), {"device": torch.device("cpu")})()


def test_state_dict_matches_the_reference_layout():
    with open(os.path.join(GOLDEN, "audio_keys.json")) as f:
        ref = [(k, tuple(s)) for k, s in json.load(f)]
    mine = [(k, tuple(v.shape)) for k, v in AudioFeatureNet().state_dict().items()]
    assert len(ref) == 235 and mine == ref
    assert sum(k.startswith("generator.") for k, _ in ref) == 99
    assert [(k, tuple(s)) for k, s, *_ in audio_feature_state_dict_spec()] == ref


def test_strict_load_round_trip_and_decon_child():
    from eamm_amd import DeconvTail
    sd = synthetic_state_dict(None, seed=5, spec=audio_feature_state_dict_spec())
    m = AudioFeatureNet()
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert isinstance(m.decon, DeconvTail)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "lstm.weight_hh_l2"}, strict=True)


def test_public_interface():
    assert list(inspect.signature(AudioFeatureNet.forward).parameters) == ["self", "example_image", "audio", "pose", "jaco_net", "weight"]
    assert inspect.signature(AudioFeatureNet.lstm_features).parameters["weight"].default == 1.6
    params = inspect.signature(animate_from_features).parameters
    assert {"audio_feature", "audio", "pose", "audio_weight"} <= set(params) and params["audio_weight"].default == 1.6
    for name in ("eamm_audio_create", "eamm_audio_destroy", "eamm_audio_last_error", "eamm_audio_load_tensor",
                 "eamm_audio_finalize_weights", "eamm_audio_lstm_features", "eamm_audio_check"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "eamm_hip.h")).read()
    assert "eamm_audio_lstm_features(" in header and "eamm_audio_check(" in header


def test_jaco_net_refusals():
    m = AudioFeatureNet()
    image, audio, pose = synthetic_audio_inputs(1, 2)
    with pytest.raises(NotImplementedError, match="StyleGAN2"):
        m(image, audio, pose, "gan", 1.6)
    with pytest.raises(Exception, match="jaco_net type wrong"):
        m(image, audio, pose, "rnn", 1.6)


@pytest.mark.parametrize("what,shape", [("example_image", (1, 3, 128, 128)), ("example_image", (1, 1, 256, 256)),
                                        ("audio", (1, 4, 28, 13)), ("audio", (1, 4, 12, 28)), ("audio", (2, 4, 28, 12)),
                                        ("pose", (1, 4, 7)), ("pose", (1, 3, 6))])
def test_shape_refusals(what, shape):
    image, audio, pose = synthetic_audio_inputs(1, 4)
    args = {"example_image": image, "audio": audio, "pose": pose}
    args[what] = torch.zeros(shape)
    with pytest.raises(ValueError, match=what):
        AudioFeatureNet().lstm_features(**args)


def test_clip_count_refusal():
    image, audio, pose = torch.zeros(9, 3, 256, 256), torch.zeros(9, 2, 28, 12), torch.zeros(9, 2, 6)
    with pytest.raises(ValueError, match="1 to 8 clips"):
        AudioFeatureNet().lstm_features(image, audio, pose)
    with pytest.raises(ValueError, match="no time steps"):
        AudioFeatureNet().lstm_features(image[:1], audio[:1, :0], pose[:1, :0])


def test_runs_only_on_the_gpu():
    image, audio, pose = synthetic_audio_inputs(1, 2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        AudioFeatureNet().eval().lstm_features(image, audio, pose)


def test_animate_from_features_refuses_mixed_or_partial_audio_inputs():
    net = object()
    a, p = torch.zeros(3, 28, 12), torch.zeros(3, 6)
    with pytest.raises(ValueError, match="either lstm_features"):
        animate_from_features(None, None, None, None, None, torch.zeros(3, 256), audio_feature=net, audio=a, pose=p, backend=CPU_BACKEND)
    with pytest.raises(ValueError, match="either lstm_features"):
        animate_from_features(None, None, None, None, None, torch.zeros(3, 256), audio=a, backend=CPU_BACKEND)
    for kw in ({"audio_feature": net}, {"audio": a}, {"pose": p}, {"audio_feature": net, "audio": a}, {"audio": a, "pose": p}):
        with pytest.raises(ValueError, match="go together"):
            animate_from_features(None, None, None, None, None, None, backend=CPU_BACKEND, **kw)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_are_informative(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert float(z["lstm_saturated"]) < 0.10 and float(z["lstm_std"]) > 0.1
    n, t = int(z["clips"]), int(z["steps"])
    assert z["lstm_out"].shape[:1] == (n,) and z["lstm_out"].shape[-1] == 256
    assert 0 < float(z["floor_lstm_out"]) < 1e-4
    if "lstm_steps" in z.files:
        assert list(z["lstm_steps"][-2:]) == [t - 1 - (t - 1) % 8, t - 1] or int(z["lstm_steps"][-1]) == t - 1
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20
