"""The binding's one handle class and its shared helpers (eamm_amd/_handle.py): keys and create refusals on the host; on the
GPU the life cycle of a handle behind each of its owners -- reuse, rebuild on replaced weights, growth, a failed load, and the
generator engine's create / set_training / load order."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN, TOL
from eamm_amd import (AudioFeatureNet, DeconvTail, EmotionDetector, KPDetector, KPDetector_a, OcclusionAwareGenerator, _lib, tiny_config,
                      tiny_kp_config)
from eamm_amd._handle import Handle, weights_key
from eamm_amd.engine import Engine
from eamm_amd.weights import deconv_state_dict_spec, synthetic_keypoints, synthetic_source, synthetic_state_dict
from oracle import eamm_oracle as orc
from test_deconv_tail import TOL as TOL_DECONV
from test_emotion_detector import OUTPUTS as EMO_OUTPUTS, errors as emo_errors, load as load_emo, make as make_emo, tolerance as emo_tolerance
from test_kp_detector import TOL_KP, load as load_kp
from test_oracle_golden import inputs_from_fixture, load_case, sample

DEV = "cuda:0"


def same_version_replacement(old: torch.Tensor) -> nn.Parameter:
    """A new parameter of other values whose version counter equals ``old``'s (no-op in-place writes bump it)."""
    new = nn.Parameter(old.detach() * 0.5 + 0.125, requires_grad=False)
    with torch.no_grad():
        while new._version < old._version:
            new.add_(0)
    assert new is not old and new._version == old._version, (new._version, old._version)
    return new


# ---- host ----------------------------------------------------------------------------------------------------------------
def test_weights_key_sees_in_place_writes_and_replaced_tensors():
    ts = [torch.zeros(3), nn.Parameter(torch.ones(2, 2)), torch.arange(4.0)]
    key = weights_key(ts)
    assert weights_key(ts) == key and weights_key(iter(ts)) == key
    with torch.no_grad():
        ts[1].mul_(2.0)
    written = weights_key(ts)
    assert written != key
    ts[1] = same_version_replacement(ts[1])      # same counter, another tensor
    assert weights_key(ts) != written


def test_audio_key_ignores_the_generator_and_decon_entries():
    net = AudioFeatureNet()
    dev = torch.device("cpu")
    key, named = net._keyed_tensors(dev)
    names = [n for n, _ in named]
    assert names and not any(n.startswith(("generator.", "decon.")) for n in names)
    assert any(k.startswith("generator.") for k in net.state_dict()) and any(k.startswith("decon.") for k in net.state_dict())
    with torch.no_grad():
        next(net.generator.parameters()).add_(1.0)
        net.decon[0].weight.add_(1.0)
    assert net._keyed_tensors(dev)[0] == key
    with torch.no_grad():
        net.lstm.weight_hh_l0.add_(1.0)
    assert net._keyed_tensors(dev)[0] != key


def _refused_configs():
    gen = _lib.EammConfig(num_channels=3, num_kp=40)
    kp = _lib.EammKpConfig(num_channels=3, num_kp=40)
    emo = _lib.EammEmoConfig(num_channels=9)           # eamm_emo_create: num_channels must be 1 .. 8
    audio = _lib.EammAudioConfig(max_batch=4)          # eamm_audio_create: max_batch must be 8 .. 4096
    deconv = _lib.EammDeconvConfig(num_layers=1)
    return [("eamm_", gen, "num_kp must be 1 .. 30 (got 40): the flow head"), ("eamm_kp_", kp, "error -1: num_kp must be 1 .. 30 (got 40)"),
            ("eamm_deconv_", deconv, "num_layers must be in [2,8]"), ("eamm_emo_", emo, "num_channels must be 1 .. 8 (got 9)"),
            ("eamm_audio_", audio, "max_batch must be 8 .. 4096 (got 4)")]


def test_create_refusals_report_their_own_family():
    cases = _refused_configs()
    assert sorted(p for p, *_ in cases) == sorted(_lib.FAMILIES)
    # each family twice, the second time after every other family: a refusal never reports the previous family's text
    for prefix, cfg, text in cases + cases[::-1]:
        with pytest.raises(_lib.EammError) as e:
            Handle(prefix, cfg, torch.device("cuda", 0))
        assert e.value.code == _lib.ERR_ARG and text in str(e.value), (prefix, str(e.value))
        if prefix == "eamm_kp_":
            assert str(e.value).endswith(text)            # (the generator's message goes on: "... the flow head ...")


def test_check_without_a_handle():
    _lib.check(0)
    _lib.check(0, None)
    with pytest.raises(_lib.EammError) as e:
        _lib.check(_lib.ERR_ARG, None)
    assert e.value.code == _lib.ERR_ARG


# ---- GPU -----------------------------------------------------------------------------------------------------------------
DECONV_CHANNELS = (64, 32, 19)           # two layers, the fewest eamm_deconv_create takes: 1x1 -> 4x4 -> 8x8


def _kp_case(audio):
    name, cfg = ("kpa_tiny", tiny_kp_config(audio=True)) if audio else ("kp_tiny64", tiny_kp_config())
    fx, sd, x = load_kp(name, cfg, audio)

    def make(state=sd):
        m = (KPDetector_a if audio else KPDetector)(**cfg, max_batch=1)
        m.load_state_dict(state, strict=True)
        return m.to(DEV).eval()

    def matches_fixture(out):
        return all(float((out[k].cpu() - torch.from_numpy(fx[k])).abs().max()) <= TOL_KP[k] for k in ("value", "jacobian", "heatmap"))
    return make, (lambda m, xs: m(xs)), x.to(DEV), (lambda m: (m.kp, "weight")), matches_fixture


def _deconv_case():
    sd = synthetic_state_dict(None, seed=3, spec=deconv_state_dict_spec(DECONV_CHANNELS))
    x = torch.randn(3, DECONV_CHANNELS[0], generator=torch.Generator().manual_seed(0))
    ref = orc.deconv_tail(sd, x)

    def make(state=sd):
        m = DeconvTail(channels=DECONV_CHANNELS, max_batch=1)
        m.load_state_dict(state, strict=True)
        return m.to(DEV).eval()
    return (make, (lambda m, xs: {"out": m(xs)}), x.to(DEV), (lambda m: (m[0], "weight")),
            lambda out: float((out["out"].cpu() - ref).abs().max()) <= TOL_DECONV)


def _emo_case():
    fx, cfg, x, kp = load_emo("emotion_tiny128")
    kp = {k: v.to(DEV) for k, v in kp.items()}
    sd = make_emo(cfg, int(fx["weight_seed"])).state_dict()

    def make(state=sd):
        m = EmotionDetector(**cfg, max_batch=8)
        m.load_state_dict(state, strict=True)
        return m.to(DEV).eval()

    def run(m, xs):
        n = xs.shape[0]
        return m.detect(xs, kp["value"][:n], kp["jacobian"][:n])

    def matches_fixture(out):
        err = emo_errors(out, fx)
        return all(err[k] <= emo_tolerance(fx, k) for k in EMO_OUTPUTS)
    return make, run, x.to(DEV), (lambda m: (m.conv1, "weight")), matches_fixture


CASES = {"KPDetector": lambda: _kp_case(False), "KPDetector_a": lambda: _kp_case(True), "DeconvTail": _deconv_case,
         "EmotionDetector": _emo_case}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_replaced_weight_rebuilds_the_handle(name):
    """A loaded parameter replaced by another tensor with the SAME version counter: the handle is keyed on identity and version
    (``weights_key``), so the next call runs the new weights.  (Keyed on the version counters alone, the old weights kept running.)"""
    make, run, x, slot, matches_fixture = CASES[name]()
    grows = name != "EmotionDetector"        # kp / deconv rebuild larger; the emotion detector chunks by its cap
    small = x[:1] if grows else x
    m = make()
    with torch.no_grad():
        first = run(m, small)
        h = m._handle
        assert isinstance(h, Handle) and h.ptr is not None
        again = run(m, small)
        assert m._handle is h and all(torch.equal(first[k], again[k]) for k in first)       # unchanged weights: the same handle
        if grows:
            assert m._cap == 1 and x.shape[0] > 1
            whole = run(m, x)                                                                # beyond the capacity: a new, larger handle
            assert m._handle is not h and h.ptr is None and m._cap == x.shape[0]
            h = m._handle
        else:
            whole = first
        assert matches_fixture(whole)
        owner, attr = slot(m)
        setattr(owner, attr, same_version_replacement(getattr(owner, attr)))
        second = run(m, x)
        assert m._handle is not h and h.ptr is None
        want = run(make(m.state_dict()), x)                                                  # a fresh module holding the new weights
    assert all(torch.equal(second[k], want[k]) for k in want)
    assert any(not torch.equal(second[k], whole[k]) for k in whole)


@pytest.mark.gpu
def test_failed_load_destroys_the_handle():
    cs = _lib.EammDeconvConfig(num_layers=len(DECONV_CHANNELS) - 1, max_batch=1)
    cs.channels[:len(DECONV_CHANNELS)] = DECONV_CHANNELS
    sd = synthetic_state_dict(None, seed=3, spec=deconv_state_dict_spec(DECONV_CHANNELS))
    sd["0.weight"] = sd["0.weight"][:, :, :4, :4]        # the first layer's filter is 6x6
    h = Handle("eamm_deconv_", cs, torch.device(DEV))
    assert h.ptr is not None
    with pytest.raises(_lib.EammError, match="0.weight missing or mis-shaped") as e:
        h.load(sd.items())
    assert e.value.code == _lib.ERR_KEY and h.ptr is None
    h.close()
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("training", [False, True])
def test_engine_opens_and_closes_twice(training):
    """create -> set_training -> load through ``Handle``, a forward against the reference fixture, close; then all of it again."""
    cfg = tiny_config()
    for _ in range(2):
        with torch.no_grad():
            if training:
                z = np.load(os.path.join(GOLDEN, "tiny64_train.npz"))
                n = int(z["n"])
                gen = OcclusionAwareGenerator(**cfg)
                gen.load_state_dict(synthetic_state_dict(cfg, seed=int(z["weight_seed"])), strict=True)
                gen = gen.to(DEV)
                e = Engine(cfg, 64, 64, max_frames=n, max_sources=n, device=torch.device(DEV), training=True)
                e.load_state_dict(gen.state_dict())
                kp_s, kp_d = synthetic_keypoints(n, 10, seed=0), synthetic_keypoints(n, 10, seed=2)
                out = e.train_forward(synthetic_source(64, seed=1, batch=n).to(DEV), {k: v.to(DEV) for k, v in kp_d.items()},
                                      {k: v.to(DEV) for k, v in kp_s.items()}, gen._norm_modules())
                got, want = out["prediction"].cpu(), torch.from_numpy(z["single_prediction"])
            else:
                fx = load_case("tiny64_clip3")
                sd, src, kp_d, kp_s, n, per_frame = inputs_from_fixture(fx, cfg)
                assert not per_frame
                e = Engine(cfg, 64, 64, max_frames=n, max_sources=1, device=torch.device(DEV))
                e.load_state_dict(sd)
                e.encode_source(src.to(DEV))
                out = e.forward_frames({k: v.to(DEV) for k, v in kp_d.items()}, {k: v.to(DEV) for k, v in kp_s.items()})
                got, want = sample(out["prediction"].cpu(), "prediction", fx), torch.from_numpy(fx["prediction"])
            e.check_numeric()
        assert got.shape == want.shape and float((got - want).abs().max()) <= TOL["prediction"]
        e.close()
        assert e._handle.ptr is None
        e.close()
