"""Whole-path parity on the GPU: eamm_amd.OcclusionAwareGenerator (HIP library behind the reference's
module interface) against (a) the fixtures captured from the reference, (b) the CPU oracle on the
same seeded inputs, plus size-independent properties at BASELINE.json's full batch sizes."""
import numpy as np
import pytest
import torch

from conftest import TOL
from eamm_amd import EngineBackend, OcclusionAwareGenerator, animate_clip, hot_path_config, tiny_config
from eamm_amd.weights import synthetic_keypoints, synthetic_source, synthetic_state_dict
from oracle import eamm_oracle as orc
from test_oracle_golden import (NUM_KP_CASES, gray_config, inputs_from_fixture, load_case, num_kp_config, rgba_config, sample,
                                six_channel_config, two_channel_config)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("prediction", "mask", "sparse_deformed", "occlusion_map", "deformed")
_GEN = {}


@pytest.fixture(autouse=True)
def _called_as_demo_py_calls_it():
    """Inference tests run under torch.no_grad(), as the reference's caller does (demo.py:195): with gradients enabled the
    module -- like the reference's -- would build an autograd graph through the differentiable operators instead."""
    with torch.no_grad():
        yield



def generator(cfg_fn):
    """One module per config for the whole session (weights: seed 1234, like the fixtures)."""
    if cfg_fn not in _GEN:
        cfg = cfg_fn()
        gen = OcclusionAwareGenerator(**cfg)
        gen.load_state_dict(synthetic_state_dict(cfg, seed=1234), strict=True)
        _GEN[cfg_fn] = gen.to(DEV).eval()
    return _GEN[cfg_fn]


def cuda(d):
    return {k: v.to(DEV) for k, v in d.items()}


def report(tag, errs):
    print("\n" + tag + "  " + "  ".join(f"{k}={v:.2e}" for k, v in errs.items()))


@pytest.mark.parametrize("name,cfg_fn", [("tiny64_clip3", tiny_config), ("tiny64_batch2", tiny_config),
                                         ("tiny64_nojac", tiny_config), ("full256_clip2", hot_path_config),
                                         ("full512_clip1", hot_path_config),
                                         ("tiny64_gray", gray_config), ("tiny64_two_channels", two_channel_config),
                                         ("tiny64_rgba", rgba_config), ("tiny64_six_channels", six_channel_config)] + NUM_KP_CASES)
def test_module_forward_matches_reference_fixture(name, cfg_fn):
    """Reference contract forward(source, kp_driving, kp_source) -> dict, against reference outputs.  The last two: one and two
    image channels (num_channels; generator.py:14 accepts any) -- [n,C,H,W] in and out, run as the zero-extended RGB network -- and
    four and six (round 5): two groups of three channels through the motion kernels, `final` on the generic 7x7 kernel."""
    cfg = cfg_fn()
    fx = load_case(name)
    sd, src, kp_d, kp_s, n, per_frame = inputs_from_fixture(fx, cfg)
    if not per_frame:
        src = src.expand(n, -1, -1, -1).contiguous()
        kp_s = {k: v.expand(n, *v.shape[1:]).contiguous() for k, v in kp_s.items()}
    gen = generator(cfg_fn)
    out = gen(src.to(DEV), kp_source=cuda(kp_s), kp_driving=cuda(kp_d))  # demo.py:279 argument order
    assert set(out) == set(KEYS)
    errs = {}
    for key in KEYS:
        got = sample(out[key].cpu(), key, fx)
        want = torch.from_numpy(fx[key])
        assert got.shape == want.shape, (key, got.shape, want.shape)
        errs[key] = float((got - want).abs().max())
    report(name, errs)
    for key in KEYS:
        assert errs[key] <= TOL[key], (name, key, errs[key])


def test_gray_clip_interface_and_rgb_only_uint8():
    """One image channel through encode-once + batched frames (chains of ragged size), and the uint8 RGB packing refuses it."""
    cfg = gray_config()
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = generator(gray_config)
    src = synthetic_source(64, seed=1, channels=1)
    kp_s, kp_d = synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(5, 10, seed=2)
    frames, span = animate_clip(EngineBackend(gen, batch=3), src, kp_s, kp_d, 64, 64)
    assert span == (0, 5) and frames.shape == (5, 1, 64, 64)
    ref = orc.generator_forward(sd, cfg, src.expand(5, -1, -1, -1).contiguous(), kp_d,
                                {k: v.expand(5, *v.shape[1:]).contiguous() for k, v in kp_s.items()})["prediction"]
    assert float((frames.cpu() - ref).abs().max()) <= TOL["prediction"]
    with pytest.raises(RuntimeError, match="num_channels == 3"):
        animate_clip(EngineBackend(gen, batch=3), src, kp_s, kp_d, 64, 64, uint8=True)


def test_rgba_clip_interface_and_source_cache_roundtrip():
    """Four image channels through encode-once + batched frames, and the source cache of a two-group handle (two down-sampled
    float4 images + six source planes) exported from one handle and imported into another."""
    cfg = rgba_config()
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = generator(rgba_config)
    src = synthetic_source(64, seed=1, channels=4)
    kp_s, kp_d = synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(5, 10, seed=2)
    frames, span = animate_clip(EngineBackend(gen, batch=3), src, kp_s, kp_d, 64, 64)
    assert span == (0, 5) and frames.shape == (5, 4, 64, 64)
    ref = orc.generator_forward(sd, cfg, src.expand(5, -1, -1, -1).contiguous(), kp_d,
                                {k: v.expand(5, *v.shape[1:]).contiguous() for k, v in kp_s.items()})["prediction"]
    assert float((frames.cpu() - ref).abs().max()) <= TOL["prediction"]
    with pytest.raises(RuntimeError, match="num_channels == 3"):
        animate_clip(EngineBackend(gen, batch=3), src, kp_s, kp_d, 64, 64, uint8=True)
    e1 = gen.encode_source(src.to(DEV), max_frames=3)
    blob = e1.export_source_cache(1)
    g2 = OcclusionAwareGenerator(**cfg)
    g2.load_state_dict(sd, strict=True)
    g2 = g2.to(DEV).eval()
    e2 = g2._ensure_engine(64, 64, 3, 1)
    e2.import_source_cache(blob, 1)
    kd, ks = cuda({k: v[:3] for k, v in kp_d.items()}), cuda(kp_s)
    a = e1.forward_frames(kd, ks, outputs=KEYS)
    b = e2.forward_frames(kd, ks, outputs=KEYS)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def test_rgba_at_the_benchmark_geometry():
    """Four image channels on the SHIPPED configuration at 256x256, 16 frames per call (two whole-pass chains, F(4x4) bottleneck,
    flow head on the column-patch kernel with a 96-channel motion line, `final` on the generic kernel): frames 0, 8 (first of the
    second chain) and 15 against the oracle, every key."""
    cfg = {**hot_path_config(), "num_channels": 4}
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = OcclusionAwareGenerator(**cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    src = synthetic_source(256, seed=1, channels=4)
    kp_s, kp_d = synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(16, 10, seed=2)
    e = gen.encode_source(src.to(DEV), max_frames=16)
    assert e.pass_chains(16) == 2 and e.bottleneck_form(8) == 4
    out = e.forward_frames(cuda(kp_d), cuda(kp_s), outputs=KEYS)
    e.check_numeric()
    assert out["prediction"].shape == (16, 4, 256, 256) and out["sparse_deformed"].shape == (16, 11, 4, 64, 64)
    pick = [0, 8, 15]
    ref = orc.generator_forward(sd, cfg, src.expand(3, -1, -1, -1).contiguous(), {k: v[pick] for k, v in kp_d.items()},
                                {k: v.expand(3, *v.shape[1:]).contiguous() for k, v in kp_s.items()})
    errs = {k: float((out[k][pick].cpu() - ref[k]).abs().max()) for k in KEYS}
    report("rgba 256x256 x 16", errs)
    for k in KEYS:
        assert errs[k] <= TOL[k], (k, errs[k])


def test_internal_flow_matches_fixture():
    cfg = hot_path_config()
    fx = load_case("full256_clip2")
    sd, src, kp_d, kp_s, n, _ = inputs_from_fixture(fx, cfg)
    gen = generator(hot_path_config)
    e = gen.encode_source(src.to(DEV))
    out = e.forward_frames(cuda(kp_d), cuda(kp_s), outputs=("prediction", "deformation"))
    err = float((out["deformation"].cpu() - torch.from_numpy(fx["deformation"])).abs().max())
    assert err <= TOL["deformation"], err


def test_clip_interface_equals_module_forward_and_oracle():
    """encode once + batched frames == per-frame module calls == oracle (tiny config, full tensors)."""
    cfg = tiny_config()
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = generator(tiny_config)
    src, kp_s, kp_d = synthetic_source(64, seed=1), synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(7, 10, seed=2)
    frames, span = animate_clip(EngineBackend(gen, batch=3), src, kp_s, kp_d, 64, 64)  # 3+3+1: ragged last batch
    assert span == (0, 7) and frames.shape == (7, 3, 64, 64)
    ref = np.stack(orc.animate_clip(sd, cfg, src, kp_s, kp_d))  # [T,H,W,3]
    err = np.abs(frames.cpu().numpy().transpose(0, 2, 3, 1) - ref).max()
    assert err <= TOL["prediction"], err
    for t in (0, 6):
        one = gen(src.to(DEV), kp_source=cuda(kp_s), kp_driving=cuda({k: v[t:t + 1] for k, v in kp_d.items()}))
        assert float((one["prediction"][0] - frames[t]).abs().max()) <= 1e-5
    u8, _ = animate_clip(EngineBackend(gen, batch=4), src, kp_s, kp_d, 64, 64, uint8=True)
    assert u8.dtype == torch.uint8 and u8.shape == (7, 64, 64, 3)
    want = np.clip(np.rint(ref * 255), 0, 255)
    assert np.abs(u8.cpu().numpy().astype(np.float32) - want).max() <= 1


def test_full_batch16_properties():
    """BASELINE config 3 size (256x256, 16 frames per launch).  Properties that need no CPU reference:
    (a) frames are independent: frame i of a 16-batch == the same key points run alone;
    (b) permuting the driving frames permutes the outputs; (c) outputs are sigmoid-ranged and finite;
    and, at the launch geometry the benchmark runs (batch-16 tile / split-K / Winograd plans), EVERY output key of
    four of the sixteen frames against the CPU oracle."""
    cfg = hot_path_config()
    gen = generator(hot_path_config)
    src, kp_s, kp_d = synthetic_source(256, seed=1), synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(16, 10, seed=2)
    e = gen.encode_source(src.to(DEV), max_frames=16)
    assert e.bottleneck_form(16) == 4                                   # the form bench.py times
    full = e.forward_frames(cuda(kp_d), cuda(kp_s), outputs=KEYS + ("deformation",))
    pred = full["prediction"]
    assert pred.shape == (16, 3, 256, 256) and torch.isfinite(pred).all()
    assert float(pred.min()) > 0 and float(pred.max()) < 1 and float(pred.std()) > 0.05
    assert float((full["mask"].sum(dim=1) - 1).abs().max()) <= 1e-5  # softmax over the K+1 motions
    for i in (0, 9, 15):
        alone = e.forward_frames(cuda({k: v[i:i + 1] for k, v in kp_d.items()}), cuda(kp_s))["prediction"]
        assert float((alone[0] - pred[i]).abs().max()) <= 2e-5  # split-K plans differ with M: not bit-exact
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(0))
    shuffled = e.forward_frames(cuda({k: v[perm] for k, v in kp_d.items()}), cuda(kp_s))["prediction"]
    assert torch.equal(shuffled, pred[perm.to(DEV)])  # same launch geometry -> bit-exact
    # oracle on four of the sixteen frames, all keys (the oracle needs ~0.4 s per frame at this size)
    sd = synthetic_state_dict(cfg, seed=1234)
    worst = {k: 0.0 for k in KEYS}
    for i in (0, 3, 12, 15):
        with torch.no_grad():
            ref = orc.generator_forward(sd, cfg, src, {k: v[i:i + 1] for k, v in kp_d.items()}, kp_s)
        for k in KEYS:
            worst[k] = max(worst[k], float((full[k][i].cpu() - ref[k][0]).abs().max()))
    report("batch16 vs oracle (frames 0,3,12,15)", worst)
    for k in KEYS:
        assert worst[k] <= TOL[k], (k, worst[k])


def _num_kp_engine(num_kp, size, frames):
    """A generator of the shipped configuration with another num_kp, its source encoded for `frames` frames per call."""
    cfg = {**hot_path_config(), "num_kp": num_kp}
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = OcclusionAwareGenerator(**cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    src, kp_s, kp_d = synthetic_source(size, seed=1), synthetic_keypoints(1, num_kp, seed=0), synthetic_keypoints(frames, num_kp, seed=2)
    return cfg, sd, src, kp_s, kp_d, gen.encode_source(src.to(DEV), max_frames=frames)


def _against_oracle(tag, full, pick, cfg, sd, src, kp_s, kp_d):
    n = len(pick)
    ref = orc.generator_forward(sd, cfg, src.expand(n, -1, -1, -1).contiguous(), {k: v[pick] for k, v in kp_d.items()},
                                {k: v.expand(n, *v.shape[1:]).contiguous() for k, v in kp_s.items()})
    errs = {k: float((full[k][pick].cpu() - ref[k]).abs().max()) for k in KEYS}
    report(tag, errs)
    for k in KEYS:
        assert errs[k] <= TOL[k], (tag, k, errs[k])


@pytest.mark.parametrize("num_kp", [5, 15, 30])
def test_num_kp_at_the_16_frame_launch_geometry(num_kp):
    """num_kp != 10 at the size the benchmark times (256x256, 16 frames per call): K sets the flow head's N = 7(K+2) padding and
    the line width of motion_front_kernel, and both change tile choice with the batch size -- the num_kp fixtures run one or two
    frames only.  Every key of frames 0 and 15 against the oracle, the softmax over the K+1 motions, frame independence."""
    cfg, sd, src, kp_s, kp_d, e = _num_kp_engine(num_kp, 256, 16)
    full = e.forward_frames(cuda(kp_d), cuda(kp_s), outputs=KEYS)
    e.check_numeric()
    assert full["prediction"].shape == (16, 3, 256, 256) and full["mask"].shape == (16, num_kp + 1, 64, 64)
    assert float((full["mask"].sum(dim=1) - 1).abs().max()) <= 1e-5
    alone = e.forward_frames(cuda({k: v[9:10] for k, v in kp_d.items()}), cuda(kp_s))["prediction"]
    assert float((alone[0] - full["prediction"][9]).abs().max()) <= 2e-5
    _against_oracle(f"num_kp {num_kp}, 256x256 x 16 vs oracle (frames 0, 15)", full, [0, 15], cfg, sd, src, kp_s, kp_d)


def test_num_kp_15_at_512_batch8():
    """num_kp = 15 at 512x512, 8 frames per call (the motion grid is 128x128 there): one frame against the oracle, every key."""
    cfg, sd, src, kp_s, kp_d, e = _num_kp_engine(15, 512, 8)
    full = e.forward_frames(cuda(kp_d), cuda(kp_s), outputs=KEYS)
    e.check_numeric()
    assert full["prediction"].shape == (8, 3, 512, 512)
    assert float((full["mask"].sum(dim=1) - 1).abs().max()) <= 1e-5
    alone = e.forward_frames(cuda({k: v[5:6] for k, v in kp_d.items()}), cuda(kp_s))["prediction"]
    assert float((alone[0] - full["prediction"][5]).abs().max()) <= 2e-5
    _against_oracle("num_kp 15, 512x512 x 8 vs oracle (frame 6)", full, [6], cfg, sd, src, kp_s, kp_d)


def test_batch8_512_matches_oracle():
    """BASELINE config 5 size (512x512, batch 8): every output key of two of the eight frames against the CPU oracle at
    the batch-8 launch geometry, the reference fixture's frame inside the batch, and frame independence."""
    cfg = hot_path_config()
    gen = generator(hot_path_config)
    src, kp_s, kp_d = synthetic_source(512, seed=1), synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(8, 10, seed=2)
    e = gen.encode_source(src.to(DEV), max_frames=8)
    full = e.forward_frames(cuda(kp_d), cuda(kp_s), outputs=KEYS)
    pred = full["prediction"]
    assert pred.shape == (8, 3, 512, 512) and torch.isfinite(pred).all()
    alone = e.forward_frames(cuda({k: v[5:6] for k, v in kp_d.items()}), cuda(kp_s))["prediction"]
    assert float((alone[0] - pred[5]).abs().max()) <= 2e-5
    sd = synthetic_state_dict(cfg, seed=1234)
    worst = {k: 0.0 for k in KEYS}
    for i in (2, 7):
        with torch.no_grad():
            ref = orc.generator_forward(sd, cfg, src, {k: v[i:i + 1] for k, v in kp_d.items()}, kp_s)
        for k in KEYS:
            worst[k] = max(worst[k], float((full[k][i].cpu() - ref[k][0]).abs().max()))
    report("512x512 batch8 vs oracle (frames 2,7)", worst)
    for k in KEYS:
        assert worst[k] <= TOL[k], (k, worst[k])
    # frame 0 of this batch is the frame of the reference fixture full512_clip1 (same seeds): reference outputs directly
    fx = load_case("full512_clip1")
    for k in KEYS:
        got = sample(full[k][:1].cpu(), k, fx)
        assert float((got - torch.from_numpy(fx[k])).abs().max()) <= TOL[k], k


def test_edge_cases_and_errors():
    cfg = tiny_config()
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = generator(tiny_config)
    src, kp_s = synthetic_source(64, seed=1), synthetic_keypoints(1, 10, seed=0)
    # key points far outside the frame: all K warps sample zero padding; must match the oracle, no NaN
    kp_far = {"value": torch.full((1, 10, 2), 7.0), "jacobian": torch.eye(2).expand(1, 10, 2, 2).contiguous()}
    out = gen(src.to(DEV), kp_source=cuda(kp_s), kp_driving=cuda(kp_far))
    with torch.no_grad():
        ref = orc.generator_forward(sd, cfg, src, kp_far, kp_s)
    for k in KEYS:
        assert torch.isfinite(out[k]).all()
        assert float((out[k].cpu() - ref[k]).abs().max()) <= TOL[k], k
    # singular driving jacobian: the reference raises from torch.inverse (dense_motion.py:56)
    kp_bad = {"value": torch.zeros(1, 10, 2), "jacobian": torch.zeros(1, 10, 2, 2)}
    with pytest.raises(RuntimeError):
        gen(src.to(DEV), kp_source=cuda(kp_s), kp_driving=cuda(kp_bad))
    # missing key -> KeyError, wrong device -> RuntimeError (SURVEY.md 8b error contract)
    with pytest.raises(KeyError):
        gen(src.to(DEV), kp_source=cuda(kp_s), kp_driving={"jacobian": kp_far["jacobian"].to(DEV)})
    with pytest.raises(RuntimeError):
        gen(src.to(DEV), kp_source=cuda(kp_s), kp_driving=kp_far)  # CPU tensors
    # reloading different weights through load_state_dict must take effect (engine re-packs)
    gen2 = OcclusionAwareGenerator(**cfg).to(DEV).eval()
    gen2.load_state_dict(synthetic_state_dict(cfg, seed=1234))
    kp_d = synthetic_keypoints(1, 10, seed=2)
    a = gen2(src.to(DEV), kp_source=cuda(kp_s), kp_driving=cuda(kp_d))["prediction"].clone()
    gen2.load_state_dict(synthetic_state_dict(cfg, seed=99))
    b = gen2(src.to(DEV), kp_source=cuda(kp_s), kp_driving=cuda(kp_d))["prediction"]
    assert float((a - b).abs().max()) > 1e-3
    with torch.no_grad():
        ref = orc.generator_forward(synthetic_state_dict(cfg, seed=99), cfg, src, kp_d, kp_s)["prediction"]
    assert float((b.cpu() - ref).abs().max()) <= TOL["prediction"]


def test_num_kp_range_is_1_to_30_and_other_values_are_refused_with_the_documented_error():
    """num_kp enters the 4(K+1)-channel hourglass input line, the softmax width of the flow head and its 7(K+2)-column padding; the
    library accepts 1 .. 30 (reference fixtures at 1 / 5 / 15 / 30 above) and refuses the rest by name instead of computing garbage
    (the reference, dense_motion.py:15-18, accepts any K: a documented limit)."""
    src = synthetic_source(64, seed=1).to(DEV)
    for k in (31, 40):
        cfg = num_kp_config(k)()
        gen = OcclusionAwareGenerator(**cfg)
        gen.load_state_dict(synthetic_state_dict(cfg, seed=1234), strict=True)      # the holders take any K ...
        gen = gen.to(DEV).eval()
        with pytest.raises(RuntimeError, match=r"num_kp must be 1 \.\. 30 \(got %d\)" % k):    # ... the engine refuses it at its first use
            gen(src, kp_source=cuda(synthetic_keypoints(1, k, seed=0)), kp_driving=cuda(synthetic_keypoints(1, k, seed=2)))
    # a K that differs between the module and the key points it is fed: the reference fails inside its tensor algebra; here by name
    gen = generator(tiny_config)
    with pytest.raises(RuntimeError):
        gen(src, kp_source=cuda(synthetic_keypoints(1, 10, seed=0)), kp_driving=cuda(synthetic_keypoints(1, 9, seed=2)))


VARIANTS = {
    # name: (config overrides, dense_motion overrides, H, W)
    "rect_64x96": ({}, {}, 64, 96),
    "scale_half": ({}, {"scale_factor": 0.5}, 64, 64),          # motion grid 32x32 vs feature map 16x16: flow is resized
    "scale_one": ({"num_down_blocks": 1}, {"scale_factor": 1, "num_blocks": 2}, 32, 32),   # no anti-alias buffer at all
    "no_occlusion": ({"estimate_occlusion_map": False}, {}, 64, 64),
    "three_down": ({"num_down_blocks": 3, "max_features": 256}, {}, 64, 64),   # feature map 8x8 vs motion grid 16x16
    # widths that are NOT multiples of the kernels' 32-channel granule (VERDICT r03 missing 3; generator.py:14-48 accepts any):
    # generator 48 / 96 / 192, hourglass 80 / 100 / 100 -> 100 / 80 / 40 -- the state_dict is padded at load time
    "odd_widths": ({"block_expansion": 48, "max_features": 200}, {"block_expansion": 40, "max_features": 100}, 64, 64),
    "odd_widths_capped": ({"block_expansion": 24, "max_features": 72, "num_bottleneck_blocks": 3}, {"block_expansion": 20, "max_features": 50}, 64, 64),
    # one / two image channels (run as the zero-extended RGB network) together with the other load-time rewrites
    "gray_scale_one": ({"num_channels": 1}, {"scale_factor": 1}, 64, 64),
    "two_channels_odd_widths": ({"num_channels": 2, "block_expansion": 48, "max_features": 200}, {"block_expansion": 40, "max_features": 100}, 64, 96),
    # four / five image channels (two channel groups) together with the other rewrites: rectangular frame, resized flow, odd widths
    "rgba_scale_half_rect": ({"num_channels": 4}, {"scale_factor": 0.5}, 64, 96),
    "five_channels_odd_widths": ({"num_channels": 5, "block_expansion": 48, "max_features": 200}, {"block_expansion": 40, "max_features": 100}, 64, 64),
    "rgba_scale_one": ({"num_channels": 4, "num_down_blocks": 1}, {"scale_factor": 1, "num_blocks": 2}, 32, 32),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_constructor_variants_match_oracle(name):
    """Constructor variants of the reference module beyond the shipped YAML (generator.py:14-48, dense_motion.py:12-30):
    rectangular frames, other scale factors (flow / occlusion bilinear resize, generator.py:52-56,82-83), no
    occlusion head -- each against the CPU oracle on the same seeded weights."""
    over, dm_over, H, W = VARIANTS[name]
    cfg = tiny_config()
    cfg.update(over)
    cfg["dense_motion_params"] = {**cfg["dense_motion_params"], **dm_over}
    sd = synthetic_state_dict(cfg, seed=4321)
    gen = OcclusionAwareGenerator(**cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    n = 2
    rs = np.random.RandomState(9)
    src = torch.from_numpy(rs.uniform(0, 1, (n, cfg["num_channels"], H, W)).astype(np.float32))
    kp_s, kp_d = synthetic_keypoints(n, 10, seed=0), synthetic_keypoints(n, 10, seed=2)
    out = gen(src.to(DEV), kp_source=cuda(kp_s), kp_driving=cuda(kp_d))
    with torch.no_grad():
        ref = orc.generator_forward(sd, cfg, src, kp_d, kp_s)
    keys = [k for k in KEYS if k in ref]
    assert set(out) == set(keys)
    errs = {k: float((out[k].cpu() - ref[k]).abs().max()) for k in keys}
    report(name, errs)
    for k in keys:
        assert out[k].shape == ref[k].shape and errs[k] <= TOL[k], (name, k, errs[k])


@pytest.mark.parametrize("form,env", [(4, {"EAMM_WINO4_MIN_M": "1"}),
                                      (2, {"EAMM_WINO_TILE": "2", "EAMM_WINO_MIN_M": "1"}),
                                      (0, {"EAMM_WINO_MIN_M": "-1"})])
def test_bottleneck_forms_match_reference_fixture(form, env, monkeypatch):
    """The three forms of the bottleneck convolutions -- Winograd F(4x4,3x3), F(2x2,3x3), direct -- forced through the
    library's knobs (read at eamm_create) on the tiny configuration, each against the reference fixture."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = tiny_config()
    fx = load_case("tiny64_clip3")
    sd, src, kp_d, kp_s, n, _ = inputs_from_fixture(fx, cfg)
    gen = OcclusionAwareGenerator(**cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    e = gen.encode_source(src.to(DEV), max_frames=n)
    assert e.bottleneck_form(n) == form
    pred = e.forward_frames(cuda(kp_d), cuda(kp_s))["prediction"]
    err = float((pred.cpu() - torch.from_numpy(fx["prediction"])).abs().max())
    report(f"bottleneck form {form}", {"prediction": err})
    assert err <= TOL["prediction"]


def test_module_forward_source_cache():
    """forward() skips the source encoder only for the very same, unmodified tensor object; an in-place change or a
    different tensor re-encodes (results must track the data, as in the reference which always re-encodes)."""
    cfg = tiny_config()
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = OcclusionAwareGenerator(**cfg)
    gen.load_state_dict(sd)
    gen = gen.to(DEV).eval()
    kp_s, kp_d = cuda(synthetic_keypoints(1, 10, seed=0)), cuda(synthetic_keypoints(1, 10, seed=2))
    src = synthetic_source(64, seed=1).to(DEV)
    a = gen(src, kp_source=kp_s, kp_driving=kp_d)["prediction"].clone()
    b = gen(src, kp_source=kp_s, kp_driving=kp_d)["prediction"]          # cached encoder
    assert torch.equal(a, b)
    src.mul_(0.5)                                                          # in-place edit of the same object
    c = gen(src, kp_source=kp_s, kp_driving=kp_d)["prediction"]
    with torch.no_grad():
        ref = orc.generator_forward(sd, cfg, src.cpu(), {k: v.cpu() for k, v in kp_d.items()}, {k: v.cpu() for k, v in kp_s.items()})
    assert float((c.cpu() - ref["prediction"]).abs().max()) <= TOL["prediction"] and float((a - c).abs().max()) > 1e-3
    other = synthetic_source(64, seed=5).to(DEV)                           # a different tensor
    d = gen(other, kp_source=kp_s, kp_driving=kp_d)["prediction"]
    assert float((d - c).abs().max()) > 1e-3
    gen.encode_source(src)                                                 # clip API use in between invalidates
    e = gen(other, kp_source=kp_s, kp_driving=kp_d)["prediction"]
    assert torch.equal(d, e)


def test_forward_frames_is_graph_capturable():
    """eamm_forward_frames enqueues only kernels / stream-ordered copies on the caller's stream (no hidden
    synchronisation or allocation), so the launch sequence can be captured into a HIP graph and replayed bit-exactly."""
    gen = generator(tiny_config)
    eng = gen.encode_source(synthetic_source(64, seed=1).to(DEV), max_frames=4)
    kp_s, kp_d = cuda(synthetic_keypoints(1, 10, seed=0)), cuda(synthetic_keypoints(4, 10, seed=2))
    ref = eng.forward_frames(kp_d, kp_s)["prediction"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eng.forward_frames(kp_d, kp_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eng.forward_frames(kp_d, kp_s)["prediction"]
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    kp_d["value"].copy_(cuda(synthetic_keypoints(4, 10, seed=9))["value"])   # new inputs in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eng.forward_frames(kp_d, kp_s)["prediction"])


def test_source_cache_export_import_roundtrip():
    """The multi-GPU broadcast payload: export on one handle, import on another, identical frames."""
    from eamm_amd import Engine
    cfg = tiny_config()
    sd = synthetic_state_dict(cfg, seed=1234)
    src, kp_s, kp_d = synthetic_source(64, seed=1), synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(4, 10, seed=2)
    a, b = Engine(cfg, 64, 64, 4, 1, torch.device(DEV)), Engine(cfg, 64, 64, 4, 1, torch.device(DEV))
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    a.encode_source(src.to(DEV))
    blob = a.export_source_cache(1)
    assert blob.numel() == a.source_cache_numel(1) == 16 * 16 * 128 + 16 * 16 * 4 + 3 * 64 * 64
    b.import_source_cache(blob, 1)
    pa = a.forward_frames(cuda(kp_d), cuda(kp_s))["prediction"]
    pb = b.forward_frames(cuda(kp_d), cuda(kp_s))["prediction"]
    assert torch.equal(pa, pb)
    with pytest.raises(RuntimeError):
        Engine(cfg, 64, 64, 4, 1, torch.device(DEV)).forward_frames(cuda(kp_d), cuda(kp_s))  # nothing encoded
    a.close(); b.close()


def test_generator_without_motion_network():
    """dense_motion_params=None (reference generator.py:18-23, 64): the module has no dense_motion_network, forward
    returns 'prediction' only and never reads the key points; against the reference's own output (fixture)."""
    cfg = tiny_config()
    cfg["dense_motion_params"], cfg["estimate_occlusion_map"] = None, False
    fx = load_case("tiny64_nomotion")
    sd = synthetic_state_dict(cfg, seed=int(fx["weight_seed"]))
    gen = OcclusionAwareGenerator(**cfg)
    assert gen.dense_motion_network is None and not any(k.startswith("dense_motion_network") for k in gen.state_dict())
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    src = synthetic_source(64, seed=int(fx["source_seed"]), batch=2).to(DEV)
    out = gen(src, kp_driving=None, kp_source=None)
    assert sorted(out) == ["prediction"]
    err = float((out["prediction"].cpu() - torch.from_numpy(fx["prediction"])).abs().max())
    report("no motion network", {"prediction": err})
    assert err <= TOL["prediction"]
    with pytest.raises(KeyError):
        gen.engine.forward_frames({"value": torch.zeros(2, 10, 2, device=DEV)}, {"value": torch.zeros(2, 10, 2, device=DEV)},
                                  outputs=("prediction", "mask"))
    # the direct convolution form of the bottleneck takes its first pre-activation from the broadcast kernel
    import os
    os.environ["EAMM_WINO_MIN_M"] = "-1"
    try:
        gen2 = OcclusionAwareGenerator(**cfg)
        gen2.load_state_dict(sd, strict=True)
        out2 = gen2.to(DEV).eval()(src, kp_driving=None, kp_source=None)
    finally:
        del os.environ["EAMM_WINO_MIN_M"]
    assert float((out2["prediction"].cpu() - torch.from_numpy(fx["prediction"])).abs().max()) <= TOL["prediction"]


def test_chained_bottleneck_graph_capture_and_equivalence(monkeypatch):
    """At 16 frames the call runs as two chains of 8 frames on two streams forked from / joined into the caller's stream
    (eamm_bottleneck_chains; since round 2 the chains cover the whole per-frame pass, eamm_pass_chains; with
    EAMM_PASS_CHAINS=1 only the bottleneck).  (a) The fork / join is capturable: a HIP graph of the call replays
    bit-exactly.  (b) One chain, bottleneck-only chains and whole-pass chains compute every frame the same way up to the
    launch plans that depend on the frames per launch (split-K, transform-point groups): the frames must agree to rounding."""
    cfg = hot_path_config()
    gen = generator(hot_path_config)
    src, kp_s, kp_d = synthetic_source(256, seed=1), synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(16, 10, seed=2)
    eng = gen.encode_source(src.to(DEV), max_frames=16)
    assert eng.bottleneck_chains(16) == 2 and eng.pass_chains(16) == 2 and eng.bottleneck_chains(2) == 1 and eng.pass_chains(8) == 1
    kd, ks = cuda(kp_d), cuda(kp_s)
    ref = eng.forward_frames(kd, ks)["prediction"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.forward_frames(kd, ks)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eng.forward_frames(kd, ks)["prediction"]
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    def fresh_engine():
        g2 = OcclusionAwareGenerator(**cfg)
        g2.load_state_dict(synthetic_state_dict(cfg, seed=1234), strict=True)
        return g2.to(DEV).eval().encode_source(src.to(DEV), max_frames=16)

    monkeypatch.setenv("EAMM_PASS_CHAINS", "1")          # chains inside the bottleneck only (the round-2 start state)
    e2 = fresh_engine()
    assert e2.bottleneck_chains(16) == 2 and e2.pass_chains(16) == 1
    inner = e2.forward_frames(kd, ks)["prediction"]
    assert float((inner - ref).abs().max()) <= 2e-5
    monkeypatch.setenv("EAMM_BNECK_CHAINS", "1")         # ... and none at all
    e1 = fresh_engine()
    assert e1.bottleneck_chains(16) == 1
    one = e1.forward_frames(kd, ks)["prediction"]
    assert float((one - ref).abs().max()) <= 2e-5


@pytest.mark.parametrize("n", [9, 11, 13])
def test_odd_frame_counts_across_the_chain_thresholds(n):
    """Calls whose frame count straddles the launch-plan switches at 256x256: 9 frames (bottleneck chains only), 11 and 13
    (two whole-pass chains of UNEQUAL length: 6 + 5, 7 + 6).  First, middle and last frame of each call against the oracle,
    and every frame against the same frames computed in a 16-frame call (frames are independent: launch plans must not
    change them beyond rounding)."""
    from eamm_amd import hot_path_config as hot
    cfg = hot()
    sd = synthetic_state_dict(cfg, seed=1234)
    gen = OcclusionAwareGenerator(**cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    src, kp_s, kp_d = synthetic_source(256, seed=1), synthetic_keypoints(1, 10, seed=0), synthetic_keypoints(16, 10, seed=2)
    eng = gen.encode_source(src.to(DEV), max_frames=16)
    kd, ks = cuda(kp_d), cuda(kp_s)
    full = eng.forward_frames(kd, ks)["prediction"].clone()
    part = eng.forward_frames({k: v[:n] for k, v in kd.items()}, ks)["prediction"]
    assert part.shape[0] == n
    assert float((part - full[:n]).abs().max()) <= 2e-5
    for t in (0, n // 2, n - 1):
        with torch.no_grad():
            ref = orc.generator_forward(sd, cfg, src, {k: v[t:t + 1] for k, v in kp_d.items()}, kp_s)["prediction"]
        assert float((part[t].cpu() - ref[0]).abs().max()) <= TOL["prediction"], (n, t)


def test_deepcopy_of_a_module_with_a_live_engine():
    """a copy must not share (or try to copy) the library handle, nor read the original's tensors."""
    import copy
    cfg = tiny_config()
    gen = OcclusionAwareGenerator(**cfg)
    gen.load_state_dict(synthetic_state_dict(cfg, seed=1234), strict=True)
    gen = gen.to(DEV).eval()
    src = synthetic_source(64, seed=1).to(DEV)
    kp_s, kp_d = cuda(synthetic_keypoints(1, 10, seed=0)), cuda(synthetic_keypoints(1, 10, seed=2))
    a = gen(src, kp_source=kp_s, kp_driving=kp_d)["prediction"].clone()
    twin = copy.deepcopy(gen)
    assert twin.engine is None and gen.engine is not None
    with torch.no_grad():
        twin.final.bias.add_(0.25)                                   # the copy's own tensors
    b = twin(src, kp_source=kp_s, kp_driving=kp_d)["prediction"]
    assert twin.engine is not gen.engine and float((a - b).abs().max()) > 1e-3
    assert torch.equal(gen(src, kp_source=kp_s, kp_driving=kp_d)["prediction"], a)   # the original is untouched
