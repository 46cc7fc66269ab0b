"""AudioFeatureNet (AT_net2) and DeconvTail as trainable modules: the HIP operators of ``eamm_amd.audio_ops`` (csrc/lstm_backward.hip,
audio_backward.hip) against ATen differentiated in float64 on the CPU, and the modules' differentiable forward against training
steps of the reference itself (tests/golden/audio_eval_backward.npz, audio_train_backward.npz; tools/make_audio_train_golden.py).

Operator bars (tests/closeness.py), per tensor, relative to its largest float64 entry: 2e-5, provided ATen's own CPU fp32
run stays under a quarter of it on the same inputs; otherwise 4 x that run's distance.  No element may lie beyond the bar.
Module bars: tests/test_gpu_emotion_backward.py's rule, see ``check_module``.

Measured on an MI355X, error relative to the tensor's largest entry (ATen's CPU fp32 run in brackets); every operator case is under the
2e-5 bar, and ATen's fp32 run is under a quarter of it everywhere, so no case takes the 4 x rule:
  lstm_layer               y 1.0e-7 .. 1.5e-7 (1.1e-7 .. 1.5e-7), dxproj 0.8e-7 .. 1.6e-7 (1.1e-7 .. 2.9e-7), dW_hh 0 .. 2.3e-7 (0 .. 2.4e-7)
  conv_transpose4s2_nhwc   forward 1.2e-7 .. 1.0e-6 (1.2e-7 .. 7.7e-7), data gradient 1.1e-7 .. 1.4e-6 (0.8e-7 .. 6.0e-7),
                           weight gradient 0.3e-7 .. 3.4e-7 (0.3e-7 .. 6.6e-7), bias gradient 2.8e-8 .. 3.1e-8 (5.9e-8 .. 1.7e-6)
  maxpool3_nhwc            forward and backward bit-equal to ATen
  network, .eval()         deco_out 1.3e-6 (bar 1e-4); gradients: worst error 3.2 bars on ONE of 512 samples of audio_eocder.5.1.bias
                           (1.6e-2 of the tensor's largest entry), 3 of 2016 samples of input/audio beyond their bar, every other
                           tensor inside it; the image encoder, fc, LSTM and decon tensors at 1e-12 .. 4e-6, the audio CNN's at
                           5e-4 .. 3e-3.  Those audio-CNN figures are not the kernels': ATen's own CPU fp32 run of this composition gives
                           the SAME figures (5.1.bias 1.61e-2, 3.0.weight 1.18e-3, input/audio 5.4e-3) as soon as its convolution
                           outputs are perturbed by 1e-7 of their largest entry -- a few activations of the synthetic clip sit on a
                           ReLU / max-pool boundary and any rounding other than ATen's flips them (the rule's allowance).
  network, .train()        deco_out 2.1e-5 (bar 1e-4); every gradient sample inside its bar, worst 0.38 bars; buffers within 1e-5,
                           num_batches_tracked + T
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from closeness import close
from conftest import GOLDEN
from eamm_amd import AudioFeatureNet, KPDetector_a, audio_ops, tiny_kp_config
from eamm_amd.weights import audio_feature_state_dict_spec, kp_state_dict_spec, synthetic_audio_inputs, synthetic_state_dict

DEV = "cuda:0"
FP32_MIN_REL = 5e-3       # tests/test_train_backward.py


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- LSTM layer ------------------------------------------------------------------------------------------------------------------
# (N, T): no hand-off; one hand-off; both parity buffers reused; N > 4 (each thread of the forward carries two gate rows); the largest N
LSTM_SHAPES = [(1, 1), (1, 2), (3, 5), (5, 4), (8, 5)]


@functools.lru_cache(maxsize=None)
def lstm_reference(shape):
    n, t = shape
    g = torch.Generator().manual_seed(1000 + 10 * n + t)
    lstm = torch.nn.LSTM(64, 256, 1, batch_first=True)
    with torch.no_grad():
        for q in lstm.parameters():
            q.copy_(torch.randn(q.shape, generator=g) * (0.25 if q.dim() == 1 else 1.0 / 16.0))
    x = torch.randn(n, t, 64, generator=g)
    gy = torch.randn(n, t, 256, generator=g)
    xproj = (F.linear(x.double(), lstm.weight_ih_l0.double(), lstm.bias_ih_l0.double()) + lstm.bias_hh_l0.double()).detach().float()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        # the operator's own inputs: the projection as a leaf, the recurrence written out as nn.LSTM computes it
        xp = xproj.to(dtype).clone().requires_grad_()
        w = lstm.weight_hh_l0.detach().to(dtype).clone().requires_grad_()
        h = torch.zeros(n, 256, dtype=dtype)
        c = torch.zeros(n, 256, dtype=dtype)
        ys = []
        for s in range(t):
            i, f, gg, o = (xp[:, s] + h @ w.t()).chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            ys.append(h)
        y = torch.stack(ys, dim=1)
        (y * gy.to(dtype)).sum().backward()
        ref[dtype] = (y.detach(), xp.grad, w.grad)
    # ... and that written-out recurrence IS nn.LSTM's
    with torch.no_grad():
        y_mod, _ = lstm.double()(x.double())
    assert float((y_mod - ref[torch.float64][0]).abs().max()) < 1e-6   # xproj was rounded to fp32
    return xproj, lstm.weight_hh_l0.detach().float().clone(), gy, ref


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LSTM_SHAPES)
def test_lstm_layer_forward_and_gradients_against_float64_aten(shape):
    xproj, whh, gy, ref = lstm_reference(shape)
    (y64, dx64, dw64), (y32, dx32, dw32) = ref[torch.float64], ref[torch.float32]
    xg, wg = xproj.to(DEV).requires_grad_(), whh.to(DEV).requires_grad_()
    y = audio_ops.lstm_layer(xg, wg)
    assert tuple(y.shape) == (shape[0], shape[1], 256)
    (y * gy.to(DEV)).sum().backward()
    audio_ops.lstm_check(DEV)
    close(y, y64, y32, f"lstm {shape} y")
    close(xg.grad, dx64, dx32, f"lstm {shape} dxproj")
    close(wg.grad, dw64, dw32, f"lstm {shape} dW_hh")


# ---- ConvTranspose2d(k4, s2, p1) -------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout)
DECONV_SHAPES = [(1, 1, 1, 32, 32), (3, 4, 4, 64, 35), (2, 5, 3, 256, 128), (1, 32, 32, 128, 35)]


@functools.lru_cache(maxsize=None)
def deconv_reference(shape):
    b, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cin, cout, 4, 4, generator=g) / (cin * 4) ** 0.5
    bias = 0.1 * torch.randn(cout, generator=g)
    gy = torch.randn(b, cout, 2 * h, 2 * w, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        xl, wl, bl = (v.to(dtype).clone().requires_grad_() for v in (x, wt, bias))
        y = F.conv_transpose2d(xl, wl, bl, stride=2, padding=1)
        (y * gy.to(dtype)).sum().backward()
        ref[dtype] = (y.detach(), xl.grad, wl.grad, bl.grad)
    return x, wt, bias, gy, ref


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DECONV_SHAPES)
def test_conv_transpose4s2_forward_and_gradients_against_float64_aten(shape):
    x, wt, bias, gy, ref = deconv_reference(shape)
    (y64, dx64, dw64, db64), (y32, dx32, dw32, db32) = ref[torch.float64], ref[torch.float32]
    xg, wg, bg = nhwc(x).to(DEV).requires_grad_(), wt.to(DEV).requires_grad_(), bias.to(DEV).requires_grad_()
    y = audio_ops.conv_transpose4s2_nhwc(xg, wg, bg)
    assert tuple(y.shape) == (shape[0], 2 * shape[1], 2 * shape[2], shape[4])
    (y * nhwc(gy).to(DEV)).sum().backward()
    close(y, nhwc(y64), nhwc(y32), f"deconv {shape} forward")
    close(xg.grad, nhwc(dx64), nhwc(dx32), f"deconv {shape} data gradient")
    close(wg.grad, dw64, dw32, f"deconv {shape} weight gradient")
    close(bg.grad, db64, db32, f"deconv {shape} bias gradient")


@pytest.mark.gpu
def test_conv_transpose4s2_skips_the_bias_gradient_in_front_of_batch_statistics():
    x, wt, bias, gy, ref = deconv_reference(DECONV_SHAPES[1])
    xg, wg, bg = nhwc(x).to(DEV).requires_grad_(), wt.to(DEV).requires_grad_(), bias.to(DEV).requires_grad_()
    (audio_ops.conv_transpose4s2_nhwc(xg, wg, bg, bias_grad_is_zero=True) * nhwc(gy).to(DEV)).sum().backward()
    assert bg.grad is not None and bool((bg.grad == 0).all())
    close(wg.grad, ref[torch.float64][2], ref[torch.float32][2], "weight gradient with the bias reduction skipped")


# ---- MaxPool2d(3, (sy, sx)) ------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 28, 12, 128, 1, 2), (2, 26, 5, 512, 2, 2), (3, 3, 3, 4, 1, 1), (1, 28, 12, 512, 2, 2), (1, 26, 5, 128, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool3_forward_is_bit_equal_and_backward_equal_without_ties(shape):
    b, h, w, c, sy, sx = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randperm(b * h * w * c, generator=g).float().reshape(b, c, h, w) / 64.0     # no two values equal: no ties
    xr = x.clone().requires_grad_()
    yr = F.max_pool2d(xr, 3, stride=(sy, sx))
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xg = nhwc(x).to(DEV).requires_grad_()
    y = audio_ops.maxpool3_nhwc(xg, sy, sx)
    (y * nhwc(gy).to(DEV)).sum().backward()
    assert torch.equal(y.detach().cpu(), nhwc(yr.detach()))
    assert torch.equal(xg.grad.cpu(), nhwc(xr.grad))     # a pixel that wins several windows sums them in ATen's order (oy, ox)


@pytest.mark.gpu
def test_maxpool3_first_maximum_wins_a_tie():
    x = torch.zeros(1, 4, 5, 5)                       # every window is one tie: ATen gives the gradient to its first element
    xr = x.clone().requires_grad_()
    F.max_pool2d(xr, 3, stride=(1, 2)).sum().backward()
    xg = nhwc(x).to(DEV).requires_grad_()
    audio_ops.maxpool3_nhwc(xg, 1, 2).sum().backward()
    assert torch.equal(xg.grad.cpu(), nhwc(xr.grad))


# ---- the whole network against training steps of the reference -------------------------------------------------------------------
def make_net(weight_seed):
    m = AudioFeatureNet()
    m.load_state_dict(synthetic_state_dict(None, seed=int(weight_seed), spec=audio_feature_state_dict_spec()), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def module_step(mode):
    """ONE forward + backward of the opted-in network on a fixture's inputs and loss, in ``.train()`` or ``.eval()``."""
    z = np.load(os.path.join(GOLDEN, f"audio_{mode}_backward.npz"))
    fx = {k: z[k] for k in z.files}
    image, audio, pose = synthetic_audio_inputs(int(fx["clips"]), int(fx["steps"]), seed=int(fx["input_seed"]))
    m = make_net(fx["weight_seed"]).requires_grad_(True).train(mode == "train")
    leaves = {"image": image.to(DEV).requires_grad_(), "audio": audio.to(DEV).requires_grad_(), "pose": pose.to(DEV).requires_grad_()}
    deco = m(leaves["image"], leaves["audio"], leaves["pose"], "cnn", float(fx["weight"]))
    with torch.no_grad():
        saved = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(int(fx["loss_seed"]))
    (deco * torch.randn(deco.shape, generator=g).to(DEV)).sum().backward()
    m.check()
    return fx, m, {"deco_out": deco}, leaves, saved


def check_module(fx, got):
    """tests/test_gpu_emotion_backward.py:259-286: per-tensor bar max(4 dist, FP32_MIN_REL scale); at most max(2, n // 200) samples
    beyond it (1 below 400 samples); none beyond 20 bars; a gradient that is zero by construction on the largest tensor's scale."""
    unused = json.loads(str(fx["no_grad"]))
    assert len(unused) == 82 and all(n.startswith("generator.") for n in unused)
    names = [n for n in got if n not in unused]
    assert len(names) == 88 and all("grad/" + n in fx for n in names)
    for n in unused:
        assert got[n] is None, n
    gmax = max(float(fx["gmax/" + n]) for n in names)
    worst = 0.0
    for n in names:
        assert got[n] is not None, n
        want = torch.from_numpy(fx["grad/" + n])
        mine = got[n].detach().cpu().double().reshape(-1)[::int(fx["stride/" + n])]
        assert mine.shape == want.shape and bool(torch.isfinite(mine).all()), n
        scale = float(fx["gmax/" + n])
        if scale < 1e-9 * gmax:      # zero by construction in exact arithmetic: the largest tensor's scale
            scale = gmax
        bar = max(4.0 * float(fx["dist/" + n]) / scale, FP32_MIN_REL) * scale
        diff = (mine - want).abs()
        beyond = int((diff > bar).sum())
        allowed = max(2, diff.numel() // 200) if diff.numel() >= 400 else 1
        worst = max(worst, float(diff.max()) / bar)
        print(f"  {n:44s} err/scale {float(diff.max()) / scale:.2e}  reference fp32 {float(fx['dist/' + n]) / scale:.2e}  beyond the bar {beyond}")
        assert beyond <= allowed, (n, beyond, allowed, float(diff.max()), bar)
        assert float(diff.max()) <= 20 * bar, (n, float(diff.max()), bar)
    print(f"  worst error / bar {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_module_outputs_and_gradients_match_the_reference(mode):
    fx, m, taps, leaves, _ = module_step(mode)
    deco = taps["deco_out"]
    assert deco.requires_grad and tuple(deco.shape) == (int(fx["clips"]), int(fx["steps"]), 35, 64, 64)
    mine = deco.detach().cpu().double().reshape(-1)[::int(fx["ostride/deco_out"])]
    err = float((mine - torch.from_numpy(fx["out/deco_out"])).abs().max())
    tol = max(1e-4, 4.0 * float(fx["floor/deco_out"]))
    print(f"  deco_out: max|hip - reference| {err:.2e}, tolerance {tol:.2e}")
    assert err <= tol, (err, tol)
    got = {n: q.grad for n, q in m.named_parameters()}
    got.update({"input/" + n: t.grad for n, t in leaves.items()})
    check_module(fx, got)


@pytest.mark.gpu
def test_lstm_features_of_the_graph_route_match_the_reference():
    fx, m, _, leaves, saved = module_step("eval")
    out = m.lstm_features(leaves["image"].detach(), leaves["audio"].detach(), leaves["pose"].detach(), float(fx["weight"]))
    assert out.requires_grad                              # opted in, gradients enabled: the graph route
    mine = out.detach().cpu().double().reshape(-1)[::int(fx["ostride/lstm_out"])]
    err = float((mine - torch.from_numpy(fx["out/lstm_out"])).abs().max())
    assert err <= max(1e-4, 4.0 * float(fx["floor/lstm_out"])), err
    with pytest.raises(ValueError, match="state="):
        m.lstm_features(leaves["image"].detach(), leaves["audio"].detach(), leaves["pose"].detach(), float(fx["weight"]), state={})


@pytest.mark.gpu
def test_train_mode_updates_the_running_statistics_per_step_as_the_reference():
    """Statistics batched over T instead of per step would miss both checks: the running values and ``num_batches_tracked`` + T."""
    fx, m, _, _, saved = module_step("train")
    checked = 0
    for key in fx:
        if not key.startswith("buf/"):
            continue
        name = key[4:]
        want = torch.from_numpy(fx[key])
        mine = saved[name].detach().cpu().double().reshape(-1)[::int(fx["bstride/" + name])]
        if name.endswith("num_batches_tracked"):
            assert torch.equal(mine, want), (name, mine, want)
        else:
            e = float((mine - want).abs().max())
            assert e <= 1e-5 * max(1.0, float(want.abs().max())), (name, e)
        checked += 1
    assert checked == 3 * 17      # 8 BatchNorms in the image encoder, 5 in the audio CNN, 4 in decon


@pytest.mark.gpu
def test_train_mode_under_no_grad_is_the_same_composition_without_a_graph():
    fx, m, taps, leaves, _ = module_step("train")
    held = {k: v.detach().clone() for k, v in m.state_dict().items()}
    try:
        with torch.no_grad():
            deco = m(leaves["image"].detach(), leaves["audio"].detach(), leaves["pose"].detach(), "cnn", float(fx["weight"]))
        assert not deco.requires_grad
        err = float((deco - taps["deco_out"].detach()).abs().max())
        assert err <= max(1e-4, 4.0 * float(fx["floor/deco_out"])), err
    finally:
        m.load_state_dict(held)      # (the second call moved the running statistics again)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["audio_small", "audio_batch2"])
def test_eval_graph_route_matches_the_inference_fixtures(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    image, audio, pose = (t.to(DEV) for t in synthetic_audio_inputs(int(z["clips"]), int(z["steps"]), seed=int(z["input_seed"])))
    m = make_net(z["weight_seed"]).eval().requires_grad_(True)
    feats = m.lstm_features(image, audio, pose, float(z["weight"]))
    deco = m(image, audio, pose, "cnn", float(z["weight"]))
    assert feats.requires_grad and deco.requires_grad
    err = float(np.abs(feats.detach().cpu().numpy() - z["lstm_out"]).max())
    assert err <= max(1e-4, 4 * float(z["floor_lstm_out"])), (name, err)          # tests/test_gpu_audio_feature.py's tolerances
    err = float(np.abs(deco.detach()[:, :, ::5, ::7, ::7].cpu().numpy() - z["deco_sample"]).max())
    assert err <= max(1e-4, 4 * float(z["floor_deco_out"])), (name, err)
    # frozen again: the engine, no graph
    m.requires_grad_(False)
    assert not m(image, audio, pose, "cnn", float(z["weight"])).requires_grad


@pytest.mark.gpu
def test_one_train_part1_shaped_step_reaches_every_trained_network():
    """train.py ``train_part1`` (model.py:187-221), smoke only: deco_out[:, i] -> KPDetector_a -> L1 on value and jacobian."""
    n, t = 2, 2
    image, audio, pose = (v.to(DEV) for v in synthetic_audio_inputs(n, t, seed=5))
    m = make_net(2468).requires_grad_(True).train()
    kcfg = tiny_kp_config(audio=True)
    det = KPDetector_a(**kcfg)
    det.load_state_dict(synthetic_state_dict(kcfg, seed=78, spec=kp_state_dict_spec(kcfg)))
    det = det.to(DEV).eval().requires_grad_(True)
    assert det.out_filters == 35
    deco = m(image, audio, pose, "cnn", 1.6)
    g = torch.Generator().manual_seed(6)
    loss = 0.0
    for i in range(t):
        kp = det(deco[:, i].contiguous())
        loss = loss + (kp["value"] - torch.rand(kp["value"].shape, generator=g).to(DEV) * 2 + 1).abs().mean()
        loss = loss + (kp["jacobian"] - torch.randn(kp["jacobian"].shape, generator=g).to(DEV)).abs().mean()
    loss.backward()
    m.check()
    grads = {"lstm.weight_hh_l0": m.lstm.weight_hh_l0.grad, "decon.0.weight": m.decon[0].weight.grad,
             "audio_eocder.0.0.weight": m.audio_eocder[0][0].weight.grad, "down_blocks.0.conv.weight": m.down_blocks[0].conv.weight.grad,
             "pose_encoder.0.weight": m.pose_encoder[0].weight.grad, "kp_detector_a.kp.weight": det.kp.weight.grad}
    for name, gr in grads.items():
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, name
    assert all(q.grad is None for k, q in m.named_parameters() if k.startswith("generator."))
