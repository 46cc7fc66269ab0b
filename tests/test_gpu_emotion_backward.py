"""EmotionDetector as a trainable module: the HIP backward of its ResNet trunk's operators (csrc/conv_s2_backward.hip,
emotion_backward.hip; ``eamm_amd.emo_ops``) against ATen differentiated in float64 on the CPU, and the detector's differentiable
forward against a training step of the reference itself (tests/golden/emotion_tiny128_train_backward.npz,
tools/make_emotion_train_golden.py).

Bars (tests/closeness.py), per tensor, relative to its largest reference entry: max(4 x the reference's own
fp32-vs-fp64 distance for that tensor, a floor).  The floor is closeness.OP_FLOOR for the operators (no element may lie beyond the bar)
and FP32_MIN_REL for the module's gradients, which all sit behind ReLUs: there at most max(2, n // 200) elements (one if n < 400) may
lie beyond the bar, none beyond 20 bars.  A tensor whose reference gradient is below 1e-9 of the largest gradient (a convolution
bias in front of batch statistics) is scaled by that largest one.  The reference's own fp32 run differs from its float64 run by at
most 5.3e-5 relative on any gradient tensor, a hundredth of FP32_MIN_REL.
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
from eamm_amd import EmotionDetector, KPDetector_a, _lib, _op, emo_ops, tiny_kp_config
from eamm_amd._handle import ptr as p, stream_ptr as stream   # (for the calls below that read an entry's return code themselves)
from eamm_amd.weights import (emotion_state_dict_spec, kp_state_dict_spec, synthetic_keypoints, synthetic_source,
                              synthetic_state_dict)

DEV = "cuda:0"
FP32_MIN_REL = 5e-3       # tests/test_train_backward.py
UNUSED = ("fc.", "fc_n.", "final_4.", "final_10.")


# ---- stride-2 convolution ------------------------------------------------------------------------------------------------------
# (B, Hin, Win, Cin, Cout): one output pixel with every border case; h != w; M = 135 = one tile plus a tail across frame
# boundaries; M = 192; deep K on 4 pixels (the forward's split-K path)
CONV_SHAPES = [(1, 2, 2, 32, 32), (2, 6, 10, 64, 128), (9, 10, 6, 32, 32), (3, 16, 16, 64, 128), (1, 4, 4, 256, 512)]


@functools.lru_cache(maxsize=None)
def conv_reference(k, shape):
    """x, weight, dY (NCHW / OIHW, fp32 values) and ATen's y, dX, dW in float64 and float32, on the CPU."""
    b, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(100 * k + sum(shape))
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    gy = torch.randn(b, cout, h // 2, w // 2, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        xl, wl = x.to(dtype).clone().requires_grad_(), wt.to(dtype).clone().requires_grad_()
        y = F.conv2d(xl, wl, stride=2, padding=k // 2)
        (y * gy.to(dtype)).sum().backward()
        ref[dtype] = (y.detach(), xl.grad, wl.grad)
    return x, wt, gy, ref


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CONV_SHAPES)
@pytest.mark.parametrize("k", [1, 3])
def test_conv_s2_forward_and_gradients_against_float64_aten(k, shape):
    x, wt, gy, ref = conv_reference(k, shape)
    (y64, dx64, dw64), (y32, dx32, dw32) = ref[torch.float64], ref[torch.float32]
    xg, wg = nhwc(x).to(DEV).requires_grad_(), wt.to(DEV).requires_grad_()
    y = emo_ops.conv2d_s2_nhwc(xg, wg)
    assert tuple(y.shape) == (shape[0], shape[1] // 2, shape[2] // 2, shape[4])
    (y * nhwc(gy).to(DEV)).sum().backward()
    close(y, nhwc(y64), nhwc(y32), f"k{k} {shape} forward")
    close(xg.grad, nhwc(dx64), nhwc(dx32), f"k{k} {shape} data gradient")
    close(wg.grad, dw64, dw32, f"k{k} {shape} weight gradient")
    if k == 1:
        got = xg.grad.cpu()
        assert bool((got[:, 1::2] == 0).all()) and bool((got[:, :, 1::2] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CONV_SHAPES)
@pytest.mark.parametrize("k", [1, 3])
def test_conv_s2_gradients_write_everything_and_repeat_bit_for_bit(k, shape):
    """The C entries on NaN-poisoned outputs, three times: every element written (a 1x1's odd pixels with exact zeros), the same
    bits every time; a workspace one float short is refused."""
    L = _lib.lib()
    b, h, w, cin, cout = shape
    x, wt, gy, ref = conv_reference(k, shape)
    xd, wd, gd = nhwc(x).to(DEV), wt.to(DEV), nhwc(gy).to(DEV)
    nd, nw = L.eamm_op_conv_s2_dgrad_workspace_floats(b, h, w, cin, cout, k), L.eamm_op_conv_s2_wgrad_workspace_floats(b, h, w, cin, cout, k)
    nf = L.eamm_op_conv_s2_workspace_floats(b, h, w, cin, cout, k)
    assert nd > 0 and nw > 0 and nf > 0
    runs = []
    for _ in range(3):
        dx, dw = torch.full_like(xd, float("nan")), torch.full_like(wd, float("nan"))
        wsd, wsw = torch.full((nd,), float("nan"), device=DEV), torch.full((nw,), float("nan"), device=DEV)
        _op.call("conv_s2_dgrad", gd.device, gd, b, h, w, cin, wd, cout, k, dx, work=wsd)
        _op.call("conv_s2_wgrad", gd.device, xd, gd, b, h, w, cin, cout, k, dw, work=wsw)
        runs.append((dx.cpu(), dw.cpu()))
    dx, dw = runs[0]
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw).all())
    assert all(torch.equal(dx, r[0]) and torch.equal(dw, r[1]) for r in runs[1:])
    close(dx, nhwc(ref[torch.float64][1]), nhwc(ref[torch.float32][1]), f"k{k} {shape} data gradient (C entry)")
    if k == 1:
        assert bool((dx[:, 1::2] == 0).all()) and bool((dx[:, :, 1::2] == 0).all()) and bool((dx[:, ::2, ::2] != 0).any())
    out = torch.empty(b, h // 2, w // 2, cout, device=DEV)
    ws = torch.empty(max(nd, nw, nf), device=DEV)
    assert L.eamm_op_conv_s2_dgrad(0, p(gd), b, h, w, cin, p(wd), cout, k, p(dx.to(DEV)), p(ws), nd - 1, stream()) == _lib.ERR_ARG
    assert L.eamm_op_conv_s2_wgrad(0, p(xd), p(gd), b, h, w, cin, cout, k, p(dw.to(DEV)), p(ws), nw - 1, stream()) == _lib.ERR_ARG
    assert L.eamm_op_conv_s2(0, p(xd), b, h, w, cin, p(wd), cout, k, p(out), p(ws), nf - 1, stream()) == _lib.ERR_ARG


# ---- max-pool ------------------------------------------------------------------------------------------------------------------
def pool_case(shape, plateau):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(7 + sum(shape))
    x = torch.randn(b, c, h, w, generator=g)
    if plateau:      # post-ReLU zeros: whole windows of equal values, and one all-zero plane
        x = torch.relu(x - 0.5)
        x[0, 0] = 0
    gy = torch.randn(b, c, h // 2, w // 2, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        xl = x.to(dtype).clone().requires_grad_()
        y = F.max_pool2d(xl, 3, 2, 1)
        (y * gy.to(dtype)).sum().backward()
        ref[dtype] = (y.detach(), xl.grad)
    return x, gy, ref


@pytest.mark.gpu
@pytest.mark.parametrize("shape,plateau", [((1, 2, 2, 64), False), ((2, 6, 10, 64), False), ((3, 32, 32, 64), False), ((2, 6, 10, 64), True),
                                           ((1, 4, 4, 64), True)])
def test_maxpool_backward_takes_atens_first_maximum(shape, plateau):
    x, gy, ref = pool_case(shape, plateau)
    xg = nhwc(x).to(DEV).requires_grad_()
    y = emo_ops.maxpool3s2_nhwc(xg)
    assert torch.equal(y.detach().cpu(), nhwc(ref[torch.float32][0]))
    (y * nhwc(gy).to(DEV)).sum().backward()
    got, want = xg.grad.cpu(), nhwc(ref[torch.float64][1])
    assert bool(((got != 0) == (want != 0)).all()), "gradient positions differ from ATen's"
    close(got, want, nhwc(ref[torch.float32][1]), f"maxpool {shape} plateau={plateau}")
    # the C entry on a poisoned buffer: every element written
    b, h, w, c = shape
    dx = torch.full_like(xg, float("nan")).detach()
    _op.call("emo_maxpool_backward", dx.device, xg.detach(), nhwc(gy).to(DEV), b, h, w, c, dx)
    assert torch.equal(dx.cpu(), got)


@pytest.mark.gpu
def test_maxpool_all_zero_plane_puts_the_gradient_on_the_first_in_image_tap():
    """A 4x4 plane of zeros: window (oy, ox) covers rows 2 oy - 1 .. 2 oy + 1; its first in-image tap is (max(2 oy - 1, 0), max(2 ox - 1, 0))."""
    x = torch.zeros(1, 4, 4, 64, device=DEV, requires_grad=True)
    emo_ops.maxpool3s2_nhwc(x).sum().backward()
    want = torch.zeros(4, 4)
    for oy in range(2):
        for ox in range(2):
            want[max(2 * oy - 1, 0), max(2 * ox - 1, 0)] += 1
    assert torch.equal(x.grad.cpu()[0, :, :, 5], want)
    xc = torch.zeros(1, 1, 4, 4, requires_grad=True)
    F.max_pool2d(xc, 3, 2, 1).sum().backward()
    assert torch.equal(xc.grad[0, 0], want)


# ---- the `final` stack ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 9])
def test_emo_final_forward_and_gradients(B):
    g = torch.Generator().manual_seed(21 + B)
    a = torch.randn(B, 64, generator=g).abs()            # the input is fc_all's post-ReLU output
    w98 = 0.5 * torch.randn(98, generator=g)
    gv, gj = torch.randn(B, 4, 2, generator=g), torch.randn(B, 4, 2, 2, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        al, wl = a.to(dtype).clone().requires_grad_(), w98.to(dtype).clone().requires_grad_()
        c1w, c1b, c2w, c2b, c3w, c3b = wl[0:8].view(2, 1, 4), wl[8:10], wl[10:42].view(4, 2, 4), wl[42:46], wl[46:94].view(4, 4, 3), wl[94:98]
        y = torch.relu(F.max_pool1d(F.conv1d(al[:, None], c1w, c1b, 2, 1), 2, 2))
        r = F.conv1d(torch.relu(F.conv1d(y, c2w, c2b, 2, 1)), c3w, c3b)
        value, jac = r[:, :, :2], r[:, :, 2:].reshape(B, 4, 2, 2)
        ((value * gv.to(dtype)).sum() + (jac * gj.to(dtype)).sum()).backward()
        ref[dtype] = (value.detach(), jac.detach(), al.grad, wl.grad)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    ag, wg = a.to(DEV).requires_grad_(), w98.to(DEV).requires_grad_()
    value, jac = emo_ops.emo_final(ag, wg)
    ((value * gv.to(DEV)).sum() + (jac * gj.to(DEV)).sum()).backward()
    for name, got, i in (("value", value, 0), ("jacobian", jac, 1), ("grad input", ag.grad, 2), ("grad weights", wg.grad, 3)):
        close(got, r64[i], r32[i], f"emo_final B={B} {name}")
    # a loss on one output only: the other's gradient is absent, not a zero tensor
    ag.grad = wg.grad = None
    v2, _ = emo_ops.emo_final(ag, wg)
    (v2 * gv.to(DEV)).sum().backward()
    assert bool(torch.isfinite(ag.grad).all()) and float(wg.grad[46:].abs().max()) > 0


# ---- the module against the reference's training step -------------------------------------------------------------------------------
def make(cfg, seed, **kw):
    m = EmotionDetector(**cfg, **kw)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed, spec=emotion_state_dict_spec(cfg)), strict=True)
    return m


def load_train_fixture():
    z = np.load(os.path.join(GOLDEN, "emotion_tiny128_train_backward.npz"))
    fx = {k: z[k] for k in z.files}
    cfg = json.loads(str(fx["config"]))
    n, size = int(fx["frames"]), int(fx["size"])
    x = synthetic_source(size, seed=int(fx["image_seed"]), batch=n)
    kp = synthetic_keypoints(n, 10, seed=int(fx["kp_seed"]))
    return fx, cfg, x, kp


@pytest.fixture(scope="module")
def train_step():
    """ONE .train() forward + backward of the differentiable detector on the fixture's inputs and loss."""
    fx, cfg, x, kp = load_train_fixture()
    m = make(cfg, int(fx["weight_seed"])).to(DEV)
    m.requires_grad_(True).train()
    leaves = {"image": x.to(DEV).requires_grad_(), "value": kp["value"].to(DEV).requires_grad_(), "jacobian": kp["jacobian"].to(DEV).requires_grad_()}
    k, fake = m(leaves["image"], leaves["value"], leaves["jacobian"])
    out = {"value": k["value"], "jacobian": k["jacobian"], "fake": fake}
    g = torch.Generator().manual_seed(int(fx["loss_seed"]))
    sum((out[n] * torch.randn(out[n].shape, generator=g).to(DEV)).sum() for n in ("value", "jacobian", "fake")).backward()
    torch.cuda.synchronize()
    return fx, m, out, leaves


@pytest.mark.gpu
def test_train_mode_outputs_match_the_reference(train_step):
    fx, m, out, _ = train_step
    assert all(v.requires_grad for v in out.values())
    for k, v in out.items():
        err = float((v.detach().cpu().double() - torch.from_numpy(fx["out/" + k])).abs().max())
        tol = max(1e-4, 4.0 * float(fx["floor/" + k]))
        print(f"  {k}: max|hip - reference| {err:.2e}, tolerance {tol:.2e}")
        assert err <= tol, (k, err, tol)


@pytest.mark.gpu
def test_train_mode_gradients_match_the_reference(train_step):
    fx, m, _, leaves = train_step
    got = {n: q.grad for n, q in m.named_parameters()}
    got.update({"input/" + n: t.grad for n, t in leaves.items()})
    unused = json.loads(str(fx["no_grad"]))
    assert sorted(n for n in got if n.startswith(UNUSED)) == unused and len(unused) == 14
    names = [n for n in got if n not in unused]
    assert len(names) == 121 and all("grad/" + n in fx for n in names)
    gmax = max(float(fx["gmax/" + n]) for n in names)
    worst = 0.0
    for n in unused:
        assert got[n] is None, n
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
        print(f"  {n:52s} err/scale {float(diff.max()) / scale:.2e}  reference fp32 {float(fx['dist/' + n]) / scale:.2e}  beyond the bar {beyond}")
        assert beyond <= allowed, (n, beyond, allowed, float(diff.max()), bar)
        assert float(diff.max()) <= 20 * bar, (n, float(diff.max()), bar)
    print(f"  worst error / bar {worst:.3f}")


@pytest.mark.gpu
def test_train_mode_updates_the_running_statistics_as_the_reference(train_step):
    fx, m, _, _ = train_step
    now = m.state_dict()
    checked = 0
    for key in fx:
        if not key.startswith("buf/"):
            continue
        name = key[4:]
        want = torch.from_numpy(fx[key])
        mine = now[name].detach().cpu().double().reshape(-1)[::int(fx["bstride/" + name])]
        if name.endswith("num_batches_tracked"):
            assert torch.equal(mine, want), name
        else:
            e = float((mine - want).abs().max())
            assert e <= 1e-5 * max(1.0, float(want.abs().max())), (name, e)
        checked += 1
    assert checked == 3 * 30      # 10 BatchNorms in the hourglass, 20 in the trunk


@pytest.mark.gpu
def test_train_mode_under_no_grad_is_the_same_composition_without_a_graph(train_step):
    fx, m, out, leaves = train_step
    saved = {k: v.detach().clone() for k, v in m.state_dict().items()}
    try:
        with torch.no_grad():
            k, fake = m(leaves["image"].detach(), leaves["value"].detach(), leaves["jacobian"].detach())
        assert not fake.requires_grad and not k["value"].requires_grad
        for name, v in (("value", k["value"]), ("jacobian", k["jacobian"]), ("fake", fake)):
            assert float((v - out[name].detach()).abs().max()) <= max(1e-4, 4.0 * float(fx["floor/" + name])), name
    finally:
        m.load_state_dict(saved)      # (the second call moved the running statistics again)


# ---- .eval(): the graph route against the engine and its fixture ------------------------------------------------------------------
def load_eval_fixture():
    z = np.load(os.path.join(GOLDEN, "emotion_tiny128.npz"))
    fx = {k: z[k] for k in z.files}
    cfg = json.loads(str(fx["config"]))
    n, size = int(fx["frames"]), int(fx["size"])
    x = synthetic_source(size, seed=int(fx["image_seed"]), batch=n)
    kp = synthetic_keypoints(n, 10, seed=int(fx["kp_seed"]))
    return fx, cfg, x.to(DEV), kp["value"].to(DEV), kp["jacobian"].to(DEV)


def eval_tolerance(fx, k):
    return max(1e-4, 4.0 * float(fx["floor_" + k]))      # tests/test_emotion_detector.py:103


@pytest.mark.gpu
def test_eval_graph_route_matches_the_inference_fixture():
    fx, cfg, x, v, j = load_eval_fixture()
    m = make(cfg, int(fx["weight_seed"])).to(DEV).eval().requires_grad_(True)
    kp, fake = m(x, v, j)
    out = {"value": kp["value"], "jacobian": kp["jacobian"], "fake": fake}
    for k, t in out.items():
        assert t.requires_grad, k
        err = float((t.detach().cpu() - torch.from_numpy(fx[k])).abs().max())
        assert err <= eval_tolerance(fx, k), (k, err, eval_tolerance(fx, k))
    # gradients enabled and only an input asking: the graph route too, and the gradient reaches that input
    m.requires_grad_(False)
    vg = v.clone().requires_grad_()
    kp2, fake2 = m(x, vg, j)
    assert kp2["value"].requires_grad
    (kp2["value"].sum() + fake2.sum()).backward()
    assert bool(torch.isfinite(vg.grad).all()) and float(vg.grad.abs().max()) > 0
    assert all(q.grad is None for q in m.parameters())


@pytest.mark.gpu
def test_a_fresh_detector_is_frozen_and_returns_the_engines_bits():
    fx, cfg, x, v, j = load_eval_fixture()
    m = make(cfg, int(fx["weight_seed"])).to(DEV).eval()
    assert not any(q.requires_grad for q in m.parameters())
    kp, fake = m(x, v, j)                         # gradients enabled, nothing asks for one: the engine
    det = m.detect(x, v, j)
    assert not fake.requires_grad and not kp["value"].requires_grad
    assert torch.equal(fake, det["fake"]) and torch.equal(kp["value"], det["value"]) and torch.equal(kp["jacobian"], det["jacobian"])
    with torch.no_grad():
        kp2, fake2 = m(x, v, j)
    assert torch.equal(fake2, fake) and torch.equal(kp2["value"], kp["value"])
    with pytest.raises(RuntimeError, match="inference-only"):
        m.feature(x.clone().requires_grad_())


@pytest.mark.gpu
def test_one_adam_step_then_the_engine_runs_the_updated_weights():
    """Step size.  Adam's first step moves EVERY weight by lr against its gradient's sign, so the outputs move by lr x the sum of
    all |d out / d w|.  Measured with the reference on the CPU (float64 step, then fp32 against float64 on the same weights): at
    lr = 1e-3 the outputs grow from about 1.5 to 107 (value), 738 (jacobian) and 271 (fake), and the reference's own fp32 distance
    to 3.1e-5, 1.6e-4 and 6.8e-5 -- four times that is above this fixture's bar, which is an absolute one for outputs of order 1.
    At lr = 1e-5 the outputs move by about 0.2 and the reference's fp32 distance stays at 1.4e-6, 7.1e-7 and 9.3e-7: the regime
    the bar was stated for.  Hence lr = 1e-5."""
    fx, cfg, x, v, j = load_eval_fixture()
    m = make(cfg, int(fx["weight_seed"])).to(DEV).eval()
    with torch.no_grad():
        before = m.detect(x, v, j)
    m.requires_grad_(True)
    kp, fake = m(x, v, j)
    g = torch.Generator().manual_seed(3)
    sum((t * torch.randn(t.shape, generator=g).to(DEV)).sum() for t in (kp["value"], kp["jacobian"], fake)).backward()
    held = {n: q.detach().clone() for n, q in m.named_parameters()}
    torch.optim.Adam([q for q in m.parameters() if q.grad is not None], lr=1e-5).step()
    for n, q in m.named_parameters():
        assert (q.grad is None) == n.startswith(UNUSED), n
        moved = q.grad is not None and float(q.grad.abs().max()) > 0
        assert torch.equal(q.detach(), held[n]) == (not moved), n
    assert sum(not torch.equal(q.detach(), held[n]) for n, q in m.named_parameters()) >= 100
    kp, fake = m(x, v, j)                         # the graph route on the updated weights, running statistics
    graph = {"value": kp["value"].detach(), "jacobian": kp["jacobian"].detach(), "fake": fake.detach()}
    m.requires_grad_(False)
    with torch.no_grad():
        kp, fake = m(x, v, j)                     # frozen .eval(): the engine, its handle rebuilt for the new weights
    engine = {"value": kp["value"], "jacobian": kp["jacobian"], "fake": fake}
    assert not fake.requires_grad
    for k in engine:
        assert not torch.equal(engine[k], before[k]), k
        err = float((engine[k] - graph[k]).abs().max())
        assert err <= eval_tolerance(fx, k), (k, err)


@pytest.mark.gpu
def test_the_loss_trains_kp_detector_a_through_value_and_jacobian():
    """TrainPart2Model's data flow (reference modules/model.py:312-413), smoke only: KPDetector_a's key points feed the emotion
    detector, an L1 offset loss against a fixed target plus a cross-entropy on ``fake`` reaches both modules."""
    fx, cfg, x, _, _ = load_eval_fixture()
    emo = make(cfg, int(fx["weight_seed"])).to(DEV).eval().requires_grad_(True)
    kcfg = tiny_kp_config(audio=True)
    det = KPDetector_a(**kcfg)
    det.load_state_dict(synthetic_state_dict(kcfg, seed=78, spec=kp_state_dict_spec(kcfg)))
    det = det.to(DEV).eval().requires_grad_(True)
    n = x.shape[0]
    fmap = (0.05 * torch.randn(n, det.out_filters, 16, 16, generator=torch.Generator().manual_seed(4))).to(DEV)
    kp_a = det(fmap)
    off, fake = emo(x, kp_a["value"], kp_a["jacobian"])
    g = torch.Generator().manual_seed(5)
    target_v, target_j = torch.randn(n, 4, 2, generator=g).to(DEV), torch.randn(n, 4, 2, 2, generator=g).to(DEV)
    loss = (off["value"] - target_v).abs().mean() + (off["jacobian"] - target_j).abs().mean() + \
        F.cross_entropy(fake, torch.tensor([1, 4, 7][:n], device=DEV))
    loss.backward()
    for name, mod in (("emotion", emo), ("kp_a", det)):
        grads = {k: q.grad for k, q in mod.named_parameters() if q.grad is not None}
        assert grads, name
        assert all(bool(torch.isfinite(t).all()) for t in grads.values()), name
        assert sum(float(t.abs().max()) > 0 for t in grads.values()) >= len(grads) // 2, name
    assert float(det.kp.weight.grad.abs().max()) > 0 and float(det.jacobian.weight.grad.abs().max()) > 0
    assert float(emo.conv1.weight.grad.abs().max()) > 0 and float(emo.layer2[0].downsample[0].weight.grad.abs().max()) > 0
