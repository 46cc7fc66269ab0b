"""KPDetector / KPDetector_a as trainable modules: the HIP backward of the heads' reduction (csrc/kp_head.hip,
``eamm_amd.kp_ops.kp_head``) and the detectors' differentiable forward, against the oracle differentiated by autograd in float64
on the CPU (``oracle/eamm_oracle.py``: kp_head, kp_detector_forward, kp_detector_a_forward, generator_forward).

Bars (tests/closeness.py), per tensor, relative to its largest reference entry: max(4 x the oracle's own fp32-vs-fp64
distance for that tensor, a floor).  The floor is TIGHT_MIN_REL where no ReLU lies between the tensor and the loss (the
operator, the heads' parameters, KPDetector_a's feature map) and FP32_MIN_REL behind ReLUs (the hourglass's parameters and the
image: every path from them to the loss crosses the hourglass's ReLUs; in the chain test every detector tensor, since the
generator's ReLUs follow): there an activation within an ulp of zero may take the other branch in a run that rounds differently,
so at most max(2, n // 200) elements (one if n < 400) may lie beyond the bar, none beyond 20 bars.  Without a ReLU: none.

The seeds below were chosen on the CPU so that the oracle's own fp32 run meets these conditions against its float64 run with
room to spare (no tensor's fp32-vs-fp64 distance above a fifth of FP32_MIN_REL: no flipped ReLU in the oracle's own fp32 run).
"""
import pytest
import torch

from closeness import kp_close
from eamm_amd import KPDetector, KPDetector_a, OcclusionAwareGenerator, tiny_config, tiny_kp_config
from eamm_amd.weights import kp_state_dict_spec, synthetic_keypoints, synthetic_source, synthetic_state_dict
from oracle import eamm_oracle as orc

DEV = "cuda:0"
FP32_MIN_REL = 5e-3       # tests/test_train_backward.py
TIGHT_MIN_REL = 2e-5
TOL_KP = {"value": 5e-5, "jacobian": 1e-4, "heatmap": 5e-5}     # tests/test_kp_detector.py
T = 0.1                   # the shipped configurations' temperature


# ---------------------------------------------------------------------------------------------------------------------
close = lambda *a, **k: kp_close(*a, nonfinite="match", **k)      # a window of one pixel has the grid 0 / 0: not finite in the reference and here


def head_expression(logits, K, njm, pad, temperature):
    """``orc.kp_head`` after its two convolutions, applied to NHWC logits [B,h,w,Cs] (any dtype / device): the torch expression the
    operator replaces.  The convolution with padding ``pad`` is the window of the "same"-padded one that starts at 3 - pad."""
    b, h, w, _ = logits.shape
    off = 3 - pad
    win = logits[:, off:h - off, off:w - off]
    hh, ww = win.shape[1:3]
    pred = win[..., :K].permute(0, 3, 1, 2)
    heat = torch.softmax(pred.reshape(b, K, -1) / temperature, dim=2).view(b, K, hh, ww)
    grid = orc.coordinate_grid(hh, ww, logits.dtype, logits.device)
    out = {"value": (heat[..., None] * grid[None, None]).sum(dim=(2, 3)), "heatmap": heat}
    if njm:
        jm = win[..., K:K + 4 * njm].permute(0, 3, 1, 2).reshape(b, njm, 4, hh, ww)
        out["jacobian"] = (heat[:, :, None] * jm).reshape(b, K, 4, -1).sum(dim=-1).view(b, K, 2, 2)
    return out


def weighted(out, weights, keys):
    return sum((out[k] * weights[k].to(out[k].device, out[k].dtype)).sum() for k in keys if k in out)


MAPS = [(9, 14, 0), (16, 16, 0), (7, 7, 0), (11, 8, 3), (10, 13, 1)]
HEADS = [(1, 1), (10, 10), (10, 1), (10, 0), (15, 15), (30, 30)]
SETS = [("value",), ("jacobian",), ("heatmap",), ("value", "jacobian", "heatmap")]


def head_logits(h, w, K, njm, B, seed=11):
    """Key-point logits N(0, 0.05^2): at temperature 0.1 the softmax's exponents have deviation 0.5, so the heat-maps stay far from
    one-hot (a one-hot softmax has no gradient to check); jacobian maps N(0, 1); padded channels carry noise that must be ignored."""
    cs = (K + 4 * njm + 31) // 32 * 32
    g = torch.Generator().manual_seed(seed + 1000 * h + 100 * w + 10 * K + njm + B)
    x = torch.randn(B, h, w, cs, generator=g)
    x[..., :K] *= 0.05
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("K,njm", HEADS)
@pytest.mark.parametrize("h,w,pad", MAPS)
def test_kp_head_forward_and_backward_against_float64_autograd(h, w, pad, K, njm, B):
    from eamm_amd import kp_ops
    logits = head_logits(h, w, K, njm, B)
    cs = logits.shape[3]
    off, oh, ow = 3 - pad, h - 6 + 2 * pad, w - 6 + 2 * pad
    ref = {}
    for dtype in (torch.float64, torch.float32):
        leaf = logits.clone().to(dtype).requires_grad_()       # (a copy: .to() of the same dtype returns the tensor itself)
        ref[dtype] = (leaf, head_expression(leaf, K, njm, pad, T))
    out64 = ref[torch.float64][1]
    if oh * ow > 1:
        assert float(out64["heatmap"].detach().max()) <= 0.5
    g = torch.Generator().manual_seed(5)
    weights = {k: torch.randn(v.shape, generator=g) for k, v in out64.items()}
    x = logits.to(DEV).requires_grad_()
    out = kp_ops.kp_head(x, K, njm, pad, T)
    assert sorted(out) == sorted(out64)
    for k in out:
        close(out[k], out64[k], ref[torch.float32][1][k], f"forward {k}", TIGHT_MIN_REL)
    inside = torch.zeros(h, w, cs, dtype=torch.bool)
    inside[off:h - off, off:w - off, :K + 4 * njm] = True
    for keys in SETS:
        keys = tuple(k for k in keys if k in out64)
        if not keys:
            continue
        want = {}
        for dtype, (leaf, o) in ref.items():
            leaf.grad = None
            weighted(o, weights, keys).backward(retain_graph=True)
            want[dtype] = leaf.grad.clone()
        x.grad = None
        # best effort here (the caching allocator hands the freed block to the next request of its size, the gradient buffer);
        # test_kp_head_backward_writes_the_whole_buffer poisons the buffer it passes itself
        poison = torch.full_like(x, float("nan"))
        del poison
        weighted(out, weights, keys).backward(retain_graph=True)
        got = x.grad.cpu()
        assert bool((got[:, ~inside] == 0).all()), (keys, "gradient outside the window / in the padded channels")
        close(got, want[torch.float64], want[torch.float32], f"grad_logits {'+'.join(keys)}", TIGHT_MIN_REL)
        if oh * ow == 1 and "value" not in keys:     # softmax over one pixel: p = 1, a - sum p a = 0
            assert bool((got[..., :K] == 0).all()), keys


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 9])
def test_kp_head_backward_writes_the_whole_buffer(B):
    """The C entry on a NaN-filled gradient buffer: every element is written, zeros outside the window and in the padded channels."""
    import ctypes as C
    from eamm_amd import _lib
    h, w, K, njm, pad = 10, 13, 10, 10, 1
    x = head_logits(h, w, K, njm, B).to(DEV)
    cs = x.shape[3]
    new = lambda *s: torch.empty(*s, device=DEV)
    value, jac, stats = new(B, K, 2), new(B, K, 2, 2), new(B, K, 2)
    ws = new(_lib.lib().eamm_op_kp_head_workspace_floats(B, K))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().eamm_op_kp_head(0, p(x), B, K, njm, h, w, cs, pad, T, p(value), p(jac), None, p(stats), p(ws), ws.numel(), stream))
    g = torch.Generator().manual_seed(2)
    gv, gj, gh = (torch.randn(s, generator=g).to(DEV) for s in ((B, K, 2), (B, K, 2, 2), (B, K, h - 6 + 2 * pad, w - 6 + 2 * pad)))
    for grads in ((gv, None, None), (None, gj, None), (None, None, gh), (gv, gj, gh)):
        grad = torch.full_like(x, float("nan"))
        _lib.check(_lib.lib().eamm_op_kp_head_backward(0, p(x), p(stats), p(value), p(jac), p(grads[0]), p(grads[1]), p(grads[2]), B, K, njm,
                                                       h, w, cs, pad, T, p(grad), p(ws), ws.numel(), stream))
        grad = grad.cpu()
        assert bool(torch.isfinite(grad).all())
        off = 3 - pad
        inside = torch.zeros(h, w, cs, dtype=torch.bool)
        inside[off:h - off, off:w - off, :K + 4 * njm] = True
        assert bool((grad[:, ~inside] == 0).all()) and bool((grad[:, inside] != 0).any())


def _load(mod, cfg, seed):
    sd = synthetic_state_dict(cfg, seed=seed, spec=kp_state_dict_spec(cfg))
    mod.load_state_dict(sd)
    return mod.to(DEV), sd


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 9])
def test_operator_forward_equals_the_inference_call(B):
    """The operator's forward with ``stats`` is the detectors' inference call (the same launch without ``stats``) on the same logits:
    bit-equal in both kernel forms -- one workgroup per (image, key point) at B = 1, the pixel-sliced form at B = 9 -- and the
    saved (maximum, denominator) reproduce the heat-map."""
    import ctypes as C
    from eamm_amd import _lib
    h, w, K, njm, pad = 16, 16, 10, 10, 0
    x = head_logits(h, w, K, njm, B).to(DEV)
    cs = x.shape[3]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for with_stats in (False, True):
        new = lambda *s: torch.full(s, float("nan"), device=DEV)
        value, jac, heat, stats = new(B, K, 2), new(B, K, 2, 2), new(B, K, h - 6, w - 6), new(B, K, 2)
        ws = torch.empty(_lib.lib().eamm_op_kp_head_workspace_floats(B, K), device=DEV)
        _lib.check(_lib.lib().eamm_op_kp_head(0, p(x), B, K, njm, h, w, cs, pad, T, p(value), p(jac), p(heat), p(stats) if with_stats else None,
                                              p(ws), ws.numel(), stream))
        outs.append((value, jac, heat, stats))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    stats, heat = outs[1][3], outs[1][2]
    win = x[:, 3:h - 3, 3:w - 3, :K].permute(0, 3, 1, 2)
    again = torch.exp(win / T - stats[:, :, 0, None, None]) / stats[:, :, 1, None, None]
    assert float((again - heat).abs().max()) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 9])
def test_differentiable_heads_match_the_engine(B):
    """KPDetector_a on the same feature map: the composition of operators against the frozen detector's engine call."""
    cfg = tiny_kp_config(audio=True)
    det, _ = _load(KPDetector_a(**cfg).eval(), cfg, 77)
    fmap = torch.randn(B, det.out_filters, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    engine = det(fmap)
    assert not any(v.requires_grad for v in engine.values())
    graph = det(fmap.clone().requires_grad_())
    assert sorted(graph) == sorted(engine) and all(v.requires_grad for v in graph.values())
    for k in engine:
        assert float((graph[k].detach() - engine[k]).abs().max()) <= TOL_KP[k], k


# ---------------------------------------------------------------------------------------------------------------------
def _leaves(sd, dtype):
    leaf = lambda k, v: v.is_floating_point() and "running" not in k and k != "down.weight"
    return {k: (v.detach().clone().to(dtype).requires_grad_() if leaf(k, v) else v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _oracle_detector(cfg, sd, x, weights, dtype, audio, train, monkeypatch):
    """(outputs, {name: gradient}, running statistics or None) of the oracle in ``dtype`` on the CPU."""
    sdd = _leaves(sd, dtype)
    xin = x.detach().clone().to(dtype).requires_grad_()
    stats = None
    if train:
        monkeypatch.setattr(orc, "_TRAIN", {"parallel": False, "stats": {}})
    try:
        out = orc.kp_detector_a_forward(sdd, cfg, xin) if audio else orc.kp_detector_forward(sdd, cfg, xin)
        if train:
            stats = dict(orc._TRAIN["stats"])
    finally:
        if train:
            monkeypatch.setattr(orc, "_TRAIN", None)
    weighted(out, weights, list(out)).backward()
    grads = {"param/" + k: v.grad for k, v in sdd.items() if v.requires_grad}
    grads["input"] = xin.grad
    return out, grads, stats


def _compare_detector(det, got_out, got_in_grad, o64, g64, g32, what, all_relu=False):
    gmax = max(float(v.abs().max()) for v in g64.values() if v is not None)
    got = {"param/" + k: p.grad for k, p in det.named_parameters()}
    got["input"] = got_in_grad
    for k, want in g64.items():
        if want is None:          # a tensor the oracle's output does not depend on (KPDetector_a's predictor)
            assert got[k] is None, k
            continue
        assert got[k] is not None, k
        head = k.startswith(("param/kp.", "param/jacobian."))
        behind_relu = all_relu or not (head or (k == "input" and isinstance(det, KPDetector_a)))
        close(got[k], want, g32[k], f"{what} {k}", TIGHT_MIN_REL if head or not behind_relu else FP32_MIN_REL, relu=behind_relu, gmax=gmax)


KP_SEED, KP_IMAGE_SEED = 77, 3


@pytest.mark.gpu
@pytest.mark.parametrize("train", [False, True])
def test_kp_detector_gradients_against_the_oracle(train, monkeypatch):
    cfg = tiny_kp_config()
    det, sd = _load(KPDetector(**cfg), cfg, KP_SEED)
    x = synthetic_source(64, seed=KP_IMAGE_SEED, batch=3)
    if not train:
        with torch.no_grad():
            engine = det.eval()(x.to(DEV))
    det.requires_grad_(True).train(train)
    xg = x.to(DEV).requires_grad_()
    out = det(xg)
    g = torch.Generator().manual_seed(9)
    weights = {k: torch.randn(out[k].shape, generator=g) for k in ("value", "jacobian", "heatmap")}
    weighted(out, weights, list(weights)).backward()
    o64, g64, s64 = _oracle_detector(cfg, sd, x, weights, torch.float64, False, train, monkeypatch)
    _, g32, _ = _oracle_detector(cfg, sd, x, weights, torch.float32, False, train, monkeypatch)
    for k in weights:
        assert float((out[k].detach().cpu() - o64[k].detach().float()).abs().max()) <= TOL_KP[k], k
        if not train:
            assert float((out[k].detach() - engine[k]).abs().max()) <= TOL_KP[k], k
    _compare_detector(det, out, xg.grad, o64, g64, g32, "train" if train else "eval")
    if train:
        now = det.state_dict()
        assert s64
        for prefix, (rm, rv) in s64.items():
            for name, want in ((".running_mean", rm), (".running_var", rv)):
                e = float((now[prefix + name].cpu().double() - want.detach()).abs().max())
                assert e <= 1e-5 * max(1.0, float(want.abs().max())), (prefix + name, e)
        with torch.no_grad():       # .train() under no_grad: the same composition, without a graph
            again = det(x.to(DEV))
        assert not any(v.requires_grad for v in again.values())
        for k in weights:
            assert float((again[k] - out[k].detach()).abs().max()) <= TOL_KP[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "single_jacobian_map", "no_jacobian", "kp5", "kp15"])
def test_kp_detector_a_gradients_against_the_oracle(variant, monkeypatch):
    cfg = tiny_kp_config(audio=True)
    if variant == "single_jacobian_map":
        cfg["single_jacobian_map"] = True
    if variant == "no_jacobian":
        cfg["estimate_jacobian"] = False
    if variant.startswith("kp"):
        cfg["num_kp"] = int(variant[2:])
    det, sd = _load(KPDetector_a(**cfg), cfg, 78)
    det.requires_grad_(True).eval()
    fmap = 0.05 * torch.randn(3, det.out_filters, 16, 16, generator=torch.Generator().manual_seed(4))   # (heat-maps far from one-hot)
    assert tuple(fmap.shape) == (3, 35, 16, 16)
    xg = fmap.to(DEV).requires_grad_()
    out = det(xg)
    assert ("jacobian" in out) == (variant != "no_jacobian")
    g = torch.Generator().manual_seed(9)
    weights = {k: torch.randn(out[k].shape, generator=g) for k in ("value", "jacobian", "heatmap") if k in out}
    weighted(out, weights, list(weights)).backward()
    o64, g64, _ = _oracle_detector(cfg, sd, fmap, weights, torch.float64, True, False, monkeypatch)
    _, g32, _ = _oracle_detector(cfg, sd, fmap, weights, torch.float32, True, False, monkeypatch)
    for k in weights:
        assert float((out[k].detach().cpu() - o64[k].detach().float()).abs().max()) <= TOL_KP[k], k
    assert all(p.grad is None for n, p in det.named_parameters() if n.startswith("predictor."))
    assert all(p.grad is not None for n, p in det.named_parameters() if not n.startswith("predictor."))
    _compare_detector(det, out, xg.grad, o64, g64, g32, variant)
    # detect(heatmap=False) skips the heat-map on this path too
    short = det.detect(xg, heatmap=False)
    assert sorted(short) == sorted(k for k in out if k != "heatmap") and short["value"].requires_grad


# ---------------------------------------------------------------------------------------------------------------------
CHAIN_GEN_SEED, CHAIN_KP_SEED = 77, 77


def _oracle_chain(gcfg, gsd, kcfg, ksd, src, drv, kp_s, weights, dtype):
    ksdd = _leaves(ksd, dtype)
    gsdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in gsd.items()}
    kd = orc.kp_detector_forward(ksdd, kcfg, drv.to(dtype))
    kd = {k: kd[k] for k in ("value", "jacobian")}
    ks = {k: v.to(dtype) for k, v in kp_s.items()}
    out = orc.generator_forward(gsdd, gcfg, src.to(dtype), kd, ks)
    weighted(out, weights, list(weights)).backward()
    return {"param/" + k: v.grad for k, v in ksdd.items() if v.requires_grad}


@pytest.mark.gpu
def test_detector_trains_through_the_generator():
    """detector -> generator -> weighted loss -> backward -> Adam: the fine-tuning step of the reference's GeneratorFullModel."""
    gcfg, kcfg = tiny_config(), tiny_kp_config()
    gsd = synthetic_state_dict(gcfg, seed=CHAIN_GEN_SEED)
    gen = OcclusionAwareGenerator(**gcfg)
    gen.load_state_dict(gsd)
    gen = gen.to(DEV).eval().requires_grad_(False)
    det, ksd = _load(KPDetector(**kcfg), kcfg, CHAIN_KP_SEED)
    det.requires_grad_(True).eval()
    n = 2
    src, drv = synthetic_source(64, seed=1, batch=n), synthetic_source(64, seed=8, batch=n)
    kp_s = synthetic_keypoints(n, 10, seed=4)
    ks = {k: v.to(DEV) for k, v in kp_s.items()}

    def loss_of():
        kp_d = det(drv.to(DEV))
        out = gen(src.to(DEV), kp_driving={k: kp_d[k] for k in ("value", "jacobian")}, kp_source=ks)
        return out

    out = loss_of()
    g = torch.Generator().manual_seed(9)
    weights = {k: torch.randn(out[k].shape, generator=g) for k in ("prediction", "deformed", "occlusion_map")}
    weighted(out, weights, list(weights)).backward()
    g64 = _oracle_chain(gcfg, gsd, kcfg, ksd, src, drv, kp_s, weights, torch.float64)
    g32 = _oracle_chain(gcfg, gsd, kcfg, ksd, src, drv, kp_s, weights, torch.float32)
    gmax = max(float(v.abs().max()) for v in g64.values())
    for name, p in det.named_parameters():
        assert p.grad is not None, name
        head = name.startswith(("kp.", "jacobian."))
        close(p.grad, g64["param/" + name], g32["param/" + name], "chain " + name, TIGHT_MIN_REL if head else FP32_MIN_REL, relu=True,
              gmax=gmax)
    before = {k: v.detach().clone() for k, v in det.named_parameters()}
    first = out["prediction"].detach().clone()
    torch.optim.Adam(det.parameters(), lr=1e-3).step()
    for k, v in det.named_parameters():
        assert not torch.equal(v.detach(), before[k]), k
    second = loss_of()["prediction"].detach()
    assert not torch.equal(first, second)
    # the frozen .eval() call runs the engine on the UPDATED weights (its handle is rebuilt)
    det.requires_grad_(False)
    with torch.no_grad():
        frozen = det(drv.to(DEV))
    assert not any(v.requires_grad for v in frozen.values())
    now = {k: v.detach().cpu() for k, v in det.state_dict().items()}
    want = orc.kp_detector_forward(now, kcfg, drv)
    for k in ("value", "jacobian", "heatmap"):
        assert float((frozen[k].cpu() - want[k]).abs().max()) <= TOL_KP[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("audio", [False, True])
def test_a_fresh_detector_is_frozen_and_runs_the_engine(audio):
    cfg = tiny_kp_config(audio=audio)
    det, _ = _load((KPDetector_a if audio else KPDetector)(**cfg), cfg, 77)
    det.eval()
    assert not any(p.requires_grad for p in det.parameters())
    x = (torch.randn(2, det.out_filters, 16, 16, generator=torch.Generator().manual_seed(0)) if audio else synthetic_source(64, seed=2, batch=2)).to(DEV)
    with_grad_mode = det(x)
    with torch.no_grad():
        without = det(x)
    for k in with_grad_mode:
        assert not with_grad_mode[k].requires_grad and not without[k].requires_grad
        assert torch.equal(with_grad_mode[k], without[k]), k
