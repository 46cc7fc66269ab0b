"""``eamm_amd.Adam`` on a GPU, on a real network: KPDetector at ``tiny_kp_config()`` after ``requires_grad_(True)``.  One real forward +
loss + backward gives the gradients; two copies of the parameters are then stepped three times from those recorded gradients (scaled
differently per step), one by ``eamm_amd.Adam`` on the GPU and one by torch's single-tensor Adam on the CPU in float64 and float32
(tests/optim_common.py): every parameter and both moments pass ``closeness.close`` at OP_FLOOR, ``step`` is equal, the detector's
inference engine runs on the updated weights, a ``state_dict`` taken in mid-run continues on ``torch.optim.Adam``, and a
``channels_last`` parameter is updated where it lies."""
import copy

import pytest
import torch

import optim_common as oc
from closeness import close
from eamm_amd import Adam, KPDetector, tiny_kp_config
from eamm_amd.weights import kp_state_dict_spec, synthetic_source, synthetic_state_dict
from oracle import eamm_oracle as orc
from test_gpu_kp_backward import KP_IMAGE_SEED, KP_SEED, TOL_KP, weighted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_SCALE = (1.0, 0.6, -0.8)           # step k runs on the recorded gradient times GRAD_SCALE[k]
LR = {"lr": oc.LR, "betas": oc.BETAS}

_run = {}


def the_run():
    """The detector after three GPU steps, with everything the tests compare, made once:
    names, det, x, sd; grads {name: fp32 CPU}; oracle[dtype] = (params, optimiser) after three CPU steps; mid = the GPU optimiser's
    state_dict and parameters after step 2."""
    if _run:
        return _run
    cfg = tiny_kp_config()
    sd = synthetic_state_dict(cfg, seed=KP_SEED, spec=kp_state_dict_spec(cfg))
    det = KPDetector(**cfg)
    det.load_state_dict(sd)
    det = det.to(DEV)
    det.requires_grad_(True).eval()
    x = synthetic_source(64, seed=KP_IMAGE_SEED, batch=3)
    out = det(x.to(DEV))
    g = torch.Generator().manual_seed(9)
    weighted(out, {k: torch.randn(out[k].shape, generator=g) for k in ("value", "jacobian", "heatmap")}, list(out)).backward()
    names = [n for n, _ in det.named_parameters()]
    grads = {n: p.grad.detach().cpu().clone() for n, p in det.named_parameters()}
    assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and sum(float(v.abs().max()) > 0 for v in grads.values()) > len(names) // 2
    start = {n: p.detach().cpu().clone() for n, p in det.named_parameters()}

    oracle = {}
    for dtype in (torch.float64, torch.float32):
        params = {n: torch.nn.Parameter(start[n].to(dtype).clone()) for n in names}
        opt = torch.optim.Adam(list(params.values()), foreach=False, **LR)
        for scale in GRAD_SCALE:
            for n in names:
                params[n].grad = (grads[n] * scale).to(dtype)
            opt.step()
        oracle[dtype] = (params, opt)

    opt = Adam(det.parameters(), **LR)
    mid = None
    for k, scale in enumerate(GRAD_SCALE):
        for n, p in det.named_parameters():
            p.grad = (grads[n] * scale).to(DEV)
        opt.step()
        if k == 1:
            torch.cuda.synchronize()
            mid = (copy.deepcopy(opt.state_dict()), {n: p.detach().cpu().clone() for n, p in det.named_parameters()})
    torch.cuda.synchronize()
    _run.update(cfg=cfg, sd=sd, det=det, x=x, names=names, grads=grads, start=start, oracle=oracle, opt=opt, mid=mid)
    return _run


def test_three_steps_on_the_key_point_detector_match_the_cpu_oracle():
    r = the_run()
    (p64, o64), (p32, o32) = r["oracle"][torch.float64], r["oracle"][torch.float32]
    for n, p in r["det"].named_parameters():
        state, s64, s32 = r["opt"].state[p], o64.state[p64[n]], o32.state[p32[n]]
        close(p, p64[n], p32[n], f"{n} p")
        close(state["exp_avg"], s64["exp_avg"], s32["exp_avg"], f"{n} exp_avg")
        close(state["exp_avg_sq"], s64["exp_avg_sq"], s32["exp_avg_sq"], f"{n} exp_avg_sq")
        assert state["step"].device.type == "cpu" and state["step"].dtype == torch.float32 and state["step"].dim() == 0
        assert float(state["step"]) == float(s64["step"]) == 3.0
        assert state["exp_avg"].device == p.device and state["exp_avg"].stride() == p.stride()
        assert not torch.equal(p.detach().cpu(), r["start"][n]) or float(r["grads"][n].abs().max()) == 0


def test_the_engine_runs_on_the_updated_weights():
    r = the_run()
    det = r["det"]
    was_training = [p.requires_grad for p in det.parameters()]
    try:
        det.requires_grad_(False).eval()
        with torch.no_grad():
            got = det(r["x"].to(DEV))
        torch.cuda.synchronize()
    finally:
        for p, flag in zip(det.parameters(), was_training):
            p.requires_grad_(flag)
    p64 = r["oracle"][torch.float64][0]
    sd = {k: (p64[k].detach() if k in p64 else v.double() if v.is_floating_point() else v) for k, v in r["sd"].items()}
    want = orc.kp_detector_forward(sd, r["cfg"], r["x"].double())
    old = orc.kp_detector_forward({k: v.double() if v.is_floating_point() else v for k, v in r["sd"].items()}, r["cfg"], r["x"].double())
    for k, tol in TOL_KP.items():
        err = float((got[k].cpu().double() - want[k]).abs().max())
        moved = float((old[k] - want[k]).abs().max())
        print(f"  {k:10s} engine vs oracle on the updated weights {err:.2e} (tol {tol:g}); the three steps moved it by {moved:.2e}")
        assert err <= tol, (k, err)
        assert moved > 4 * tol, (k, "the update is too small for this check to see stale weights", moved)


def test_a_state_dict_from_the_gpu_continues_on_torch_adam_on_the_cpu():
    r = the_run()
    state_dict, params_mid = r["mid"]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        params = {n: torch.nn.Parameter(params_mid[n].to(dtype).clone()) for n in r["names"]}
        opt = torch.optim.Adam(list(params.values()), foreach=False, **LR)
        opt.load_state_dict(copy.deepcopy(state_dict))
        for n in r["names"]:
            st = opt.state[params[n]]
            assert st["exp_avg"].device.type == "cpu" and st["exp_avg"].dtype == dtype and float(st["step"]) == 2.0
            params[n].grad = (r["grads"][n] * GRAD_SCALE[2]).to(dtype)
        opt.step()
        ref[dtype] = (params, opt)
    (p64, o64), (p32, o32) = ref[torch.float64], ref[torch.float32]
    for n, p in r["det"].named_parameters():
        state = r["opt"].state[p]
        close(p, p64[n], p32[n], f"continued {n} p")
        close(state["exp_avg"], o64.state[p64[n]]["exp_avg"], o32.state[p32[n]]["exp_avg"], f"continued {n} exp_avg")
        close(state["exp_avg_sq"], o64.state[p64[n]]["exp_avg_sq"], o32.state[p32[n]]["exp_avg_sq"], f"continued {n} exp_avg_sq")


def test_a_torch_state_dict_loads_onto_the_gpu_and_continues():
    """The other direction, train.py:33: an optimiser state saved by torch.optim.Adam (here after two CPU steps in float32) loads into
    eamm_amd.Adam over GPU parameters, and the third step matches the CPU's third step."""
    r = the_run()
    names, grads = r["names"][:6], r["grads"]
    ref, saved = {}, None
    for dtype in (torch.float32, torch.float64):
        params = {n: torch.nn.Parameter(r["start"][n].to(dtype).clone()) for n in names}
        opt = torch.optim.Adam(list(params.values()), foreach=False, **LR)
        for k, scale in enumerate(GRAD_SCALE):
            for n in names:
                params[n].grad = (grads[n] * scale).to(dtype)
            opt.step()
            if k == 1 and dtype == torch.float32:
                saved = (copy.deepcopy(opt.state_dict()), {n: params[n].detach().clone() for n in names})
        ref[dtype] = (params, opt)
    gpu = {n: torch.nn.Parameter(saved[1][n].to(DEV)) for n in names}
    opt = Adam(list(gpu.values()), **LR)
    opt.load_state_dict(saved[0])
    for n in names:
        assert opt.state[gpu[n]]["exp_avg"].device == gpu[n].device and opt.state[gpu[n]]["step"].device.type == "cpu"
        gpu[n].grad = (grads[n] * GRAD_SCALE[2]).to(DEV)
    opt.step()
    torch.cuda.synchronize()
    (p64, o64), (p32, o32) = ref[torch.float64], ref[torch.float32]
    for n in names:
        close(gpu[n], p64[n], p32[n], f"loaded {n} p")
        close(opt.state[gpu[n]]["exp_avg_sq"], o64.state[p64[n]]["exp_avg_sq"], o32.state[p32[n]]["exp_avg_sq"], f"loaded {n} exp_avg_sq")
        assert float(opt.state[gpu[n]]["step"]) == 3.0


def test_a_channels_last_parameter_is_updated_in_place():
    g = torch.Generator().manual_seed(4)
    host = torch.randn(6, 5, 3, 3, generator=g) * (10 * oc.LR)
    grad = torch.randn(6, 5, 3, 3, generator=g)
    grad.reshape(-1)[oc.DEAD::7] = 0
    p = torch.nn.Parameter(host.to(DEV).contiguous(memory_format=torch.channels_last))
    plain = torch.nn.Parameter(host.to(DEV))
    assert not p.is_contiguous() and p.stride() == (45, 1, 15, 5)
    address, strides, version = p.data_ptr(), p.stride(), p._version
    opt = Adam([p, plain], weight_decay=0.01, **LR)
    want = {}
    for dtype in (torch.float64, torch.float32):
        q = torch.nn.Parameter(host.to(dtype).clone())
        ref = torch.optim.Adam([q], weight_decay=0.01, foreach=False, **LR)
        for _ in range(2):
            q.grad = grad.to(dtype)
            ref.step()
        want[dtype] = (q, ref.state[q])
    for _ in range(2):
        p.grad = grad.to(DEV)                       # contiguous: copied once into the parameter's layout
        plain.grad = grad.to(DEV)
        assert p.grad.is_contiguous() and p.grad.stride() != p.stride()
        opt.step()
    torch.cuda.synchronize()
    assert p.data_ptr() == address and p.stride() == strides and p._version > version
    assert p.grad.is_contiguous() and torch.equal(p.grad.cpu(), grad)             # the caller's gradient is left alone
    st = opt.state[p]
    assert st["exp_avg"].stride() == strides and st["exp_avg_sq"].stride() == strides
    (q64, s64), (q32, s32) = want[torch.float64], want[torch.float32]
    oc.compare((p, st["exp_avg"], st["exp_avg_sq"]), host, (q64, s64["exp_avg"], s64["exp_avg_sq"]), (q32, s32["exp_avg"], s32["exp_avg_sq"]),
               "channels_last")
    # the same values as the contiguous parameter's, element for element
    assert torch.equal(p.detach().cpu(), plain.detach().cpu()) and torch.equal(st["exp_avg"].cpu(), opt.state[plain]["exp_avg"].cpu())


def test_other_dtypes_on_a_gpu_are_refused_by_name():
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        p = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=dtype))
        before = p.detach().clone()
        opt = Adam([p], **LR)
        p.grad = torch.ones_like(p)
        with pytest.raises(ValueError, match=f"eamm_amd.Adam: a parameter of dtype {dtype}"):
            opt.step()
        assert torch.equal(p.detach(), before)


def test_a_parameter_without_a_gradient_keeps_its_step_and_the_stream_is_the_current_one():
    g = torch.Generator().manual_seed(5)
    host = [torch.randn(n, generator=g) * 1e-3 for n in (9, 4100, 5)]
    ps = [torch.nn.Parameter(h.to(DEV)) for h in host]
    qs = [torch.nn.Parameter(h.clone()) for h in host]
    a, b = Adam(ps, **LR), torch.optim.Adam(qs, foreach=False, **LR)
    side = torch.cuda.Stream(DEV)
    for step in range(3):
        grads = [torch.randn(h.shape, generator=g) for h in host]
        with torch.cuda.stream(side):
            for i, (p, q) in enumerate(zip(ps, qs)):
                skip = i == 1 and step == 1
                p.grad, q.grad = (None, None) if skip else (grads[i].to(DEV, non_blocking=False), grads[i])
            a.step()
        b.step()
    side.synchronize()
    for p, q in zip(ps, qs):
        assert float(a.state[p]["step"]) == float(b.state[q]["step"])
        close(p, q.detach().double(), q, "skipped-step run p", oc.OP_FLOOR)
    assert float(a.state[ps[1]]["step"]) == 2.0 and float(a.state[ps[0]]["step"]) == 3.0
