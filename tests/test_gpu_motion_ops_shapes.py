"""The differentiable dense-motion operators (eamm_amd/motion_ops.py; csrc/motion.hip, csrc/motion_backward.hip) away from the one
shape of test_gpu_motion_ops.py (16 x 16 = exactly one full workgroup of 256 threads, K = 10, every gradient requested): dead
lanes in the last workgroup, several workgroups per frame, h != w, K = 1 .. 30, every logit layout, null gradient pointers
through the C ABI, the workspace contract, the determinism the kernels' header claims, samples outside the map, anti-alias
shapes whose taps all cross the border, and near-singular key-point jacobians.

Reference: that file's ``_reference_front`` (with its ``_grid``) and its head formulas, evaluated on the CPU in float64.  Bars: per tensor
max(the bar that file uses for the tensor, 4 x floor), floor = the SAME torch reference evaluated in float32 against its float64
evaluation on the same inputs (4 x: the project's margin for another summation / fma order, as tests/test_adversarial.py).
Every comparison prints error / floor.

Cell borders: d(bilinear sample)/d(position) jumps where the pixel coordinate is an integer, and an fp32 kernel may sit on the
other side of the jump than the float64 reference.  For every (frame, motion >= 1, pixel) whose float64 sampling position lies
within 1e-4 of an integer, the upstream gradient of that motion's warped RGB at that pixel is zeroed -- for both sides alike; the
forward comparison (continuous) is untouched.  The masked share is asserted <= 0.5 % per case."""
import functools

import pytest
import torch
import torch.nn.functional as F

from eamm_amd.weights import antialias_kernel, synthetic_keypoints
from test_gpu_motion_ops import _reference_front

gpu = pytest.mark.gpu
DEV = "cuda:0"
VAR = 0.01
SHARE_CAP = 0.005
BAR_CAP = 4e-5

# name: n, K, h, w, jacobians, seed s, hourglass line widths, (ld, ldo): ldo None = no occlusion head, "stacked" = channel K + 1 of ld
CASES = {
    "A": dict(n=2, k=10, h=17, w=15, jac=True, s=5, cpads=(64,), head=(11, 1)),         # 255 px: one dead lane; ld = K + 1 exactly
    "B": dict(n=2, k=5, h=16, w=17, jac=False, s=6, cpads=(64,), head=(32, None)),      # 272 px: 16 live lanes in workgroup 2
    "C": dict(n=1, k=1, h=24, w=20, jac=True, s=7, cpads=(32,), head=(3, "stacked")),   # softmax of two; stacked, ld = K + 2
    "D": dict(n=2, k=15, h=13, w=20, jac=True, s=8, cpads=(64,), head=(32, 32)),        # 260 px: 4 live lanes; Cpad == 4(K+1)
    "E": dict(n=1, k=30, h=24, w=24, jac=True, s=9, cpads=(124, 128), head=(32, 1)),    # K = 30 with and without padding
    "F": dict(n=2, k=10, h=64, w=64, jac=True, s=10, cpads=(64,), head=(32, 32)),       # the generator's grid, 16 workgroups
    "G": dict(n=2, k=10, h=20, w=28, jac=True, s=11, cpads=(64,), head=(32, 1), source_jacobian_gain=3.0),   # ~90 % outside
    "H": dict(n=2, k=10, h=48, w=64, jac=True, s=12, cpads=(64,), head=(32, 32)),       # large and not square
}
FRONT_RUNS = [(name, cpad) for name, c in CASES.items() for cpad in c["cpads"]]

# the bars of test_gpu_motion_ops.py, per tensor
BASE = {"hourglass input": 1e-5, "sparse_deformed": 1e-5, "d small": 2e-5,
        "mask": 2e-6, "deformation": 2e-6, "occlusion": 2e-6, "d mask logits": 1e-5, "d occlusion logits": 1e-5,
        # kp_records' own output has no bar there: it is element-wise 2 x 2 algebra, like the head's outputs (2e-6)
        "records": 2e-6}


def _base(key):
    return 2e-5 if key.startswith("d kp_") else BASE[key]


def _rel(got, want, unit_scale=True):
    """max |got - want| / max(1, max |want|): the scaling of test_gpu_motion_ops._close (unit_scale=False: / max |want|, and the
    absolute error where `want` is all zero)."""
    want = want.detach().double()
    err = float((got.detach().cpu().double() - want).abs().max())
    top = float(want.abs().max())
    return err / (max(1.0, top) if unit_scale else (top if top > 0 else 1.0))


def _bars(floor):
    return {k: max(_base(k), 4 * f) for k, f in floor.items()}


def _compare(tag, got, want, floor, unit_scale=True):
    rows, bad = [], []
    bars = _bars(floor)
    for k, g in got.items():
        assert g.shape == want[k].shape, (tag, k, g.shape, want[k].shape)
        err = _rel(g, want[k], unit_scale)
        ratio = f"{err / floor[k]:.2f}" if floor[k] > 0 else "-"
        rows.append(f"{k} {err:.2e} = {ratio} x floor {floor[k]:.1e}")
        if not err <= bars[k]:
            bad.append((k, err, bars[k]))
    print("\n" + tag + ":  " + ";  ".join(rows))
    assert not bad, (tag, bad)


def _grad(t):
    return torch.zeros_like(t) if t.grad is None else t.grad


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_()      # (a copy: .to() of a float32 tensor to float32 is the tensor itself)


def _leaves(kp, dtype):
    return {a: _leaf(b, dtype) for a, b in kp.items()}


def _kp_grads(out, kdr, ksr):
    for a in kdr:
        out["d kp_driving." + a] = _grad(kdr[a])
        out["d kp_source." + a] = _grad(ksr[a])
    return out


def _want_and_floor(evaluate, unit_scale=True):
    want, single = evaluate(torch.float64), evaluate(torch.float32)
    return want, {k: _rel(single[k], want[k], unit_scale) for k in want}


# ----------------------------------------------------------------------------------------------------------------------------
# inputs and the torch reference (CPU), computed once per case and shared
# ----------------------------------------------------------------------------------------------------------------------------
def _front_eval(inp, g_hg, g_sd, dtype):
    """Forward outputs and every gradient of the loss <hg, g_hg> + <sparse_deformed, g_sd> (a None term is dropped)."""
    kdr, ksr = _leaves(inp["kd"], dtype), _leaves(inp["ks"], dtype)
    sr = _leaf(inp["small"], dtype)
    hg, sd, _ = _reference_front(kdr, ksr, sr, VAR, inp["jac"])
    loss = 0
    if g_hg is not None:
        loss = loss + (hg * g_hg.to(dtype)).sum()
    if g_sd is not None:
        loss = loss + (sd * g_sd.to(dtype)).sum()
    loss.backward()
    return _kp_grads({"hourglass input": hg.detach(), "sparse_deformed": sd.detach(), "d small": _grad(sr)}, kdr, ksr)


def _border_mask(inp):
    """[n,K+1,h,w] bool: motions >= 1 whose float64 sampling position is within 1e-4 of an integer pixel coordinate."""
    h, w = inp["small"].shape[2:]
    with torch.no_grad():
        motions = _reference_front({a: b.double() for a, b in inp["kd"].items()}, {a: b.double() for a, b in inp["ks"].items()},
                                   inp["small"].double(), VAR, inp["jac"])[2]
    ix = ((motions[..., 0] + 1) * w - 1) / 2
    iy = ((motions[..., 1] + 1) * h - 1) / 2
    near = (ix - ix.round()).abs().lt(1e-4) | (iy - iy.round()).abs().lt(1e-4)
    near[:, 0] = False                       # the identity grid depends on nothing
    return near


def _make_inputs(n, k, h, w, jac, s, source_jacobian_gain=None, source_shift=0.0):
    gen = torch.Generator().manual_seed(s)
    small = torch.rand(n, 3, h, w, generator=gen)
    kd, ks = synthetic_keypoints(n, k, seed=s + 2, jacobian=jac), synthetic_keypoints(n, k, seed=s, jacobian=jac)
    if source_jacobian_gain is not None:
        ks["jacobian"] = ks["jacobian"] * source_jacobian_gain
    ks["value"] = ks["value"] + source_shift
    inp = dict(n=n, k=k, h=h, w=w, jac=jac, kd=kd, ks=ks, small=small)
    g_hg = torch.randn(n, k + 1, 4, h, w, generator=gen)
    g_sd = torch.randn(n, k + 1, 3, h, w, generator=gen)
    near = _border_mask(inp)
    keep = (~near)[:, :, None].float()
    g_hg[:, :, 1:4] *= keep
    g_sd *= keep
    inp.update(g_hg=g_hg, g_sd=g_sd, share=float(near[:, 1:].float().mean()))
    return inp


@functools.lru_cache(maxsize=None)
def _case_inputs(name):
    c = CASES[name]
    return _make_inputs(c["n"], c["k"], c["h"], c["w"], c["jac"], c["s"], c.get("source_jacobian_gain"))


@functools.lru_cache(maxsize=None)
def _front_reference(name):
    inp = _case_inputs(name)
    return _want_and_floor(lambda dt: _front_eval(inp, inp["g_hg"], inp["g_sd"], dt))


def _make_head_inputs(inp, ld, ldo, seed):
    n, k, h, w = inp["n"], inp["k"], inp["h"], inp["w"]
    gen = torch.Generator().manual_seed(seed)
    return dict(lm=torch.randn(n, h, w, ld, generator=gen), stacked=ldo == "stacked",
                lo=torch.randn(n, h, w, ldo, generator=gen) if isinstance(ldo, int) else None,
                g_m=torch.randn(n, k + 1, h, w, generator=gen), g_d=torch.randn(n, h, w, 2, generator=gen),
                g_o=torch.randn(n, h, w, generator=gen) if ldo is not None else None)


def _head_eval(inp, hd, g_m, g_d, g_o, dtype):
    """dense_motion.py:98-111 as test_gpu_motion_ops.test_motion_head_against_torch_double states it; a None term is dropped."""
    n, k, h, w = inp["n"], inp["k"], inp["h"], inp["w"]
    kdr, ksr = _leaves(inp["kd"], dtype), _leaves(inp["ks"], dtype)
    lmr = _leaf(hd["lm"], dtype)
    lor = _leaf(hd["lo"], dtype) if hd["lo"] is not None else None
    motions = _reference_front(kdr, ksr, torch.zeros(n, 3, h, w, dtype=dtype), VAR, inp["jac"])[2]
    mask = F.softmax(lmr[..., :k + 1].permute(0, 3, 1, 2), dim=1)
    defo = (motions.permute(0, 1, 4, 2, 3) * mask[:, :, None]).sum(dim=1).permute(0, 2, 3, 1)
    out = {"mask": mask.detach(), "deformation": defo.detach()}
    loss = 0
    if g_m is not None:
        loss = loss + (mask * g_m.to(dtype)).sum()
    if g_d is not None:
        loss = loss + (defo * g_d.to(dtype)).sum()
    has_occ = hd["stacked"] or lor is not None
    if has_occ:
        occ = torch.sigmoid(lmr[..., k + 1] if hd["stacked"] else lor[..., 0])
        out["occlusion"] = occ.detach()
        if g_o is not None:
            loss = loss + (occ * g_o.to(dtype)).sum()
    loss.backward()
    out["d mask logits"] = _grad(lmr)[..., :k + 1]
    if has_occ:
        out["d occlusion logits"] = _grad(lmr)[..., k + 1] if hd["stacked"] else _grad(lor)[..., 0]
    return _kp_grads(out, kdr, ksr)


@functools.lru_cache(maxsize=None)
def _head_case(name):
    inp = _case_inputs(name)
    ld, ldo = CASES[name]["head"]
    hd = _make_head_inputs(inp, ld, ldo, CASES[name]["s"] + 100)
    want, floor = _want_and_floor(lambda dt: _head_eval(inp, hd, hd["g_m"], hd["g_d"], hd["g_o"], dt))
    return hd, want, floor


def test_floors_and_masked_shares_of_the_eight_cases():
    """No GPU: the float32-vs-float64 floors of the torch reference that set the bars of the GPU tests below, and the share of
    samples masked at cell borders.  No bar may exceed 4e-5 (so none can grow unnoticed), no share 0.5 %."""
    for name in CASES:
        inp = _case_inputs(name)
        floors = {"front": _front_reference(name)[1], "head": _head_case(name)[2]}
        print(f"\ncase {name}: masked share {inp['share']:.1e}")
        for part, floor in floors.items():
            print(f"  {part}: " + ";  ".join(f"{k} {v:.1e}" for k, v in floor.items()))
            worst = max(_bars(floor).items(), key=lambda kv: kv[1])
            assert worst[1] <= BAR_CAP, (name, part, worst)
        assert inp["share"] <= SHARE_CAP, (name, inp["share"])


# ----------------------------------------------------------------------------------------------------------------------------
# the HIP operators through eamm_amd.motion_ops
# ----------------------------------------------------------------------------------------------------------------------------
def _to_dev(kp, grad=True):
    return {a: b.to(DEV).requires_grad_(grad) for a, b in kp.items()}


def _small_nhwc(inp):
    return F.pad(inp["small"].permute(0, 2, 3, 1), (0, 1)).contiguous().to(DEV)


def _kp_grads_dev(out, kdd, ksd):
    for a in kdd:
        out["d kp_driving." + a] = kdd[a].grad
        out["d kp_source." + a] = ksd[a].grad
    return out


def _hg_planes(hg, k):
    n, h, w = hg.shape[:3]
    return hg[..., :4 * (k + 1)].reshape(n, h, w, k + 1, 4).permute(0, 3, 4, 1, 2)


def _hip_front(inp, cpad, g_hg, g_sd):
    from eamm_amd import motion_ops
    n, k, h, w = inp["n"], inp["k"], inp["h"], inp["w"]
    kdd, ksd = _to_dev(inp["kd"]), _to_dev(inp["ks"])
    sd_in = _small_nhwc(inp).requires_grad_()
    hg, sdef = motion_ops.motion_front(motion_ops.kp_records(kdd, ksd), sd_in, VAR, cpad)
    assert hg.shape == (n, h, w, cpad) and sdef.shape == (n, k + 1, 3, h, w)
    if cpad > 4 * (k + 1):
        assert float(hg.detach()[..., 4 * (k + 1):].abs().max()) == 0.0
    got_hg = _hg_planes(hg, k)
    ((got_hg * g_hg.to(DEV)).sum() + (sdef * g_sd.to(DEV)).sum()).backward()
    assert float(sd_in.grad[..., 3].abs().max()) == 0.0
    got = {"hourglass input": got_hg, "sparse_deformed": sdef, "d small": sd_in.grad[..., :3].permute(0, 3, 1, 2)}
    return _kp_grads_dev(got, kdd, ksd)


@gpu
@pytest.mark.parametrize("name,cpad", FRONT_RUNS, ids=[f"{a}-{b}" for a, b in FRONT_RUNS])
def test_kp_records_and_motion_front_shapes(name, cpad):
    inp = _case_inputs(name)
    assert inp["share"] <= SHARE_CAP, inp["share"]
    want, floor = _front_reference(name)
    got = _hip_front(inp, cpad, inp["g_hg"], inp["g_sd"])
    _compare(f"front {name} (Cpad {cpad}, masked {inp['share']:.1e})", got, want, floor)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_motion_head_shapes_and_logit_layouts(name):
    from eamm_amd import motion_ops
    inp = _case_inputs(name)
    hd, want, floor = _head_case(name)
    k = inp["k"]
    kdd, ksd = _to_dev(inp["kd"]), _to_dev(inp["ks"])
    lmd = hd["lm"].to(DEV).requires_grad_()
    lod = hd["lo"].to(DEV).requires_grad_() if hd["lo"] is not None else None
    mask, defo, occ = motion_ops.motion_head(lmd, lod, motion_ops.kp_records(kdd, ksd), stacked=hd["stacked"])
    got = {"mask": mask, "deformation": defo}
    loss = (mask * hd["g_m"].to(DEV)).sum() + (defo * hd["g_d"].to(DEV)).sum()
    if hd["g_o"] is not None:
        got["occlusion"] = occ
        loss = loss + (occ * hd["g_o"].to(DEV)).sum()
    else:
        assert occ is None
    loss.backward()
    got["d mask logits"] = lmd.grad[..., :k + 1]
    used = k + 1
    if hd["stacked"]:
        got["d occlusion logits"], used = lmd.grad[..., k + 1], k + 2
    if lmd.shape[3] > used:
        assert float(lmd.grad[..., used:].abs().max()) == 0.0
    if lod is not None:
        got["d occlusion logits"] = lod.grad[..., 0]
        if lod.shape[3] > 1:
            assert float(lod.grad[..., 1:].abs().max()) == 0.0
    _compare(f"head {name} (ld, ldo = {CASES[name]['head']})", _kp_grads_dev(got, kdd, ksd), want, floor)


# ----------------------------------------------------------------------------------------------------------------------------
# the C ABI directly: null gradient pointers (autograd materialises zeros, so motion_ops never passes one) and the workspace
# ----------------------------------------------------------------------------------------------------------------------------
def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _front_backward_raw(rec, small, cpad, g_hg, g_sd, want_small, short=0):
    """eamm_op_motion_front_backward as motion_ops calls it, on NaN-filled outputs and workspace -> (code, d records, d small)."""
    from eamm_amd import _lib
    from eamm_amd._handle import ptr as _ptr, stream_ptr as _stream
    n, k = rec.shape[:2]
    h, w = small.shape[1:3]
    dev = rec.device
    g_rec, g_small = _nan(n, k, 8), (_nan(n, h, w, 4) if want_small else None)
    ws = _nan(_lib.lib().eamm_op_motion_workspace_floats(n, k, h, w))
    with torch.cuda.device(dev):
        code = _lib.lib().eamm_op_motion_front_backward(dev.index, _ptr(rec), _ptr(small), n, k, h, w, VAR, cpad, _ptr(g_hg), _ptr(g_sd),
                                                        _ptr(g_small), _ptr(g_rec), _ptr(ws), ws.numel() - short, _stream(dev))
    torch.cuda.synchronize()
    return code, g_rec, g_small


def _head_backward_raw(mask, occ, rec, g_m, g_d, g_o, ld, ldo, short=0):
    """eamm_op_motion_head_backward likewise -> (code, d mask logits [n,h,w,ld], d occlusion logits [n,h,w,ldo], d records)."""
    from eamm_amd import _lib
    from eamm_amd._handle import ptr as _ptr, stream_ptr as _stream
    n, k1, h, w = mask.shape
    k = k1 - 1
    dev = mask.device
    g_lm, g_lo, g_rec = _nan(n, h, w, ld), _nan(n, h, w, ldo), _nan(n, k, 8)
    ws = _nan(_lib.lib().eamm_op_motion_workspace_floats(n, k, h, w))
    with torch.cuda.device(dev):
        code = _lib.lib().eamm_op_motion_head_backward(dev.index, _ptr(mask), _ptr(occ), _ptr(rec), n, k, h, w, _ptr(g_m), _ptr(g_d),
                                                       _ptr(g_o), _ptr(g_lm), ld, _ptr(g_lo), ldo, _ptr(g_rec), _ptr(ws),
                                                       ws.numel() - short, _stream(dev))
    torch.cuda.synchronize()
    return code, g_lm, g_lo, g_rec


def _hg_line(g_hg, cpad, seed):
    """[n,K+1,4,h,w] -> the hourglass input's NHWC line [n,h,w,Cpad]; the padding channels (outputs that are constant zero) carry
    random upstream gradients, which must reach nothing."""
    n, k1, _, h, w = g_hg.shape
    line = torch.randn(n, h, w, cpad, generator=torch.Generator().manual_seed(seed))
    line[..., :4 * k1] = g_hg.permute(0, 3, 4, 1, 2).reshape(n, h, w, 4 * k1)
    return line.to(DEV)


@gpu
@pytest.mark.parametrize("which", ["only_grad_hourglass_in", "only_grad_sparse_deformed", "grad_small_null"])
def test_front_backward_accepts_null_gradient_pointers(which):
    from eamm_amd import _lib, motion_ops
    inp = _case_inputs("D")
    cpad = 64
    g_hg = None if which == "only_grad_sparse_deformed" else inp["g_hg"]
    g_sd = None if which == "only_grad_hourglass_in" else inp["g_sd"]
    want, floor = _want_and_floor(lambda dt: _front_eval(inp, g_hg, g_sd, dt))
    kdd, ksd = _to_dev(inp["kd"]), _to_dev(inp["ks"])
    rec = motion_ops.kp_records(kdd, ksd)
    want_small = which != "grad_small_null"
    code, g_rec, g_small = _front_backward_raw(rec.detach(), _small_nhwc(inp), cpad, None if g_hg is None else _hg_line(g_hg, cpad, 1),
                                               None if g_sd is None else g_sd.to(DEV), want_small)
    assert code == _lib.EAMM_OK
    assert torch.isfinite(g_rec).all()
    rec.backward(g_rec)
    got = _kp_grads_dev({}, kdd, ksd)
    if want_small:
        assert torch.isfinite(g_small).all() and float(g_small[..., 3].abs().max()) == 0.0
        got["d small"] = g_small[..., :3].permute(0, 3, 1, 2)
    _compare(f"front backward, {which}", got, want, floor)


@gpu
@pytest.mark.parametrize("which", ["only_grad_mask", "only_grad_deformation", "grad_occlusion_null"])
def test_head_backward_accepts_null_gradient_pointers(which):
    from eamm_amd import _lib, motion_ops
    inp = _case_inputs("D")
    hd = _head_case("D")[0]
    ld, ldo = CASES["D"]["head"]
    k = inp["k"]
    g_m = None if which == "only_grad_deformation" else hd["g_m"]
    g_d = None if which == "only_grad_mask" else hd["g_d"]
    want, floor = _want_and_floor(lambda dt: _head_eval(inp, hd, g_m, g_d, None, dt))
    kdd, ksd = _to_dev(inp["kd"]), _to_dev(inp["ks"])
    rec = motion_ops.kp_records(kdd, ksd)
    with torch.no_grad():
        mask, _, occ = motion_ops.motion_head(hd["lm"].to(DEV), hd["lo"].to(DEV), rec.detach())
    dev = lambda t: None if t is None else t.to(DEV)
    code, g_lm, g_lo, g_rec = _head_backward_raw(mask, occ, rec.detach(), dev(g_m), dev(g_d), None, ld, ldo)
    assert code == _lib.EAMM_OK
    assert torch.isfinite(g_lm).all() and torch.isfinite(g_lo).all() and torch.isfinite(g_rec).all()
    assert float(g_lm[..., k + 1:].abs().max()) == 0.0 and float(g_lo[..., 1:].abs().max()) == 0.0
    rec.backward(g_rec)
    got = _kp_grads_dev({"d mask logits": g_lm[..., :k + 1], "d occlusion logits": g_lo[..., 0]}, kdd, ksd)
    _compare(f"head backward, {which}", got, {a: want[a] for a in got}, floor)


@gpu
def test_workspace_contract():
    """eamm_op_motion_workspace_floats = n ceil(hw / 256) K 8, and both backward entries refuse a workspace one float short with the
    argument error before any launch: the NaN-filled outputs stay untouched."""
    from eamm_amd import _lib
    for c in CASES.values():
        n, k, h, w = c["n"], c["k"], c["h"], c["w"]
        assert _lib.lib().eamm_op_motion_workspace_floats(n, k, h, w) == n * ((h * w + 255) // 256) * k * 8, c
    inp = _case_inputs("B")
    n, k, h, w = inp["n"], inp["k"], inp["h"], inp["w"]
    rec = torch.zeros(n, k, 8, device=DEV)
    code, g_rec, g_small = _front_backward_raw(rec, _small_nhwc(inp), 64, _hg_line(inp["g_hg"], 64, 1), inp["g_sd"].to(DEV), True, short=1)
    assert code == _lib.ERR_ARG and torch.isnan(g_rec).all() and torch.isnan(g_small).all()
    mask, occ = torch.full((n, k + 1, h, w), 1.0 / (k + 1), device=DEV), torch.full((n, h, w), 0.5, device=DEV)
    g = torch.ones(n, k + 1, h, w, device=DEV)
    code, g_lm, g_lo, g_rec = _head_backward_raw(mask, occ, rec, g, None, None, 32, 1, short=1)
    assert code == _lib.ERR_ARG and torch.isnan(g_lm).all() and torch.isnan(g_lo).all() and torch.isnan(g_rec).all()


# ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_record_gradients_are_deterministic():
    """motion_backward.hip's header: the per-key-point sums are reduced per workgroup and then in a fixed order over the workgroups,
    so the key-point gradients repeat bit for bit (case F: 16 workgroups per frame); the small image's gradient is accumulated
    with float atomics and only has to stay within its bar."""
    from eamm_amd import motion_ops
    inp = _case_inputs("F")
    hd, head_want, head_floor = _head_case("F")
    want, floor = _front_reference("F")
    kdd, ksd = _to_dev(inp["kd"]), _to_dev(inp["ks"])
    kp_leaves = [kdd["value"], kdd["jacobian"], ksd["value"], ksd["jacobian"]]
    sd_in = _small_nhwc(inp).requires_grad_()
    lmd, lod = hd["lm"].to(DEV).requires_grad_(), hd["lo"].to(DEV).requires_grad_()
    rec = motion_ops.kp_records(kdd, ksd)
    hg, sdef = motion_ops.motion_front(rec, sd_in, VAR, 64)
    front = (_hg_planes(hg, inp["k"]) * inp["g_hg"].to(DEV)).sum() + (sdef * inp["g_sd"].to(DEV)).sum()
    mask, defo, occ = motion_ops.motion_head(lmd, lod, rec)
    head = (mask * hd["g_m"].to(DEV)).sum() + (defo * hd["g_d"].to(DEV)).sum() + (occ * hd["g_o"].to(DEV)).sum()
    names = ["d kp_driving.value", "d kp_driving.jacobian", "d kp_source.value", "d kp_source.jacobian"]
    first = {}
    for run in range(5):
        gf = torch.autograd.grad(front, kp_leaves + [sd_in], retain_graph=True)
        gh = torch.autograd.grad(head, kp_leaves + [lmd, lod], retain_graph=True)
        now = {"front " + a: g for a, g in zip(names, gf)}
        now.update({"head " + a: g for a, g in zip(names, gh)})
        now["head d mask logits"], now["head d occlusion logits"] = gh[4], gh[5]     # no reduction at all: one thread per pixel
        if run == 0:
            first = {a: g.clone() for a, g in now.items()}
            _compare("determinism run 0, front", dict(zip(names, gf[:4])), want, floor)
            _compare("determinism run 0, head", dict(zip(names, gh[:4])), head_want, head_floor)
        for a, g in now.items():
            assert torch.equal(g, first[a]), (run, a)
        _compare(f"determinism run {run}", {"d small": gf[4][..., :3].permute(0, 3, 1, 2)}, want, floor)


@gpu
def test_samples_outside_the_map():
    """Source key points moved by +4: T_k(z) = J_k (z - kd_k) + ks_k lands more than a pixel outside [-1, 1]^2 for every pixel and
    every k >= 1 (grid_sample's zeros padding: the warp AND its position derivative vanish), while the heat-maps of the driving
    key points are as before."""
    c = CASES["D"]
    inp = _make_inputs(c["n"], c["k"], c["h"], c["w"], True, c["s"], source_shift=4.0)
    n, k, h, w = inp["n"], inp["k"], inp["h"], inp["w"]
    with torch.no_grad():
        motions = _reference_front({a: b.double() for a, b in inp["kd"].items()}, {a: b.double() for a, b in inp["ks"].items()},
                                   inp["small"].double(), VAR, True)[2][:, 1:]
    ix, iy = ((motions[..., 0] + 1) * w - 1) / 2, ((motions[..., 1] + 1) * h - 1) / 2
    assert bool(((ix > w) | (ix < -2) | (iy > h) | (iy < -2)).all())                 # both corners of a sample at > w are outside
    want, floor = _want_and_floor(lambda dt: _front_eval(inp, inp["g_hg"], inp["g_sd"], dt))
    got = _hip_front(inp, 64, inp["g_hg"], inp["g_sd"])
    assert float(got["hourglass input"][:, 1:, 1:4].abs().max()) == 0.0 and float(got["sparse_deformed"][:, 1:].abs().max()) == 0.0
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    _compare("outside the map", got, want, floor)
    # upstream gradients on the warps of motions >= 1 only: nothing of the source image was sampled, so nothing flows back to it
    g_hg, g_sd = inp["g_hg"].clone(), inp["g_sd"].clone()
    g_hg[:, 0], g_sd[:, 0] = 0, 0
    g_hg[:, :, 0] = 0
    alone = _hip_front(inp, 64, g_hg, g_sd)
    assert float(alone["d small"].abs().max()) == 0.0
    for a, g in alone.items():
        if a.startswith("d kp_"):
            assert float(g.abs().max()) == 0.0, a


# ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("b,hh,ww,scale", [(3, 32, 48, 0.25), (1, 8, 8, 0.25), (1, 20, 12, 0.25), (2, 12, 20, 1)])
def test_antialias_down_shapes(b, hh, ww, scale):
    """The F.conv2d reference of test_gpu_motion_ops.test_antialias_down_forward_and_backward at sizes that are not square, where
    every 13 x 13 tap window crosses the border (8 x 8), and with less than one block of threads (20 x 12 -> 5 x 3 outputs)."""
    from eamm_amd import motion_ops
    gen = torch.Generator().manual_seed(b * 1000 + hh)
    src = torch.rand(b, 3, hh, ww, generator=gen)
    wgt = antialias_kernel(3)
    xr = src.double().requires_grad_()
    ref = xr if scale == 1 else F.conv2d(F.pad(xr, (6, 6, 6, 6)), wgt.double(), groups=3)[:, :, ::4, ::4]    # util.py:1044-1052
    g = torch.randn(ref.shape, generator=gen)
    (ref * g.double()).sum().backward()
    xd = src.to(DEV).requires_grad_()
    out = motion_ops.antialias_down(xd, wgt.to(DEV) if scale != 1 else None, scale)
    assert out.shape == (b, ref.shape[2], ref.shape[3], 4) and float(out[..., 3].abs().max()) == 0.0
    fwd = _rel(out[..., :3].permute(0, 3, 1, 2), ref)
    (out[..., :3].permute(0, 3, 1, 2) * g.to(DEV)).sum().backward()
    bwd = _rel(xd.grad, xr.grad)
    print(f"\nantialias {b}x{hh}x{ww} scale {scale}: forward {fwd:.1e} backward {bwd:.1e}")
    assert fwd <= 2e-6 and bwd <= 2e-6, (fwd, bwd)


# ----------------------------------------------------------------------------------------------------------------------------
def _records_eval(kd, ks, g_rec, dtype, jac_grads=True):
    kdr, ksr = _leaves(kd, dtype), _leaves(ks, dtype)
    if not jac_grads:
        kdr["jacobian"].requires_grad_(False)
        ksr["jacobian"].requires_grad_(False)
    n, k = kd["value"].shape[:2]
    jac = torch.matmul(ksr["jacobian"], torch.inverse(kdr["jacobian"]))                 # dense_motion.py:55-56
    rec = torch.cat([kdr["value"], ksr["value"], jac.reshape(n, k, 4)], dim=2)
    (rec * g_rec.to(dtype)).sum().backward()
    return _kp_grads({"records": rec.detach()}, kdr, ksr)


def _hip_records(kd, ks, g_rec, jac_grads=True):
    from eamm_amd import motion_ops
    kdd, ksd = _to_dev(kd), _to_dev(ks)
    if not jac_grads:
        kdd["jacobian"].requires_grad_(False)
        ksd["jacobian"].requires_grad_(False)
    rec = motion_ops.kp_records(kdd, ksd)
    (rec * g_rec.to(DEV)).sum().backward()
    return kdd, ksd, _kp_grads_dev({"records": rec.detach()}, kdd, ksd)


@gpu
@pytest.mark.parametrize("which", ["150_records", "determinant_1e-3", "values_only"])
def test_kp_records_blocks_conditioning_and_partial_gradients(which):
    """n = 5, K = 30: 150 records, two 128-thread blocks in the backward.  "determinant_1e-3": one driving jacobian near singular
    (not singular): J = Js inverse(Jd) ~ 1e3 and d Jd ~ 1e6; errors are taken relative to max |want|.  "values_only": the jacobians
    are inputs that need no gradient (null d jacobian pointers)."""
    n, k = 5, 30
    kd, ks = synthetic_keypoints(n, k, seed=13), synthetic_keypoints(n, k, seed=11)
    if which == "determinant_1e-3":
        kd["jacobian"][3, 17] = torch.tensor([[1.3, 0.7], [0.9, (1e-3 + 0.63) / 1.3]])
        assert abs(float(torch.det(kd["jacobian"][3, 17].double())) - 1e-3) < 1e-6
    g_rec = torch.randn(n, k, 8, generator=torch.Generator().manual_seed(3))
    jac_grads = which != "values_only"
    want, floor = _want_and_floor(lambda dt: _records_eval(kd, ks, g_rec, dt, jac_grads), unit_scale=False)
    kdd, ksd, got = _hip_records(kd, ks, g_rec, jac_grads)
    if not jac_grads:
        assert kdd["jacobian"].grad is None and ksd["jacobian"].grad is None
        got = {a: g for a, g in got.items() if g is not None}
        want = {a: want[a] for a in got}
    _compare(f"kp_records, {which}", got, want, floor, unit_scale=False)


@gpu
def test_kp_records_raise_on_a_nan_driving_jacobian():
    from eamm_amd import motion_ops
    kd, ks = synthetic_keypoints(2, 10, seed=2), synthetic_keypoints(2, 10, seed=0)
    kd["jacobian"][1, 3, 0, 1] = float("nan")
    with pytest.raises(RuntimeError, match="singular"):
        motion_ops.kp_records(_to_dev(kd, grad=False), _to_dev(ks, grad=False))
