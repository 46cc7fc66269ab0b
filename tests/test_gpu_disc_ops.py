"""The discriminator's operator entries (eamm_disc_*) at the smallest shapes that can still go wrong, against F.conv2d /
F.instance_norm / F.leaky_relu / F.avg_pool2d on the CPU in float64, at closeness.close's bar: no element beyond
max(4 |ATen fp32 - fp64|_max, 2e-5 x scale), ATen's distance measured in the same test.

Every case is a function of ``place`` (tests/guarded.py) and is registered there as ``disc-<name>`` under the entries it calls, so
that tests/test_gpu_guarded_ops.py runs the same cases between guard bands; here each runs twice on plain tensors and the two
runs' outputs must be bit-equal (fixed-order sums, no atomics)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from eamm_amd import _lib, _op
from eamm_amd.disc_ops import thin_channels
from closeness import close
from guarded import Plain, case, same_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _call(name, *args, work=None):
    _op.call(name, torch.device(DEV), *args, work=work, family="disc")


def _work(place, name, *dims):
    n = getattr(_lib.lib(), f"eamm_disc_{name}_workspace_floats")(*dims)
    assert n > 0, (name, dims)
    return place(n, "work")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv_inputs(shape, cout, real, seed):
    """x NHWC [B,H,W,C] (channels at and above ``real`` exact zeros), w [cout,real,4,4] He-normal, bias 0.1 randn; fp32."""
    g = torch.Generator().manual_seed(seed)
    b, h, w, c = shape
    x = torch.randn(b, h, w, c, generator=g)
    x[..., real:] = 0
    wt = torch.randn(cout, real, 4, 4, generator=g) * math.sqrt(2.0 / (16 * real))
    bias = 0.1 * torch.randn(cout, generator=g)
    return x, wt, bias


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def conv4_forward_case(shape, cout, place, real=None, rubbish=False, seed=1):
    """pad = 0.  real: the filter's channels of a thin input ([B,H,W,Cp], Cp = shape[3]); rubbish: the filter is handed over with Cp
    channels, non-zero values where the input's padding channels (exact zeros) meet it -- the result is the clean call's."""
    b, h, w, c = shape
    thin = c if real is not None else 0
    real = c if real is None else real
    x, wt, bias = _conv_inputs(shape, cout, real, seed)
    want = [_nhwc(F.conv2d(x[..., :real].permute(0, 3, 1, 2).to(dt), wt.to(dt), bias.to(dt))) for dt in (torch.float64, torch.float32)]
    if rubbish:
        wt = torch.cat([wt, 3.0 + torch.rand(cout, c - real, 4, 4, generator=torch.Generator().manual_seed(seed + 9))], dim=1)
    cw = wt.shape[1]
    out = place((b, h - 3, w - 3, cout), "out", name="out")
    _call("conv4", place(x, "in"), b, h, w, cw, place(wt, "in"), place(bias, "in"), cout, 0, 0, thin, out,
          work=_work(place, "conv4", b, h, w, cw, cout, 0, 0, thin))
    close(out, want[0], want[1], f"conv4 {shape}->{cout} real {real}" + (" rubbish" if rubbish else ""))
    return out


# ---- data gradient ------------------------------------------------------------------------------------------------------------------
def conv4_dgrad_case(dy_shape, cin, place, cp=0, seed=2):
    """pad = 3, transposed filter: dy [B,h,w,Cout] -> dx [B,h+3,w+3,cin] (cp: thin, [.,cp] with zeros at and above cin)."""
    b, h, w, cout = dy_shape
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(b, h, w, cout, generator=g)
    wt = torch.randn(cout, cin, 4, 4, generator=g) * math.sqrt(2.0 / (16 * cout))     # the FORWARD filter
    want = [_nhwc(F.conv_transpose2d(dy.permute(0, 3, 1, 2).to(dt), wt.to(dt))) for dt in (torch.float64, torch.float32)]
    store = cp or cin
    dx = place((b, h + 3, w + 3, store), "out", name="dx")
    _call("conv4", place(dy, "in"), b, h, w, cout, place(wt, "in"), None, cin, 3, 1, cp, dx,
          work=_work(place, "conv4", b, h, w, cout, cin, 3, 1, cp))
    close(dx[..., :cin], want[0], want[1], f"conv4 dgrad {dy_shape}->{cin} thin {cp}")
    if store > cin:
        assert float(dx[..., cin:].abs().max()) == 0.0, "the thin data gradient's padding channels are exact zeros"


# ---- weight and bias gradient -------------------------------------------------------------------------------------------------------
def conv4_wgrad_case(shape, cout, place, real=None, seed=3):
    b, h, w, c = shape
    real = c if real is None else real
    x, wt, bias = _conv_inputs(shape, cout, real, seed)
    dy = torch.randn(b, h - 3, w - 3, cout, generator=torch.Generator().manual_seed(seed + 5))
    want = []
    for dt in (torch.float64, torch.float32):
        w_, b_ = wt.to(dt).requires_grad_(), bias.to(dt).requires_grad_()
        F.conv2d(x[..., :real].permute(0, 3, 1, 2).to(dt), w_, b_).backward(dy.permute(0, 3, 1, 2).to(dt))
        want.append((w_.grad, b_.grad))
    gw, gb = place((cout, c, 4, 4), "out", name="gw"), place((cout,), "out", name="gb")
    _call("conv4_wgrad", place(x, "in"), place(dy, "in"), b, h, w, c, cout, gw, gb, work=_work(place, "conv4_wgrad", b, h, w, c, cout))
    close(gw[:, :real], want[0][0], want[1][0], f"conv4 wgrad {shape}->{cout} real {real}")
    close(gb, want[0][1], want[1][1], f"conv4 bias grad {shape}->{cout}")
    if c > real:
        assert float(gw[:, real:].abs().max()) == 0.0, "zero input channels have a zero weight gradient"


# ---- InstanceNorm + LeakyReLU + AvgPool -----------------------------------------------------------------------------------------------
def _norm_oracle(x, gamma, beta, pool, dout, dt):
    xn = x.permute(0, 3, 1, 2).to(dt).requires_grad_()
    ga = gamma.to(dt).requires_grad_() if gamma is not None else None
    be = beta.to(dt).requires_grad_() if beta is not None else None
    y = F.instance_norm(xn, weight=ga, bias=be, eps=1e-5) if ga is not None else xn
    y = F.leaky_relu(y, 0.2)
    if pool:
        y = F.avg_pool2d(y, 2)
    y.backward(dout.permute(0, 3, 1, 2).to(dt))
    return _nhwc(y.detach()), _nhwc(xn.grad), None if ga is None else ga.grad, None if be is None else be.grad


def norm_case(shape, norm, pool, place, seed=4):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, h, w, c, generator=g) * 1.5 + 0.3
    gamma = 0.5 + torch.rand(c, generator=g) if norm else None
    beta = 0.2 * torch.randn(c, generator=g) if norm else None
    oshape = (b, h // 2, w // 2, c) if pool else shape
    dout = torch.randn(*oshape, generator=g)
    want64, want32 = (_norm_oracle(x, gamma, beta, pool, dout, dt) for dt in (torch.float64, torch.float32))
    xd = place(x, "in")
    gd, bd = (place(gamma, "in"), place(beta, "in")) if norm else (None, None)
    out = place(oshape, "out", name="out")
    stats = place((b, c, 2), "out", dtype=torch.float64, name="stats") if norm else None
    ws = _work(place, "norm_act_pool", b, h, w, c, 1) if norm else None
    _call("norm_act_pool", xd, gd, bd, b, h, w, c, int(norm), int(pool), stats, out, ws, 0 if ws is None else ws.numel())
    what = f"norm_act_pool {shape} norm {int(norm)} pool {int(pool)}"
    close(out, want64[0], want32[0], what)
    dx = place(shape, "out", name="dx")
    gg, gb = (place((c,), "out", name="dgamma"), place((c,), "out", name="dbeta")) if norm else (None, None)
    ws = _work(place, "norm_act_pool_backward", b, h, w, c, 1) if norm else None
    _call("norm_act_pool_backward", xd, stats, gd, bd, place(dout, "in"), b, h, w, c, int(norm), int(pool), dx, gg, gb, ws,
          0 if ws is None else ws.numel())
    close(dx, want64[1], want32[1], what + " dx")
    if norm:
        close(gg, want64[2], want32[2], what + " dgamma")
        close(gb, want64[3], want32[3], what + " dbeta")


CASES = {
    "fwd_mtail": functools.partial(conv4_forward_case, (2, 11, 14, 32), 64),          # 8 x 11 outputs, M = 176: a 48-row tail
    "fwd_one_pixel": functools.partial(conv4_forward_case, (1, 4, 4, 64), 32),
    "fwd_row_past_tile": functools.partial(conv4_forward_case, (1, 8, 16, 32), 32),   # 5 x 13 = 65
    "fwd_two_mtiles_n96": functools.partial(conv4_forward_case, (2, 13, 15, 32), 96),  # M = 240: two M tiles, three 32-column tiles
    "dgrad": functools.partial(conv4_dgrad_case, (1, 7, 9, 64), 32),
    "dgrad_small_map": functools.partial(conv4_dgrad_case, (2, 1, 3, 32), 64),         # grad_out below the filter's size: all padding
    "dgrad_thin4": functools.partial(conv4_dgrad_case, (2, 6, 9, 64), 3, cp=4),
    "dgrad_thin16": functools.partial(conv4_dgrad_case, (2, 6, 9, 32), 13, cp=16),
    "thin4": functools.partial(conv4_forward_case, (2, 9, 12, 4), 64, real=3),
    "thin8": functools.partial(conv4_forward_case, (2, 9, 12, 8), 64, real=6),
    "thin16": functools.partial(conv4_forward_case, (2, 9, 12, 16), 32, real=13),
    "thin4_rubbish": functools.partial(conv4_forward_case, (2, 9, 12, 4), 64, real=3, rubbish=True),
    "thin8_rubbish": functools.partial(conv4_forward_case, (2, 9, 12, 8), 64, real=6, rubbish=True),
    "thin16_rubbish": functools.partial(conv4_forward_case, (2, 9, 12, 16), 32, real=13, rubbish=True),
    "wgrad_ragged_split": functools.partial(conv4_wgrad_case, (2, 11, 14, 32), 64),   # 176 pixels in slices of 96
    "wgrad_one_pixel": functools.partial(conv4_wgrad_case, (1, 4, 4, 64), 32),
    "wgrad_row_past_tile": functools.partial(conv4_wgrad_case, (1, 8, 16, 32), 32),
    "wgrad_thin4": functools.partial(conv4_wgrad_case, (2, 9, 12, 4), 64, real=3),
    "wgrad_thin8": functools.partial(conv4_wgrad_case, (2, 9, 12, 8), 64, real=6),
    "wgrad_thin16": functools.partial(conv4_wgrad_case, (2, 9, 12, 16), 32, real=13),
    "norm_pool_odd": functools.partial(norm_case, (2, 5, 7, 64), True, True),         # -> 2 x 3: odd row and odd column dropped
    "norm_nopool": functools.partial(norm_case, (2, 6, 4, 32), True, False),
    "block0_pool": functools.partial(norm_case, (1, 5, 5, 64), False, True),
    "block0_nopool": functools.partial(norm_case, (1, 5, 5, 64), False, False),
    "norm_two_values": functools.partial(norm_case, (2, 1, 2, 32), True, False),      # H * W = 2
    "norm_many_ranges": functools.partial(norm_case, (1, 19, 21, 8), True, True),     # 399 pixels: seven ranges, 32 row lanes
}

# between guard bands: every case but thin4_rubbish and thin8_rubbish
_CONV = ["fwd_mtail", "fwd_one_pixel", "fwd_row_past_tile", "fwd_two_mtiles_n96", "dgrad", "dgrad_small_map", "dgrad_thin4", "dgrad_thin16", "thin4", "thin8",
         "thin16", "thin16_rubbish"]
_WGRAD = ["wgrad_ragged_split", "wgrad_one_pixel", "wgrad_row_past_tile", "wgrad_thin4", "wgrad_thin8", "wgrad_thin16"]
_NORM = ["norm_pool_odd", "norm_nopool", "block0_pool", "block0_nopool", "norm_two_values", "norm_many_ranges"]
for _names, _entries in ((_CONV, ["eamm_disc_conv4"]), (_WGRAD, ["eamm_disc_conv4_wgrad"]),
                         (_NORM, ["eamm_disc_norm_act_pool", "eamm_disc_norm_act_pool_backward"])):
    for _n in _names:
        case("disc-" + _n, _entries, CASES[_n])


@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_matches_float64_and_repeats_itself(name):
    first, second = Plain(DEV), Plain(DEV)
    CASES[name](place=first)
    CASES[name](place=second)
    torch.cuda.synchronize()
    assert same_outputs(first, second) == [], name


@pytest.mark.parametrize("cp,real,cout", [(4, 3, 64), (8, 6, 64), (16, 13, 32)])
def test_thin_result_does_not_depend_on_the_padding_channels_of_the_filter(cp, real, cout):
    clean = conv4_forward_case((2, 9, 12, cp), cout, Plain(DEV), real=real)
    dirty = conv4_forward_case((2, 9, 12, cp), cout, Plain(DEV), real=real, rubbish=True)
    assert torch.equal(clean, dirty)


def test_thin_channels():
    assert [thin_channels(n) for n in (1, 3, 4, 5, 8, 9, 13, 16, 17, 32, 33)] == [4, 4, 4, 8, 8, 16, 16, 16, 32, 32, 64]


# ---- refusals, by message -----------------------------------------------------------------------------------------------------------
def _refused(match, name, *args, work=None):
    with pytest.raises(_lib.EammError, match=match):
        _call(name, *args, work=work)


def test_refusals_name_the_entry_and_the_reason():
    dev = torch.device(DEV)
    t = lambda *s: torch.zeros(*s, device=dev)
    ws = t(1 << 16)
    x, w, o = t(1, 3, 8, 32), t(32, 32, 4, 4), t(1, 1, 5, 32)
    _refused("eamm_disc_conv4: H and W must be at least 4", "conv4", x, 1, 3, 8, 32, w, None, 32, 0, 0, 0, o, work=ws)
    _refused("eamm_disc_conv4: Cin must be a multiple of 32", "conv4", t(1, 8, 8, 48), 1, 8, 8, 48, t(32, 48, 4, 4), None, 32, 0, 0, 0,
             t(1, 5, 5, 32), work=ws)
    _refused("eamm_disc_conv4: Cout must be a multiple of 32", "conv4", t(1, 8, 8, 32), 1, 8, 8, 32, t(48, 32, 4, 4), None, 48, 0, 0, 0,
             t(1, 5, 5, 48), work=ws)
    _refused("eamm_disc_conv4: pad must be 0", "conv4", t(1, 8, 8, 32), 1, 8, 8, 32, w, None, 32, 1, 0, 0, t(1, 7, 7, 32), work=ws)
    _refused("eamm_disc_conv4: pad = 3 goes with transposed = 1", "conv4", t(1, 8, 8, 32), 1, 8, 8, 32, w, None, 32, 3, 0, 0, t(1, 11, 11, 32),
             work=ws)
    _refused("eamm_disc_conv4: thin must be", "conv4", t(1, 8, 8, 12), 1, 8, 8, 3, t(32, 3, 4, 4), None, 32, 0, 0, 12, t(1, 5, 5, 32), work=ws)
    _refused("eamm_disc_conv4_wgrad: H and W must be at least 4", "conv4_wgrad", x, o, 1, 3, 8, 32, 32, w, None, work=ws)
    _refused("eamm_disc_conv4_wgrad: Cin must be 4, 8, 16", "conv4_wgrad", t(1, 8, 8, 48), t(1, 5, 5, 32), 1, 8, 8, 48, 32, t(32, 48, 4, 4),
             None, work=ws)
    one = t(2, 1, 1, 32)
    _refused("eamm_disc_norm_act_pool: InstanceNorm needs more than one value", "norm_act_pool", one, t(32), t(32), 2, 1, 1, 32, 1, 0,
             t(2, 32, 4), t(2, 1, 1, 32), work=ws)
    _refused("eamm_disc_norm_act_pool_backward: InstanceNorm needs more than one value", "norm_act_pool_backward", one, t(2, 32, 4), t(32),
             t(32), one, 2, 1, 1, 32, 1, 0, t(2, 1, 1, 32), t(32), t(32), work=ws)
    _refused("eamm_disc_norm_act_pool: C must be a multiple of 4", "norm_act_pool", t(1, 4, 4, 6), None, None, 1, 4, 4, 6, 0, 0, None,
             t(1, 4, 4, 6), work=ws)
    _refused("eamm_disc_norm_act_pool: a map below 2 x 2", "norm_act_pool", t(1, 1, 4, 8), None, None, 1, 1, 4, 8, 0, 1, None,
             t(1, 1, 2, 8), work=ws)
    L = _lib.lib()
    assert L.eamm_disc_conv4_workspace_floats(1, 3, 8, 32, 32, 0, 0, 0) == 0 and L.eamm_disc_norm_act_pool_workspace_floats(2, 1, 1, 32, 1) == 0


def test_a_workspace_one_float_short_is_refused():
    dev = torch.device(DEV)
    L = _lib.lib()
    t = lambda *s: torch.zeros(*s, device=dev)
    need = L.eamm_disc_conv4_workspace_floats(1, 8, 8, 32, 32, 0, 0, 0)
    _refused("eamm_disc_conv4: workspace too small", "conv4", t(1, 8, 8, 32), 1, 8, 8, 32, t(32, 32, 4, 4), None, 32, 0, 0, 0, t(1, 5, 5, 32),
             work=t(need)[:need - 1])
    need = L.eamm_disc_conv4_wgrad_workspace_floats(1, 8, 8, 32, 32)
    _refused("eamm_disc_conv4_wgrad: workspace too small", "conv4_wgrad", t(1, 8, 8, 32), t(1, 5, 5, 32), 1, 8, 8, 32, 32, t(32, 32, 4, 4), None,
             work=t(need)[:need - 1])
    need = L.eamm_disc_norm_act_pool_workspace_floats(1, 4, 4, 32, 1)
    _refused("eamm_disc_norm_act_pool: workspace too small", "norm_act_pool", t(1, 4, 4, 32), t(32), t(32), 1, 4, 4, 32, 1, 0, t(1, 32, 4),
             t(1, 4, 4, 32), work=t(need)[:need - 1])
    need = L.eamm_disc_norm_act_pool_backward_workspace_floats(1, 4, 4, 32, 1)
    _refused("eamm_disc_norm_act_pool_backward: workspace too small", "norm_act_pool_backward", t(1, 4, 4, 32), t(1, 32, 4), t(32), t(32),
             t(1, 4, 4, 32), 1, 4, 4, 32, 1, 0, t(1, 4, 4, 32), t(32), t(32), work=t(need)[:need - 1])
