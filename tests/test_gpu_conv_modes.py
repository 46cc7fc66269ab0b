"""The convolutions' engine-only operand modes at operator level: the fused pre-activation of the Winograd input transforms
(eamm_op_wino_transform, eamm_op_conv_ex pre_scale / pre_shift), the implicit GEMM's second output, NCHW store and split hand-over
(eamm_op_conv_ex out2 / scale2 / shift2 / nchw / split_n) in each of its three epilogues, 1x1 filters on 1x1 maps (AT_net2's dense
layers), and the feature warp's second output (eamm_op_warp_ex).  Inputs are seeded on the CPU, every output is pre-filled with NaN
and compared whole against a float64 reference or, where the mode must not change a value, bit for bit against the run without it.

Bounds.  u = 2^-24.
  * input transform: |V - float64| <= 16 u (|B^T| |a| |B|) per element, a = relu(x s + t) in float64.  One rounding for the fmaf, at most
    four dependent rounded operations per 1-D pass, two passes: 9 roundings to first order, under 2x margin on top.
  * second outputs: relu(fmaf(out, s2, t2)) is one rounding of out s2 + t2, so |out2 - float64| <= 2 u (|out s2| + |t2|); with s2 a
    signed power of two out s2 is exact and fl(out s2) + t2 rounded once on the host IS the fmaf: equality.
  * convolutions: tests/test_gpu_ops.py's bounds, 2e-5 (implicit GEMM) and 6e-5 (Winograd) of max(1, max |want|).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from eamm_amd import _lib
from guarded import Plain

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BT2 = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)         # conv_winograd.hip
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=torch.float64)                                                # conv_winograd4.hip


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ptr(t):
    return None if t is None else t.data_ptr()


def affine(C, g, pow2=False, positive=False):
    """Per-channel (scale, shift): about a third of the shifts >= 0.5 (a relu(shift) halo would show), some scales negative, one
    exactly 0; pow2: scales from {+-1/4, +-1/2, +-1, +-2} in a pattern that differs channel to channel (x * scale is then exact)."""
    shift = 0.2 + 0.7 * torch.randn(C, generator=g)
    shift[0], shift[C - 1] = 0.75, -0.5
    if pow2:
        scale = 2.0 ** (torch.randint(0, 4, (C,), generator=g).float() - 2.0) * (1.0 - 2.0 * torch.randint(0, 2, (C,), generator=g).float())
        scale[0], scale[1], scale[2], scale[3] = 0.25, -0.5, 2.0, -1.0
    else:
        scale = 0.3 + 0.8 * torch.randn(C, generator=g)
        scale[1], scale[2] = -0.6, 0.0
    if positive:
        scale = scale.abs().clamp_min(0.125)
    assert pow2 or positive or (bool((scale < 0).any()) and bool((scale == 0).any()))
    return scale.contiguous(), shift.contiguous()


def host_preact(x_nhwc, scale, shift):
    """relu(x * scale + shift) in fp32, multiply and add rounded separately: the kernels' fmaf when x * scale is exact"""
    return torch.relu(x_nhwc * scale + shift)


# ---- a. the input transforms alone -----------------------------------------------------------------------------------------------
T4_SHAPES = [(1, 4, 4, 4), (2, 8, 12, 36), (1, 64, 64, 256), (1, 64, 68, 256), (3, 32, 44, 260)]
T2_SHAPES = [(1, 2, 2, 4), (2, 6, 10, 64), (1, 64, 64, 256)]
TRANSFORM_CASES = [(4,) + s for s in T4_SHAPES] + [(2,) + s for s in T2_SHAPES]


def transform_ref(a64, tile):
    """a64 [B,H,W,C] float64 (activated) -> (V, bound / (16 u)) as [(tile+2)^2, B*H/tile*W/tile, C]"""
    BT = BT4 if tile == 4 else BT2
    P = tile + 2
    B, H, W, C = a64.shape
    pad = F.pad(a64, (0, 0, 1, 1, 1, 1))                                  # one pixel of zeros around H and W
    d = pad.unfold(1, P, tile).unfold(2, P, tile)                         # [B, Hq, Wq, C, P(y), P(x)]

    def tr(m, v):
        return (m @ v @ m.t()).permute(4, 5, 0, 1, 2, 3).reshape(P * P, -1, C)
    return tr(BT, d), tr(BT.abs(), d.abs())


@functools.lru_cache(maxsize=None)
def transform_problem(tile, B, H, W, C, pow2=False, positive=False):
    g = torch.Generator().manual_seed(7000 + 131 * tile + 17 * B + 3 * H + 5 * W + C + 1000 * pow2)
    x = torch.randn(B, H, W, C, generator=g)
    s, t = affine(C, g, pow2, positive)
    return x, s, t


def run_transform(x, s, t, tile, place=None):
    B, H, W, C = x.shape
    P = tile + 2
    place = place or Plain(dev())     # .to(dev()) / torch.full(nan); tests/guarded.py's Arena puts the operands between guard bands
    V = place((P * P, B * (H // tile) * (W // tile), C), "out", name="V")
    xd = place(x, "in", name="x")
    sd, td = (place(s, "in", name="pre_scale"), place(t, "in", name="pre_shift")) if s is not None else (None, None)
    assert sd is None or (sd.numel() == C and td.numel() == C)
    _lib.check(_lib.lib().eamm_op_wino_transform(0, ptr(xd), ptr(sd), ptr(td), B, H, W, C, tile, ptr(V), stream()), None)
    torch.cuda.synchronize()
    return V.cpu()


def check_transform(name, got, a64, tile, keep=None):
    want, mag = transform_ref(a64, tile)
    bound = 16 * U * mag
    err = (got.double() - want).abs()
    if keep is not None:                                                  # a mask over [transform point, tile]
        err, bound, got = err[keep], bound[keep], got[keep]
    assert torch.isfinite(got).all(), (name, "unwritten / non-finite elements")
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    print(f"transform {name}: max err / bound = {ratio:.3f}, max err = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (name, ratio)
    return ratio


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "preact"])
@pytest.mark.parametrize("tile,B,H,W,C", TRANSFORM_CASES)
def test_input_transform_matches_float64(tile, B, H, W, C, pre):
    x, s, t = transform_problem(tile, B, H, W, C)
    got = run_transform(x, s if pre else None, t if pre else None, tile)
    a64 = torch.relu(x.double() * s.double() + t.double()) if pre else x.double()
    check_transform(f"F({tile}x{tile}) {(B, H, W, C)} {'preact' if pre else 'plain'}", got, a64, tile)


@pytest.mark.parametrize("tile,B,H,W,C", [(4, 2, 8, 12, 36), (4, 3, 32, 44, 260), (2, 2, 6, 10, 64)])
def test_fused_preactivation_is_bit_equal_to_the_host_activated_input(tile, B, H, W, C):
    x, s, t = transform_problem(tile, B, H, W, C, pow2=True)
    fused = run_transform(x, s, t, tile)
    apart = run_transform(host_preact(x, s, t), None, None, tile)
    assert torch.isfinite(fused).all()
    assert same_bits(fused, apart)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "preact"])
@pytest.mark.parametrize("tile,B,H,W,C", [(4, 2, 8, 12, 36), (4, 3, 32, 44, 260), (2, 2, 6, 10, 64)])
def test_clamped_loads_are_replaced_not_multiplied(tile, B, H, W, C, pre):
    """x[0, 0, 0, :] = +inf (positive scale there).  The kernels clamp an out-of-range address into the tile's own frame, so the only
    loads that reach the pixel through a clamp are those of frame 0, tile 0, where it is d[1][1] and the halo positions d[0][0],
    d[0][1], d[1][0] read it again: a kernel that multiplied what it read by 0 instead of replacing it would make those NaN.  Row 0 of
    B^T has coefficient 0 at index 1 in both forms (and neither kernel touches d1 when it forms that row), so the entries
    V[0 * P + j] and V[i * P + 0] of tile 0 -- 11 of 36 for F(4x4), 7 of 16 for F(2x2) -- do not depend on d[1][1] but do depend on the
    halo row and column: they must be finite and within their bound, like every entry of every other tile (which also shows that the
    inf reaches no tile whose patch does not hold it).  The other entries of tile 0 carry the inf and are not compared."""
    x, s, t = transform_problem(tile, B, H, W, C, positive=True)
    xi = x.clone()
    xi[0, 0, 0, :] = float("inf")
    got = run_transform(xi, s if pre else None, t if pre else None, tile)
    a64 = torch.relu(x.double() * s.double() + t.double()) if pre else x.double()
    P = tile + 2
    keep = torch.ones(got.shape[:2], dtype=torch.bool)
    keep[:, 0] = False
    keep[:P, 0] = True                                                    # V[0 * P + j]
    keep[::P, 0] = True                                                   # V[i * P + 0]
    assert int(keep[:, 0].sum()) == 2 * P - 1
    assert not torch.isfinite(got[P + 1, 0]).any()                        # the pixel did arrive: V[1 * P + 1] carries it in every channel
    check_transform(f"F({tile}x{tile}) {(B, H, W, C)} inf corner", got, a64, tile, keep)


# ---- the convolution entry -------------------------------------------------------------------------------------------------------
def conv_problem(seed, B, H, W, C0, Cout, ks=3, C1=0, up=0, resid=False):
    """NCHW fp32 (x0, x1 or None, w, b, resid or None)"""
    g = torch.Generator().manual_seed(seed)
    cin = C0 + C1
    x0 = torch.randn(B, C0, H, W, generator=g)
    x1 = torch.randn(B, C1, H, W, generator=g) if C1 else None
    w = torch.randn(Cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    b = 0.1 * torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, H << up, W << up, generator=g) if resid else None
    return x0, x1, w, b, res


def conv_ref(x0, x1, w, b, res, up=0, act=0, pool=0, pre=None):
    """float64, NCHW"""
    x = x0.double() if x1 is None else torch.cat([x0, x1], 1).double()
    if pre is not None:
        x = torch.relu(x * pre[0].double()[None, :, None, None] + pre[1].double()[None, :, None, None])
    if up:
        x = F.interpolate(x, scale_factor=2)
    y = F.conv2d(x, w.double(), b.double(), padding=w.shape[-1] // 2)
    if res is not None:
        y = y + res.double()
    y = F.relu(y) if act == 1 else torch.sigmoid(y) if act == 2 else y
    return F.avg_pool2d(y, 2) if pool else y


def run_conv(x0, x1, w, b, res, *, up=0, act=0, pool=0, splitk=0, tile=0, pre=None, second=None, want_nchw=0, split_n=0, plain_entry=False,
             place=None):
    """One eamm_op_conv_ex call (plain_entry: eamm_op_conv) on NHWC device copies of the NCHW problem -> (out, out2 or None) on the CPU"""
    B, C0, H, W = x0.shape
    Cout, cin, ks, _ = w.shape
    C1 = cin - C0
    place = place or Plain(dev())
    d0, d1 = place(nhwc(x0), "in", name="in0"), (place(nhwc(x1), "in", name="in1") if x1 is not None else None)
    dres = place(nhwc(res), "in", name="resid") if res is not None else None
    Ho, Wo = H << up, W << up
    if split_n:
        out = place((B, Ho, Wo, split_n), "out", name="out")
        out2 = place((B, Ho, Wo, 4), "out", name="out2")
    else:
        out = place((B, Cout, Ho, Wo) if want_nchw else (B, Ho >> pool, Wo >> pool, Cout), "out", name="out")
        out2 = place((B, Ho, Wo, Cout), "out", name="out2") if second is not None else None
    pre_d = [place(v, "in", name=f"pre{i}") for i, v in enumerate(pre)] if pre is not None else [None, None]
    sec_d = [place(v, "in", name=f"second{i}") for i, v in enumerate(second)] if second is not None else [None, None]
    assert all(v is None or v.numel() == C0 for v in pre_d) and all(v is None or v.numel() == Cout for v in sec_d)
    wc, bc = w.contiguous(), b.contiguous()
    head = (0, ptr(d0), C0, ptr(d1), C1, B, H, W, up, ptr(wc), ptr(bc), Cout, ks, ks, act, pool, ptr(dres), splitk, tile, ptr(out), 0, None)
    if plain_entry:
        assert pre is None and second is None and not want_nchw and not split_n
        rc = _lib.lib().eamm_op_conv(*head, stream())
    else:
        rc = _lib.lib().eamm_op_conv_ex(*head, ptr(pre_d[0]), ptr(pre_d[1]), ptr(out2), ptr(sec_d[0]), ptr(sec_d[1]), want_nchw, split_n,
                                        stream())
    _lib.check(rc, None)
    torch.cuda.synchronize()
    return out.cpu(), (out2.cpu() if out2 is not None else None)


def check_conv(name, out_nhwc, want_nchw64, rel):
    assert torch.isfinite(out_nhwc).all(), (name, "unwritten / non-finite elements")
    err = float((nchw(out_nhwc).double() - want_nchw64).abs().max())
    top = max(1.0, float(want_nchw64.abs().max()))
    print(f"conv {name}: max|hip - float64| = {err:.3e}, bound {rel * top:.3e}")
    assert err <= rel * top, (name, err, top)


# ---- b. pre-activation through the whole Winograd convolution
PRE_CASES = {
    "2000_tails_resid": dict(tile=2000, B=1, H=6, W=10, C0=64, Cout=136, resid=True),
    "2100_relu":        dict(tile=2100, B=2, H=16, W=16, C0=128, Cout=128, act=1),
    "2103_split_bf16":  dict(tile=2103, B=2, H=16, W=16, C0=128, Cout=128, act=1),
    "2153_resid":       dict(tile=2153, B=2, H=8, W=12, C0=64, Cout=136, resid=True),
    "2156_pool":        dict(tile=2156, B=1, H=12, W=20, C0=64, Cout=72, act=1, pool=1),
}


@pytest.mark.parametrize("name", list(PRE_CASES))
def test_winograd_preactivation_through_the_convolution(name):
    c = dict(PRE_CASES[name])
    tile, act, pool = c.pop("tile"), c.pop("act", 0), c.pop("pool", 0)
    x0, _, w, b, res = conv_problem(100 + list(PRE_CASES).index(name), **c)
    g = torch.Generator().manual_seed(tile)
    pre = affine(c["C0"], g)
    out, _ = run_conv(x0, None, w, b, res, act=act, pool=pool, tile=tile, pre=pre)
    check_conv(name, out, conv_ref(x0, None, w, b, res, act=act, pool=pool, pre=pre), 6e-5)
    # signed power-of-two scales: the fused form equals the plain entry on the host-activated input, bit for bit
    pre2 = affine(c["C0"], g, pow2=True)
    fused, _ = run_conv(x0, None, w, b, res, act=act, pool=pool, tile=tile, pre=pre2)
    activated = nchw(host_preact(nhwc(x0), *pre2))
    apart, _ = run_conv(activated, None, w, b, res, act=act, pool=pool, tile=tile, plain_entry=True)
    assert torch.isfinite(fused).all()
    assert same_bits(fused, apart)


# ---- c. the second output of the implicit GEMM, in its three epilogues
OUT2_CASES = {
    "tile0_res2":       dict(tile=0, B=1, H=8, W=8, C0=64, Cout=64, resid=True),             # the engine's res2 use
    "tile0_odd_ntail":  dict(tile=0, B=2, H=5, W=7, C0=32, Cout=40),                         # raster order, N tail
    "tile0_splitk3":    dict(tile=0, B=1, H=8, W=8, C0=96, Cout=128, resid=True, splitk=3),  # splitk_reduce_kernel
    "tile0_up":         dict(tile=0, B=1, H=4, W=6, C0=64, Cout=32, up=1),
    "1001_tails_resid": dict(tile=1001, B=1, H=10, W=14, C0=32, Cout=272, resid=True),       # LDS epilogue, M and N tails
    "1004_skinny":      dict(tile=1004, B=1, H=5, W=5, C0=32, Cout=136),
    "1002_scalar":      dict(tile=1002, B=1, H=8, W=8, C0=32, Cout=38),                      # Cout % 4: the big-tile kernel's scalar epilogue
}


def second_bound_ok(out2, out, s2, t2):
    want = torch.relu(out.double() * s2.double() + t2.double())
    bound = 2 * U * ((out.double() * s2.double()).abs() + t2.double().abs())
    err = (out2.double() - want).abs()
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    return bool((err <= bound).all()), ratio


@pytest.mark.parametrize("name", list(OUT2_CASES))
def test_second_output_of_the_implicit_gemm(name):
    c = dict(OUT2_CASES[name])
    tile, splitk, up = c.pop("tile"), c.pop("splitk", 0), c.get("up", 0)
    x0, x1, w, b, res = conv_problem(200 + list(OUT2_CASES).index(name), **c)
    g = torch.Generator().manual_seed(300 + tile)
    alone, _ = run_conv(x0, x1, w, b, res, up=up, splitk=splitk, tile=tile)
    check_conv(name, alone, conv_ref(x0, x1, w, b, res, up=up), 2e-5)
    s2, t2 = affine(c["Cout"], g, pow2=True)
    out, out2 = run_conv(x0, x1, w, b, res, up=up, splitk=splitk, tile=tile, second=(s2, t2))
    assert same_bits(out, alone)
    assert same_bits(out2, torch.relu(out * s2 + t2)) or torch.equal(out2, torch.relu(out * s2 + t2))   # (-0.0 == 0.0)
    s2, t2 = affine(c["Cout"], g)
    out, out2 = run_conv(x0, x1, w, b, res, up=up, splitk=splitk, tile=tile, second=(s2, t2))
    assert same_bits(out, alone) and torch.isfinite(out2).all()
    ok, ratio = second_bound_ok(out2, out, s2, t2)
    print(f"out2 {name}: max err / bound = {ratio:.3f}")
    assert ok, (name, ratio)


# ---- d. NCHW store
NCHW_CASES = {
    "7x7_sigmoid": dict(tile=0, B=2, H=8, W=12, C0=32, Cout=3, ks=7, act=2),                 # the generator's final layer
    "3x3_up":      dict(tile=0, B=1, H=5, W=7, C0=64, Cout=35, up=1),                        # DeconvTail's last layer
    "splitk2":     dict(tile=0, B=1, H=8, W=8, C0=64, Cout=64, splitk=2),
    "1002":        dict(tile=1002, B=1, H=8, W=8, C0=32, Cout=128),
}


@pytest.mark.parametrize("name", list(NCHW_CASES))
def test_nchw_store_is_the_nhwc_output_permuted(name):
    c = dict(NCHW_CASES[name])
    tile, splitk, act, up = c.pop("tile"), c.pop("splitk", 0), c.pop("act", 0), c.get("up", 0)
    x0, x1, w, b, res = conv_problem(400 + list(NCHW_CASES).index(name), **c)
    rows, _ = run_conv(x0, x1, w, b, res, up=up, act=act, splitk=splitk, tile=tile)
    check_conv(name, rows, conv_ref(x0, x1, w, b, res, up=up, act=act), 2e-5)
    planes, _ = run_conv(x0, x1, w, b, res, up=up, act=act, splitk=splitk, tile=tile, want_nchw=1)
    assert same_bits(planes, nchw(rows))


# ---- e. split hand-over (DeconvTail -> KPDetector_a)
@pytest.mark.parametrize("name,tile,Cout", [("tile0_scalar", 0, 36), ("1003_float4", 1003, 36), ("tile0_35_of_36", 0, 35)])
def test_split_hand_over(name, tile, Cout):
    split_n = 32
    x0, x1, w, b, res = conv_problem(500 + Cout + tile, B=2, H=4, W=6, C0=64, Cout=Cout, up=1)
    rows, _ = run_conv(x0, x1, w, b, res, up=1, tile=tile)
    check_conv(name, rows, conv_ref(x0, x1, w, b, res, up=1), 2e-5)
    wide, thin = run_conv(x0, x1, w, b, res, up=1, tile=tile, split_n=split_n)
    assert same_bits(wide, rows[..., :split_n])
    assert same_bits(thin[..., :Cout - split_n], rows[..., split_n:])
    # the floats of a thin pixel past Cout - split_n keep their sentinel: DeconvTail carries a zero 36th column because of this
    assert bool(torch.isnan(thin[..., Cout - split_n:]).all())


# ---- f. 1x1 filters: AT_net2's dense layers as implicit GEMMs on 1x1 maps
DENSE_CASES = {
    "one_row":      dict(B=1, H=1, W=1, C0=64, Cout=32),
    "fc2_like":     dict(B=8, H=1, W=1, C0=512, Cout=256, act=1, splitk=4),
    "xp0_two_in":   dict(B=5, H=1, W=1, C0=96, C1=32, Cout=40),                              # two concatenated inputs
    "pointwise":    dict(B=2, H=6, W=10, C0=32, Cout=64),
    "fc1_like":     dict(B=8, H=1, W=1, C0=12288, Cout=64, act=1, splitk=4),                 # the fixed split-K of 4
}


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_one_by_one_filters(name):
    c = dict(DENSE_CASES[name])
    act, splitk = c.pop("act", 0), c.pop("splitk", 0)
    x0, x1, w, b, res = conv_problem(600 + list(DENSE_CASES).index(name), ks=1, **c)
    out, _ = run_conv(x0, x1, w, b, res, act=act, splitk=splitk, tile=0)
    check_conv(name, out, conv_ref(x0, x1, w, b, res, act=act), 2e-5)


# ---- g. the feature warp's second output
WARP_CASES = {
    "one_source":   dict(n=3, ns=1, hf=16, wf=16, C=64, h=16, w=16),
    "resized_flow": dict(n=2, ns=1, hf=32, wf=32, C=64, h=16, w=16, seed=3),
    "C8":           dict(n=2, ns=2, hf=6, wf=10, C=8, h=6, w=10, seed=4),                    # half_n = 1
    "C24":          dict(n=2, ns=1, hf=5, wf=7, C=24, h=5, w=7, seed=5),                     # half_n = 3
}


def run_warp(feat, defo, om, n, ns, hf, wf, C, h, w, second=None, plain_entry=False, place=None):
    place = place or Plain(dev())
    f_d, d_d = place(nhwc(feat), "in", name="features"), place(defo.contiguous(), "in", name="deformation")
    o_d = place(om[:, 0].contiguous(), "in", name="occlusion")
    out = place((n, hf, wf, C), "out", name="out")
    head = (0, ptr(f_d), ptr(d_d), ptr(o_d), n, ns, hf, wf, C, h, w, ptr(out), 0, None)
    if plain_entry:
        _lib.check(_lib.lib().eamm_op_warp(*head, stream()), None)
        torch.cuda.synchronize()
        return out.cpu(), None
    out2 = place((n, hf, wf, C), "out", name="out2")
    s2, t2 = (place(v, "in", name=f"second{i}") for i, v in enumerate(second))
    assert s2.numel() == C and t2.numel() == C
    _lib.check(_lib.lib().eamm_op_warp_ex(*head, ptr(out2), ptr(s2), ptr(t2), stream()), None)
    torch.cuda.synchronize()
    return out.cpu(), out2.cpu()


@pytest.mark.parametrize("name", list(WARP_CASES))
def test_second_output_of_the_feature_warp(name):
    k = dict(WARP_CASES[name])
    n, ns, hf, wf, C, h, w = (k[q] for q in ("n", "ns", "hf", "wf", "C", "h", "w"))
    g = torch.Generator().manual_seed(k.get("seed", 0))
    feat = torch.randn(ns, C, hf, wf, generator=g)
    ident = torch.stack(torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")[::-1], -1)
    defo = ident[None] + 0.3 * torch.randn(n, h, w, 2, generator=g)          # some samples fall outside the map
    om = torch.rand(n, 1, h, w, generator=g)
    d, o = defo, om
    if (h, w) != (hf, wf):    # generator.py:52-56, 82-83
        d = F.interpolate(defo.permute(0, 3, 1, 2), size=(hf, wf), mode="bilinear").permute(0, 2, 3, 1)
        o = F.interpolate(om, size=(hf, wf), mode="bilinear")
    want = F.grid_sample(feat if ns == n else feat.expand(n, -1, -1, -1), d, mode="bilinear", padding_mode="zeros", align_corners=False) * o
    args = (feat, defo, om, n, ns, hf, wf, C, h, w)
    alone, _ = run_warp(*args, plain_entry=True)
    assert torch.isfinite(alone).all()
    assert float((nchw(alone) - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))    # tests/test_gpu_ops.py's bound
    s2, t2 = affine(C, g, pow2=True)
    out, out2 = run_warp(*args, second=(s2, t2))
    assert same_bits(out, alone)
    assert same_bits(out2, torch.relu(out * s2 + t2)) or torch.equal(out2, torch.relu(out * s2 + t2))
    s2, t2 = affine(C, g)
    out, out2 = run_warp(*args, second=(s2, t2))
    assert same_bits(out, alone) and torch.isfinite(out2).all()
    ok, ratio = second_bound_ok(out2, out, s2, t2)
    print(f"warp out2 {name}: max err / bound = {ratio:.3f}")
    assert ok, (name, ratio)


# ---- h. refusals on the device path
def test_pool_with_a_residual_is_refused():
    """The pooled epilogue adds no residual: such a call used to return the convolution without it.  (The entries refuse it before any
    device work; conv_launch's own check behind them is defence in depth that no entry reaches.)"""
    x0, x1, w, b, res = conv_problem(900, B=1, H=8, W=8, C0=32, Cout=32, resid=True)
    for tile in (0, 1002):
        for plain in (True, False):
            with pytest.raises(_lib.EammError) as exc:
                run_conv(x0, x1, w, b, res, act=1, pool=1, tile=tile, plain_entry=plain)
            assert exc.value.code == _lib.ERR_ARG
