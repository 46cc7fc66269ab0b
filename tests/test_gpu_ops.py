"""Op-level parity on the GPU: the fp32-MFMA implicit-GEMM convolution (every loader / epilogue /
split-K variant) through the C ABI entry point eamm_op_conv, against torch-CPU fp32 reference ops."""
import pytest
import torch
import torch.nn.functional as F

from eamm_amd import _lib
from guarded import Plain

pytestmark = pytest.mark.gpu


def ref_conv(in0, in1, w, b, ks, kw, up, act, pool, resid):
    x = in0 if in1 is None else torch.cat([in0, in1], dim=1)
    if up:
        x = F.interpolate(x, scale_factor=2)  # nearest, as UpBlock2d (util.py:896)
    y = F.conv2d(x, w, b, padding=(ks // 2, kw // 2))
    if resid is not None:
        y = y + resid
    if act == 1:
        y = F.relu(y)
    elif act == 2:
        y = torch.sigmoid(y)
    if pool:
        y = F.avg_pool2d(y, 2)
    return y


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def run_case(B, H, W, C0, C1, Cout, ks, kw=0, up=0, act=0, pool=0, resid=False, splitk=0, tile_n=0, seed=0, zero_bias=False, place=None):
    kw = kw or ks
    g = torch.Generator().manual_seed(seed)
    cin = C0 + C1
    in0 = torch.randn(B, C0, H, W, generator=g)
    in1 = torch.randn(B, C1, H, W, generator=g) if C1 else None
    w = torch.randn(Cout, cin, ks, kw, generator=g) * (2.0 / (cin * ks * kw)) ** 0.5
    b = 0.1 * torch.randn(Cout, generator=g)
    if zero_bias:   # the column-patch kernel leaves the bias to the gather kernel that follows it
        b = torch.zeros(Cout)
    Ho, Wo = (H << up), (W << up)
    res = torch.randn(B, Cout, Ho, Wo, generator=g) if resid else None
    want = ref_conv(in0, in1, w, b, ks, kw, up, act, pool, res)
    dev = torch.device("cuda:0")
    place = place or Plain(dev)     # .to(dev) / torch.full(nan); tests/guarded.py's Arena puts the operands between guard bands
    d0 = place(nhwc(in0), "in", name="in0")
    d1 = place(nhwc(in1), "in", name="in1") if C1 else None
    dres = place(nhwc(res), "in", name="resid") if resid else None
    out = place((B, Ho >> pool, Wo >> pool, Cout), "out", name="out")
    L = _lib.lib()
    wc, bc = w.contiguous(), b.contiguous()
    rc = L.eamm_op_conv(0, d0.data_ptr(), C0, d1.data_ptr() if C1 else None, C1, B, H, W, up,
                        wc.data_ptr(), bc.data_ptr(), Cout, ks, kw, act, pool,
                        dres.data_ptr() if resid else None, splitk, tile_n, out.data_ptr(), 0, None,
                        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None)
    torch.cuda.synchronize()
    got = out.cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all(), "output has unwritten / non-finite elements"
    err = float((got - want).abs().max())
    scale = max(1.0, float(want.abs().max()))
    return err, scale


CASES = {
    # name: kwargs                                                       (shapes follow the network's layers)
    "3x3_tile32":        dict(B=1, H=16, W=16, C0=32, C1=0, Cout=32, ks=3),
    "3x3_tile64_relu":   dict(B=2, H=16, W=16, C0=64, C1=0, Cout=64, ks=3, act=1),
    "3x3_tile128_pool":  dict(B=1, H=32, W=32, C0=128, C1=0, Cout=256, ks=3, act=1, pool=1),
    "3x3_mtail_ntail":   dict(B=1, H=6, W=10, C0=32, C1=0, Cout=96, ks=3, act=1),
    "3x3_rect_pool":     dict(B=3, H=8, W=12, C0=64, C1=0, Cout=128, ks=3, act=1, pool=1),
    "3x3_up":            dict(B=2, H=8, W=8, C0=64, C1=0, Cout=32, ks=3, up=1, act=1),
    "3x3_up_concat":     dict(B=2, H=8, W=8, C0=64, C1=32, Cout=64, ks=3, up=1, act=1),
    "3x3_resid":         dict(B=1, H=16, W=16, C0=64, C1=0, Cout=64, ks=3, resid=True),
    "3x3_splitk3_pool":  dict(B=1, H=8, W=8, C0=96, C1=0, Cout=128, ks=3, act=1, pool=1, splitk=3),
    "3x3_splitk4":       dict(B=1, H=8, W=8, C0=64, C1=0, Cout=64, ks=3, act=1, splitk=4),
    "3x3_tile64_as_32":  dict(B=1, H=16, W=16, C0=32, C1=0, Cout=64, ks=3, tile_n=32),
    "3x3_tile128_as_64": dict(B=1, H=16, W=16, C0=32, C1=0, Cout=128, ks=3, tile_n=64),
    "3x3_odd_linear":    dict(B=2, H=5, W=7, C0=32, C1=0, Cout=64, ks=3, act=1),
    "3x3_up_odd_2x3":    dict(B=1, H=2, W=3, C0=64, C1=0, Cout=128, ks=3, up=1, act=1),
    "3x3_up_odd_split":  dict(B=3, H=3, W=3, C0=96, C1=32, Cout=32, ks=3, up=1, resid=True, splitk=2),
    "dma_odd_linear":    dict(B=2, H=9, W=15, C0=32, C1=0, Cout=128, ks=3, resid=True, tile_n=1002),
    "3x3_up_tile128":    dict(B=1, H=16, W=16, C0=64, C1=0, Cout=128, ks=3, up=1, act=1),
    "3x3_up_splitk3":    dict(B=1, H=4, W=6, C0=96, C1=32, Cout=64, ks=3, up=1, act=1, splitk=3),
    "3x3_up_resid":      dict(B=1, H=8, W=8, C0=32, C1=0, Cout=32, ks=3, up=1, resid=True),
    # LDS-DMA big-tile kernel (tile_n = 1000 + id): 256x256, 256x128, 512x64
    "dma256_basic":      dict(B=2, H=16, W=16, C0=64, C1=0, Cout=256, ks=3, act=1, tile_n=1001),
    "dma256_tails_res":  dict(B=1, H=10, W=14, C0=32, C1=0, Cout=272, ks=3, resid=True, tile_n=1001),
    "dma256_pool":       dict(B=3, H=16, W=16, C0=64, C1=0, Cout=256, ks=3, act=1, pool=1, tile_n=1001),
    "dma256_up_concat":  dict(B=2, H=8, W=8, C0=64, C1=32, Cout=256, ks=3, up=1, act=1, tile_n=1001),
    "dma256_splitk3":    dict(B=1, H=8, W=8, C0=96, C1=0, Cout=256, ks=3, act=1, splitk=3, tile_n=1001),
    "dma256x128":        dict(B=2, H=16, W=16, C0=64, C1=0, Cout=128, ks=3, act=1, tile_n=1002),
    "dma256x128_up":     dict(B=1, H=16, W=16, C0=64, C1=0, Cout=128, ks=3, up=1, act=1, tile_n=1002),
    "dma512x64":         dict(B=2, H=16, W=20, C0=32, C1=0, Cout=64, ks=3, act=1, tile_n=1003),
    "dma512x64_up":      dict(B=1, H=16, W=16, C0=128, C1=0, Cout=64, ks=3, up=1, act=1, tile_n=1003),
    # skinny LDS-DMA tiles (1004: 32x128, 1005: 64x128) of the deep hourglass levels at small batches
    "skinny32_enc4_like":  dict(B=1, H=4, W=4, C0=256, C1=0, Cout=256, ks=3, act=1, pool=1, tile_n=1004),
    "skinny32_dec0_like":  dict(B=2, H=2, W=2, C0=128, C1=0, Cout=256, ks=3, up=1, act=1, tile_n=1004),
    "skinny32_dec1_like":  dict(B=1, H=4, W=4, C0=128, C1=64, Cout=128, ks=3, up=1, act=1, tile_n=1004),
    "skinny32_mtail":      dict(B=1, H=5, W=5, C0=32, C1=0, Cout=136, ks=3, act=1, tile_n=1004),
    "skinny64_enc3_like":  dict(B=1, H=8, W=8, C0=128, C1=0, Cout=256, ks=3, act=1, pool=1, tile_n=1005),
    "skinny64_dec2_like":  dict(B=1, H=8, W=8, C0=64, C1=64, Cout=128, ks=3, up=1, act=1, tile_n=1005),
    "skinny64_splitk5":    dict(B=3, H=4, W=4, C0=160, C1=0, Cout=128, ks=3, resid=True, splitk=5, tile_n=1005),
    "dma256_bottleneck": dict(B=4, H=64, W=64, C0=256, C1=0, Cout=256, ks=3, resid=True, tile_n=1001),
    # column-patch kernel of the final layer's 7x1 convolution (tile_n = 4000): N = 32-float pixel stride
    "col7_final_like":   dict(B=2, H=32, W=32, C0=64, C1=0, Cout=32, ks=7, kw=1, tile_n=4000, zero_bias=True),
    "col7_one_chunk":    dict(B=1, H=16, W=48, C0=32, C1=0, Cout=32, ks=7, kw=1, tile_n=4000, zero_bias=True),
    "col7_ragged":       dict(B=3, H=20, W=24, C0=64, C1=0, Cout=32, ks=7, kw=1, tile_n=4000, zero_bias=True),
    "col7s_head_like":   dict(B=2, H=32, W=32, C0=64, C1=64, Cout=96, ks=7, kw=1, tile_n=4001, zero_bias=True),
    "col7s_ragged":      dict(B=3, H=20, W=24, C0=32, C1=32, Cout=96, ks=7, kw=1, tile_n=4001, zero_bias=True),
    "col7s_one_input":   dict(B=1, H=16, W=16, C0=96, C1=0, Cout=96, ks=7, kw=1, tile_n=4001, zero_bias=True),
    "col7_many_tiles":   dict(B=5, H=128, W=128, C0=64, C1=0, Cout=32, ks=7, kw=1, tile_n=4000, zero_bias=True),
    # spatial-patch kernel for the collapsed up-convolution (tile_n = 3000)
    "patch_up_basic":    dict(B=2, H=16, W=16, C0=64, C1=0, Cout=64, ks=3, up=1, act=1, tile_n=3000),
    "patch_up_concat":   dict(B=1, H=32, W=16, C0=32, C1=64, Cout=128, ks=3, up=1, act=1, tile_n=3000),
    "patch_up_ragged":   dict(B=2, H=10, W=22, C0=32, C1=0, Cout=40, ks=3, up=1, act=1, tile_n=3000),
    "patch_up1_like":    dict(B=1, H=64, W=64, C0=128, C1=0, Cout=64, ks=3, up=1, act=1, tile_n=3000),
    # ... in polyphase minimal-filtering form (tile_n = 3003)
    "ppoly_up_basic":    dict(B=2, H=16, W=16, C0=64, C1=0, Cout=64, ks=3, up=1, act=1, tile_n=3003),
    "ppoly_up_concat":   dict(B=1, H=32, W=16, C0=32, C1=64, Cout=128, ks=3, up=1, act=1, tile_n=3003),
    "ppoly_up_ragged":   dict(B=2, H=10, W=22, C0=32, C1=0, Cout=40, ks=3, up=1, act=1, tile_n=3003),
    "ppoly_up_odd":      dict(B=1, H=9, W=7, C0=32, C1=0, Cout=64, ks=3, up=1, act=0, tile_n=3003),
    "ppoly_up1_like":    dict(B=1, H=64, W=64, C0=128, C1=0, Cout=64, ks=3, up=1, act=1, tile_n=3003),
    "ppoly_up0_like":    dict(B=2, H=32, W=32, C0=256, C1=0, Cout=128, ks=3, up=1, act=0, tile_n=3003),
    # ... with the channel reduction split over workgroups (the hourglass decoder's last levels)
    "ppoly_split2_dec4": dict(B=2, H=32, W=32, C0=128, C1=128, Cout=64, ks=3, up=1, act=1, splitk=2, tile_n=3003),
    "ppoly_split4_dec3": dict(B=3, H=16, W=16, C0=256, C1=256, Cout=128, ks=3, up=1, act=1, splitk=4, tile_n=3003),
    "ppoly_split2_rag":  dict(B=1, H=18, W=20, C0=64, C1=64, Cout=40, ks=3, up=1, act=0, splitk=2, tile_n=3003),
    # Winograd F(2x2,3x3) path (tile_n = 2000)
    "wino_basic":        dict(B=2, H=16, W=16, C0=64, C1=0, Cout=128, ks=3, act=1, tile_n=2000),
    "wino_tails_resid":  dict(B=1, H=6, W=10, C0=64, C1=0, Cout=136, ks=3, resid=True, tile_n=2000),
    "wino_bottleneck":   dict(B=4, H=64, W=64, C0=256, C1=0, Cout=256, ks=3, resid=True, tile_n=2000),
    "wino_ring5":        dict(B=1, H=6, W=10, C0=128, C1=0, Cout=136, ks=3, resid=True, tile_n=2000),   # Cin = 128, ragged Cout
    # Winograd F(4x4,3x3) path (tile_n = 2100 + pipeline variant: 0, 3 = one DMA piece per 8 MFMAs, 6 = 3 with non-temporal V
    # loads; "ring3" / "ring4" / "interleaved" name pipelines that are gone -- the cases keep their shapes on a kept variant)
    "wino4_basic":       dict(B=2, H=16, W=16, C0=128, C1=0, Cout=128, ks=3, act=1, tile_n=2100),
    "wino4_sub2":        dict(B=2, H=16, W=16, C0=64, C1=0, Cout=64, ks=3, act=1, tile_n=2100),
    "wino4_tails_resid": dict(B=1, H=8, W=12, C0=64, C1=0, Cout=136, ks=3, resid=True, tile_n=2100),
    "wino4_bottleneck":  dict(B=4, H=64, W=64, C0=256, C1=0, Cout=256, ks=3, resid=True, tile_n=2100),
    "wino4_ring3":       dict(B=3, H=16, W=20, C0=128, C1=0, Cout=96, ks=3, act=1, tile_n=2103),
    "wino4_pe8":         dict(B=2, H=16, W=16, C0=128, C1=0, Cout=128, ks=3, act=1, tile_n=2103),
    "wino4_ring4":       dict(B=1, H=12, W=8, C0=192, C1=0, Cout=64, ks=3, resid=True, tile_n=2106),   # Cin = 192: the two-chunk fallback
    "wino4_split6":      dict(B=1, H=16, W=16, C0=128, C1=0, Cout=128, ks=3, act=1, tile_n=2156),
    "wino4_split3_res":  dict(B=2, H=8, W=12, C0=64, C1=0, Cout=136, ks=3, resid=True, tile_n=2153),
    "wino4_split2":      dict(B=1, H=64, W=64, C0=256, C1=0, Cout=256, ks=3, resid=True, tile_n=2152),
    # ... with the DownBlock2d epilogue (ReLU, 2x2 average) in the output-transform kernel: the hourglass encoder levels
    "wino4_pool_enc0":   dict(B=2, H=64, W=64, C0=64, C1=0, Cout=128, ks=3, act=1, pool=1, tile_n=2152),
    "wino4_pool_enc1":   dict(B=2, H=32, W=32, C0=128, C1=0, Cout=256, ks=3, act=1, pool=1, tile_n=2153),
    "wino4_pool_enc3":   dict(B=3, H=8, W=8, C0=512, C1=0, Cout=1024, ks=3, act=1, pool=1, tile_n=2156),
    # one frame of the bottleneck: 32-tile four-wave blocks, six transform-point rows per tile, residual in the output transform
    "wino4_one_frame_narrow": dict(B=1, H=64, W=64, C0=256, C1=0, Cout=256, ks=3, resid=True, tile_n=2156),
    "wino4_pool_ragged": dict(B=1, H=12, W=20, C0=64, C1=0, Cout=72, ks=3, act=1, pool=1, tile_n=2156),
    "wino4_interleaved": dict(B=3, H=16, W=20, C0=128, C1=0, Cout=96, ks=3, resid=True, tile_n=2106),
    "7x1_rowsplit":      dict(B=2, H=16, W=16, C0=64, C1=0, Cout=21, ks=7, kw=1),
    "7x7_head":          dict(B=1, H=16, W=16, C0=32, C1=64, Cout=12, ks=7),
    "7x7_sigmoid":       dict(B=1, H=32, W=32, C0=32, C1=0, Cout=3, ks=7, act=2),
    "7x7_first":         dict(B=1, H=32, W=32, C0=32, C1=0, Cout=64, ks=7, act=1),
    "bottleneck_256":    dict(B=2, H=64, W=64, C0=256, C1=0, Cout=256, ks=3, resid=True),
    "hg_enc4_autosplit": dict(B=4, H=4, W=4, C0=1024, C1=0, Cout=1024, ks=3, act=1, pool=1),
    "hg_dec1_autosplit": dict(B=2, H=4, W=4, C0=1024, C1=1024, Cout=512, ks=3, up=1, act=1),
    "hg_dec0_2x2":       dict(B=1, H=2, W=2, C0=1024, C1=0, Cout=1024, ks=3, up=1, act=1),
    "up1_like":          dict(B=1, H=64, W=64, C0=128, C1=0, Cout=64, ks=3, up=1, act=1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_conv_mfma_matches_torch(name):
    err, scale = run_case(**CASES[name], seed=hash(name) % 1000)
    # exact-fp32 MFMA (fmaf chain) vs oneDNN: only summation order differs
    # Winograd: same fp32 arithmetic, but the transform-domain sums cancel -> a few ulp more rounding
    assert err <= (6e-5 if CASES[name].get("tile_n", 0) >= 2000 else 2e-5) * scale, (name, err, scale)


def test_removed_winograd_launch_forms_are_refused(monkeypatch):
    """The GEMM pipeline variants other than 0 / 3 / 6, the F(2x2) variants and the half-row split are gone: the operator entry
    refuses their tile codes before it launches a GEMM, and eamm_create refuses an EAMM_WINO4_VARIANT the library does not have
    (it used to be accepted and then fail every forward)."""
    from eamm_amd import tiny_config
    from eamm_amd.engine import Engine
    shape = dict(B=1, H=16, W=16, C0=128, C1=0, Cout=128, ks=3)
    for tile_n in (2001, 2006, 2101, 2102, 2104, 2105, 2162):
        with pytest.raises(_lib.EammError):
            run_case(**shape, tile_n=tile_n)
    for variant in ("1", "2", "4", "5", "7"):
        monkeypatch.setenv("EAMM_WINO4_VARIANT", variant)
        with pytest.raises(_lib.EammError, match="EAMM_WINO4_VARIANT=" + variant) as exc:
            Engine(tiny_config(), 64, 64)
        assert exc.value.code == _lib.ERR_ARG
    for variant in ("0", "3", "6"):
        monkeypatch.setenv("EAMM_WINO4_VARIANT", variant)
        Engine(tiny_config(), 64, 64)


def test_conv_linearity_property():
    """Size-independent property at a full-size layer: conv(a*x) == a*conv(x) for a power of two
    (bit-exact in fp32) -- catches dropped K chunks / stale accumulators without a CPU reference."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    B, H, W, Cc = 4, 64, 64, 256
    x = torch.randn(B, H, W, Cc, generator=g).to(dev)
    w = (torch.randn(Cc, Cc, 3, 3, generator=g) * (1.0 / (Cc * 9)) ** 0.5).contiguous()
    b = torch.zeros(Cc)
    L = _lib.lib()
    outs = []
    for scale in (1.0, 4.0):
        xin = (x * scale).contiguous()
        out = torch.empty(B, H, W, Cc, device=dev)
        _lib.check(L.eamm_op_conv(0, xin.data_ptr(), Cc, None, 0, B, H, W, 0, w.data_ptr(), b.data_ptr(), Cc, 3, 3, 0, 0,
                                  None, 0, 0, out.data_ptr(), 0, None, torch.cuda.current_stream().cuda_stream),
                   None)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0] * 4.0, outs[1])
    assert float(outs[0].abs().max()) > 0.5


# ---- the HBM-bound kernel of the path on its own: feature warp x occlusion (reference generator.py:50-57, 79-84) -------
def _warp_case(n, ns, hf, wf, C, h, w, occ=True, seed=0, poison=False, place=None):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(ns, C, hf, wf, generator=g)
    if poison:   # a non-finite BORDER value must not leak into samples whose out-of-range corner is zero padding
        feat[:, :, 0, 0] = float("inf")
    ident = torch.stack(torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")[::-1], -1)
    defo = ident[None] + 0.3 * torch.randn(n, h, w, 2, generator=g)          # some samples fall outside the map
    if poison:
        defo[:, 0, 0] = torch.tensor([-1.0 - 1.5 / wf, -1.0 - 1.5 / hf])    # top-left sample: every corner out of range -> exactly 0
    om = torch.rand(n, 1, h, w, generator=g) if occ else None
    src = feat if ns == n else feat.expand(n, -1, -1, -1)
    d, o = defo, om
    if (h, w) != (hf, wf):    # generator.py:52-56, 82-83
        d = F.interpolate(defo.permute(0, 3, 1, 2), size=(hf, wf), mode="bilinear").permute(0, 2, 3, 1)
        o = F.interpolate(om, size=(hf, wf), mode="bilinear") if occ else None
    want = F.grid_sample(src, d, mode="bilinear", padding_mode="zeros", align_corners=False)
    if occ:
        want = want * o
    dev = torch.device("cuda:0")
    place = place or Plain(dev)
    f_d, d_d = place(nhwc(feat), "in", name="features"), place(defo.contiguous(), "in", name="deformation")
    o_d = place(om[:, 0].contiguous(), "in", name="occlusion") if occ else None
    out = place((n, hf, wf, C), "out", name="out")
    rc = _lib.lib().eamm_op_warp(0, f_d.data_ptr(), d_d.data_ptr(), o_d.data_ptr() if occ else None, n, ns, hf, wf, C, h, w,
                                 out.data_ptr(), 0, None, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None)
    return out.cpu().permute(0, 3, 1, 2), want


@pytest.mark.parametrize("name,kw", [
    ("one_source", dict(n=3, ns=1, hf=16, wf=16, C=64, h=16, w=16)),
    ("per_frame_source", dict(n=2, ns=2, hf=12, wf=20, C=32, h=12, w=20, seed=1)),
    ("no_occlusion", dict(n=2, ns=1, hf=16, wf=16, C=256, h=16, w=16, occ=False, seed=2)),
    ("resized_flow", dict(n=2, ns=1, hf=32, wf=32, C=64, h=16, w=16, seed=3)),
])
def test_warp_features_matches_grid_sample(name, kw):
    got, want = _warp_case(**kw)
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"warp {name}: max|hip - grid_sample| = {err:.2e}")
    assert err <= 2e-5 * max(1.0, float(want.abs().max())), (name, err)


def test_warp_zero_padding_is_exact_beside_a_non_finite_border_pixel():
    """a clamped out-of-range corner with weight 0 would give 0 * inf = NaN; grid_sample's zeros padding gives 0."""
    got, want = _warp_case(n=1, ns=1, hf=8, wf=8, C=32, h=8, w=8, occ=False, seed=5, poison=True)
    assert float(got[0, :, 0, 0].abs().max()) == 0.0 and float(want[0, :, 0, 0].abs().max()) == 0.0
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin)
    assert float((got[fin] - want[fin]).abs().max()) <= 2e-5 * max(1.0, float(want[fin].abs().max()))


# ---- the generator's final layer whole: 7x7 conv (64 -> 3) + bias + sigmoid on the fused column-patch kernel (round 3) ------
@pytest.mark.parametrize("name,B,H,W,C", [
    ("one_tile_row", 1, 16, 64, 64),          # tiles_y = 1: four tiles walked left to right, carries between them
    ("final_like", 2, 64, 64, 64),
    ("one_chunk", 1, 32, 48, 32),
    ("ragged", 3, 20, 24, 64),                # H, W not multiples of the 16x16 tile: partial last tile in both directions
    ("narrow", 2, 40, 12, 64),                # one tile per row: first and last at once
    ("many_rows", 5, 128, 128, 64),           # more tile rows (40) than ... not than CUs; several images
    ("more_rows_than_cus", 20, 256, 16, 32),  # 320 tile rows on <= 256 persistent workgroups: a workgroup walks two rows
])
def test_fused_final_layer_matches_torch(name, B, H, W, C, place=None):
    g = torch.Generator().manual_seed(hash(name) % 1000)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(3, C, 7, 7, generator=g) * (2.0 / (C * 49)) ** 0.5
    b = 0.1 * torch.randn(3, generator=g)
    want = torch.sigmoid(F.conv2d(x, w, b, padding=3))
    dev = torch.device("cuda:0")
    place = place or Plain(dev)
    xd = place(nhwc(x), "in", name="in0")
    out = place((B, 3, H, W), "out", name="out")
    wc, bc = w.contiguous(), b.contiguous()
    rc = _lib.lib().eamm_op_conv(0, xd.data_ptr(), C, None, 0, B, H, W, 0, wc.data_ptr(), bc.data_ptr(), 3, 7, 7, 2, 0, None, 0, 4002,
                                 out.data_ptr(), 0, None, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None)
    got = out.cpu()
    assert torch.isfinite(got).all(), "output has unwritten / non-finite elements"
    err = float((got - want).abs().max())
    print(f"fused final {name}: max|hip - torch| = {err:.2e}")
    assert err <= 2e-6, (name, err)


def test_bottleneck_gemm_is_deterministic_under_load():
    """The F(4x4) bottleneck convolution at the benchmark's launch sizes (8 and 16 frames: 128 / 256 workgroups), 60 back-to-back
    runs each: every run must be bit-identical to the first (a race in an LDS-staged epilogue shows up as a few wrong
    elements in one run out of two at these sizes -- round 3 met one in an experimental kernel) and agree with the direct
    convolution to rounding."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    L = _lib.lib()
    Cc = 256

    def run(tile, B, x, w, b, r):
        out = torch.full((B, 64, 64, Cc), float("nan"), device=dev)
        _lib.check(L.eamm_op_conv(0, x.data_ptr(), Cc, None, 0, B, 64, 64, 0, w.data_ptr(), b.data_ptr(), Cc, 3, 3, 0, 0, r.data_ptr(), 0, tile,
                                  out.data_ptr(), 0, None, st), None)
        return out

    for B in (8, 16):
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 64, 64, Cc, generator=g).to(dev)
        r = torch.randn(B, 64, 64, Cc, generator=g).to(dev)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) * (2.0 / (Cc * 9)) ** 0.5).contiguous()
        b = 0.1 * torch.randn(Cc, generator=g)
        first = run(2103, B, x, w, b, r)
        torch.cuda.synchronize()
        assert torch.isfinite(first).all()
        differing = sum(int(not torch.equal(run(2103, B, x, w, b, r), first)) for _ in range(60))
        assert differing == 0, (B, differing)
        direct = run(1001, B, x, w, b, r)      # 256x256 LDS-DMA tile, direct form
        assert float((first - direct).abs().max()) <= 2e-5 * float(direct.abs().max())
