"""The split-bf16 product form of the F(4x4,3x3) Winograd GEMM (conv_winograd4.hip, SPLIT 1): every fp32 operand is the exact sum
of three bf16 values and a product is six bf16 MFMAs with fp32 accumulation.  It runs in the whole-tile launches (groups == 1) of
pipeline variants 3 / 6 on layers with Cin % 128 == 0; everything here goes through the operator entry eamm_op_conv with the tile
codes of tests/test_gpu_ops.py (2103 / 2106) and is compared with a float64 conv2d on the CPU.

PARENT holds max |out - float64| / max |float64| of the fp32-MFMA kernel this form replaced, measured with measure() below on a
build of the commit before it (profiles/wino4_split_accuracy.txt keeps both columns).  The split form may take at most twice that:
the products drop terms <= 2^-24 relative, so what is left is summation order and the MFMA's internal rounding.
"""
import functools
import hashlib

import pytest
import torch
import torch.nn.functional as F

from eamm_amd import _lib
from guarded import Plain

pytestmark = pytest.mark.gpu

CASES = {
    "smallest_4chunk":   dict(B=2, H=16, W=16, Cin=128, Cout=128, act=1, tile_n=2103),                # the smallest launch on the 4-chunk path
    "tails_resid":       dict(B=1, H=8, W=12, Cin=256, Cout=136, resid=True, tile_n=2106),            # M tail and N tail
    "interleaved_resid": dict(B=3, H=16, W=20, Cin=128, Cout=96, resid=True, tile_n=2106),            # tiles interleaved across frames
    "fallback_192":      dict(B=1, H=12, W=8, Cin=192, Cout=64, tile_n=2106),                         # two-chunk fallback: still the fp32 form
    "bottleneck":        dict(B=4, H=64, W=64, Cin=256, Cout=256, resid=True, tile_n=2106),           # the bottleneck's own tile counts
    # adversarial magnitudes: input plane 5 x 1e4, input plane 9 x 1e-4, output channel 3 of the weights x 1e3
    "adversarial":       dict(B=2, H=16, W=16, Cin=128, Cout=128, act=1, tile_n=2103, adversarial=True),
    "adversarial_resid": dict(B=3, H=16, W=20, Cin=128, Cout=96, resid=True, tile_n=2106, adversarial=True),
}

# max |out - float64| / max |float64| of the parent's fp32 kernel (see the module docstring)
PARENT = {
    "smallest_4chunk": 8.567141e-06,
    "tails_resid": 8.378228e-06,
    "interleaved_resid": 6.409466e-06,
    "fallback_192": 1.041667e-05,
    "bottleneck": 1.174302e-05,
    "adversarial": 1.026309e-05,
    "adversarial_resid": 4.745313e-06,
}
# sha256 of the parent's output bytes (NHWC float32) for "fallback_192": that launch keeps the fp32 kernel, bit for bit
PARENT_FALLBACK_SHA256 = "cc328c315c000410ab02a2d983ddc3137bcc9a696790a85015cca7e88e149558"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def problem(name):
    """Seeded inputs and the float64 reference of a case: (x, w, b, resid or None, want float64 NCHW).  Computed once, never written."""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    x = torch.randn(c["B"], c["Cin"], c["H"], c["W"], generator=g)
    w = torch.randn(c["Cout"], c["Cin"], 3, 3, generator=g) * (2.0 / (c["Cin"] * 9)) ** 0.5
    b = 0.1 * torch.randn(c["Cout"], generator=g)
    res = torch.randn(c["B"], c["Cout"], c["H"], c["W"], generator=g) if c.get("resid") else None
    if c.get("adversarial"):
        x[:, 5] *= 1e4
        x[:, 9] *= 1e-4
        w[3] *= 1e3
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    if res is not None:
        want = want + res.double()
    if c.get("act"):
        want = F.relu(want)
    return x, w, b, res, want


def launch(name, x=None, tile_n=None, place=None):
    """One eamm_op_conv call of the case (optionally on another input / tile code) -> NHWC float32 output on the CPU."""
    c = CASES[name]
    x0, w, b, res, _ = problem(name)
    x = x0 if x is None else x
    dev = torch.device("cuda:0")
    place = place or Plain(dev)     # .to(dev) / torch.full(nan); tests/guarded.py's Arena puts the operands between guard bands
    dx = place(nhwc(x), "in", name="in0")
    dres = place(nhwc(res), "in", name="resid") if res is not None else None
    out = place((c["B"], c["H"], c["W"], c["Cout"]), "out", name="out")
    wc, bc = w.contiguous(), b.contiguous()
    rc = _lib.lib().eamm_op_conv(0, dx.data_ptr(), c["Cin"], None, 0, c["B"], c["H"], c["W"], 0, wc.data_ptr(), bc.data_ptr(),
                                 c["Cout"], 3, 3, c.get("act", 0), 0, dres.data_ptr() if dres is not None else None, 0,
                                 tile_n or c["tile_n"], out.data_ptr(), 0, None, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None)
    torch.cuda.synchronize()
    return out.cpu()


def measure(name, place=None):
    """-> (max |out - float64| / max |float64|, max |out - float64|, max |float64|, output)"""
    want = problem(name)[4]
    out = launch(name, place=place)
    assert torch.isfinite(out).all(), "output has unwritten / non-finite elements"
    err = float((out.permute(0, 3, 1, 2).double() - want).abs().max())
    top = float(want.abs().max())
    return err / top, err, top, out


@pytest.mark.parametrize("name", list(CASES))
def test_split_accuracy_within_twice_the_fp32_kernel(name):
    rel, err, top, out = measure(name)
    print(f"{name}: max|out - f64| / max|f64| = {rel:.4e} (parent fp32 kernel {PARENT[name]:.4e}), max|f64| = {top:.4e}")
    assert rel <= 2.0 * PARENT[name], (name, rel, PARENT[name])
    assert err <= 6e-5 * max(1.0, top), (name, err, top)      # the bound of tests/test_gpu_ops.py for the Winograd forms
    if name == "fallback_192":
        assert hashlib.sha256(out.numpy().tobytes()).hexdigest() == PARENT_FALLBACK_SHA256


def test_non_finite_inputs_stay_non_finite():
    """A NaN and an inf at one input pixel (two channels).  A Winograd tile is transformed as a whole -- B^T d B spreads a pixel over
    its 6x6 patch's transform points and A^T M A over the tile's 4x4 outputs, in either product form -- so the non-finite outputs are
    EXACTLY the 4x4 tiles whose 6x6 input patch holds the pixel, in every channel: a superset of the pixel's 3x3 footprint, which
    must be non-finite throughout, and nothing else (no activation here: relu would turn a NaN into 0)."""
    name = "interleaved_resid"
    c = CASES[name]
    x = problem(name)[0].clone()
    bb, py, px = 1, 8, 11        # on a tile corner: four tiles' patches hold it, the footprint touches all four
    x[bb, 7, py, px] = float("nan")
    x[bb, 70, py, px] = float("inf")
    bad = ~torch.isfinite(launch(name, x=x))                      # [B, H, W, Cout]
    assert bad[bb, py - 1:py + 2, px - 1:px + 2, :].all()         # the 3x3 footprint, every channel
    expect = torch.zeros_like(bad)
    for qy in range(c["H"] // 4):
        for qx in range(c["W"] // 4):
            if 4 * qy - 1 <= py <= 4 * qy + 4 and 4 * qx - 1 <= px <= 4 * qx + 4:
                expect[bb, 4 * qy:4 * qy + 4, 4 * qx:4 * qx + 4, :] = True
    assert torch.equal(bad, expect)


def test_split_is_deterministic_and_cache_variants_are_bit_equal():
    name = "interleaved_resid"
    first = launch(name, tile_n=2103)
    assert torch.equal(launch(name, tile_n=2103), first)
    assert torch.equal(launch(name, tile_n=2106), first)          # variant 6 = variant 3 with non-temporal V loads
