"""The split-bf16 product form of the polyphase up-block kernel (conv_mfma_patch_poly.hip, FORM 1): every fp32 operand is the exact
sum of three bf16 values and a product is six bf16 MFMAs with fp32 accumulation.  It runs in the whole-tile launches (no split of
the channel reduction) of a layer that has the three-plane weight image; everything here goes through the operator entry
eamm_op_conv with tile code 3003 (the polyphase form as the engine runs a decoder up block) or 3004 (fp32 products forced) and is
compared with a float64 interpolate(nearest x2) + conv2d on the CPU.

PARENT holds max |out - float64| / max |float64| of the fp32-MFMA kernel, measured with measure() below at tile code 3003 on a
build of the commit before this form existed (profiles/ppoly_split_accuracy.txt keeps both columns).  The split form may take at
most twice that: the products drop terms <= 2^-24 relative, so what is left is summation order (K blocks of 16 instead of 2) and
the MFMA's internal rounding.  PARENT_SHA256 holds the SHA-256 of that build's output bytes: the fp32 form must not have changed.
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
    "one_chunk_one_tile": dict(B=1, H=16, W=16, C0=32, C1=0, Cout=32),                 # prologue only, the ring never wraps
    "odd_chunks":         dict(B=1, H=16, W=16, C0=96, C1=0, Cout=64, act=1),          # odd chunk count
    "ragged":             dict(B=2, H=10, W=22, C0=32, C1=0, Cout=40),                 # partial tiles, N tail
    "concat":             dict(B=1, H=32, W=16, C0=32, C1=64, Cout=128),               # a chunk on each side of the input boundary
    "up0_like":           dict(B=2, H=32, W=32, C0=256, C1=0, Cout=128),
    "up1_like":           dict(B=1, H=64, W=64, C0=128, C1=0, Cout=64),
    # adversarial magnitudes: input plane 5 x 1e4, input plane 9 x 1e-4, output channel 3 of the weights x 1e3
    "ragged_adversarial": dict(B=2, H=10, W=22, C0=32, C1=0, Cout=40, adversarial=True),
    "concat_adversarial": dict(B=1, H=32, W=16, C0=32, C1=64, Cout=128, adversarial=True),
    "splitk":             dict(B=3, H=16, W=16, C0=256, C1=256, Cout=128, splitk=4),   # stays on the fp32 form
}

# max |out - float64| / max |float64| of the parent's fp32 kernel at tile code 3003 (see the module docstring)
PARENT = {
    "one_chunk_one_tile": 2.291490e-07,
    "odd_chunks": 4.608286e-07,
    "ragged": 3.652650e-07,
    "concat": 4.864887e-07,
    "up0_like": 8.117899e-07,
    "up1_like": 5.752481e-07,
    "ragged_adversarial": 4.148053e-07,
    "concat_adversarial": 7.345849e-07,
    "splitk": 4.551576e-07,
}
# sha256 of the parent's output bytes (NHWC float32) at tile code 3003
PARENT_SHA256 = {
    "ragged": "08af3bf3fef59d8388d392538daad4afbe277cd54ac7ee3a627565348a3f6a74",
    "up1_like": "09d0a9da3e785d8703f6c92ba28c8a482793cf75e59315d30c873aec78fcf09c",
    "splitk": "63e463a942fa7de6903f0f633ca96fefc6a51d71ff845460a34187ef73f30427",
}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def problem(name):
    """Seeded inputs and the float64 reference of a case: (x [B, C0 + C1, H, W], w, b, want float64 NCHW).  Computed once, never written."""
    c = CASES[name]
    cin = c["C0"] + c["C1"]
    g = torch.Generator().manual_seed(2000 + list(CASES).index(name))
    x = torch.randn(c["B"], cin, c["H"], c["W"], generator=g)
    w = torch.randn(c["Cout"], cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = 0.1 * torch.randn(c["Cout"], generator=g)
    if c.get("adversarial"):
        x[:, 5] *= 1e4
        x[:, 9] *= 1e-4
        w[3] *= 1e3
    want = reference(x, w, b, c.get("act", 0))
    return x, w, b, want


def reference(x, w, b, act):
    want = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
    return F.relu(want) if act else want


def launch(name, x=None, tile_n=3003, place=None):
    """One eamm_op_conv call of the case (optionally on another input / tile code) -> NHWC float32 output on the CPU."""
    c = CASES[name]
    x0, w, b, _ = problem(name)
    x = x0 if x is None else x
    dev = torch.device("cuda:0")
    place = place or Plain(dev)     # .to(dev) / torch.full(nan); tests/guarded.py's Arena puts the operands between guard bands
    d0 = place(nhwc(x[:, :c["C0"]]), "in", name="in0")
    d1 = place(nhwc(x[:, c["C0"]:]), "in", name="in1") if c["C1"] else None
    out = place((c["B"], 2 * c["H"], 2 * c["W"], c["Cout"]), "out", name="out")
    wc, bc = w.contiguous(), b.contiguous()
    rc = _lib.lib().eamm_op_conv(0, d0.data_ptr(), c["C0"], d1.data_ptr() if d1 is not None else None, c["C1"], c["B"], c["H"], c["W"],
                                 1, wc.data_ptr(), bc.data_ptr(), c["Cout"], 3, 3, c.get("act", 0), 0, None, c.get("splitk", 0),
                                 tile_n, out.data_ptr(), 0, None, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None)
    torch.cuda.synchronize()
    return out.cpu()


def measure(name, tile_n=3003, place=None):
    """-> (max |out - float64| / max |float64|, max |out - float64|, max |float64|, output)"""
    want = problem(name)[3]
    out = launch(name, tile_n=tile_n, place=place)
    assert torch.isfinite(out).all(), "output has unwritten / non-finite elements"
    err = float((out.permute(0, 3, 1, 2).double() - want).abs().max())
    top = float(want.abs().max())
    return err / top, err, top, out


def sha256(out):
    return hashlib.sha256(out.numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("name", list(CASES))
def test_split_accuracy_within_twice_the_fp32_kernel(name):
    rel, err, top, out = measure(name)
    print(f"{name}: max|out - f64| / max|f64| = {rel:.4e} (parent fp32 kernel {PARENT[name]:.4e}), max|f64| = {top:.4e}")
    assert rel <= 2.0 * PARENT[name], (name, rel, PARENT[name])
    assert err <= 6e-5 * max(1.0, top), (name, err, top)      # the bound of tests/test_gpu_ops.py for these tile codes
    if name == "splitk":                                      # the dispatch leaves split reductions on the fp32 form
        assert sha256(out) == PARENT_SHA256[name]


@pytest.mark.parametrize("name", list(PARENT_SHA256))
def test_fp32_form_is_bit_equal_to_the_parent(name):
    assert sha256(launch(name, tile_n=3004)) == PARENT_SHA256[name]


def non_finite_case():
    """"concat" with a NaN and an inf at one interior low-resolution pixel (one channel of each input), on a tile boundary in y."""
    name, bb, py, px = "concat", 0, 15, 8
    x = problem(name)[0].clone()
    x[bb, 7, py, px] = float("nan")
    x[bb, 70, py, px] = float("inf")
    return name, x, bb, py, px


def test_non_finite_inputs_stay_non_finite():
    """The centre pixel is the common term of the three products of a dimension and a neighbour enters one difference, so a
    non-finite low-resolution pixel (y, x) reaches exactly the outputs the reference's convolution of the up-sampled map gives
    it: rows 2y-1 .. 2y+2 and columns 2x-1 .. 2x+2, in every output channel (no activation here: relu would turn a NaN into 0).
    The parent's fp32 form produces this set; the split form must produce the same one (an inf splits into inf + NaN + NaN)."""
    name, x, bb, py, px = non_finite_case()
    expect = torch.zeros(CASES[name]["B"], 2 * CASES[name]["H"], 2 * CASES[name]["W"], CASES[name]["Cout"], dtype=torch.bool)
    expect[bb, 2 * py - 1:2 * py + 3, 2 * px - 1:2 * px + 3, :] = True
    for tile_n in (3003, 3004):
        assert torch.equal(~torch.isfinite(launch(name, x=x, tile_n=tile_n)), expect), tile_n


def test_split_is_deterministic():
    first = launch("up0_like")
    assert torch.equal(launch("up0_like"), first)
