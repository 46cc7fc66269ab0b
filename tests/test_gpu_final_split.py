"""The split-bf16 product form of the fused final layer (conv_col7b_kernel, conv_col7.hip): every fp32 operand is the exact sum of
three bf16 values and a product is six bf16 MFMAs with fp32 accumulation; a patch value is split once, in LDS, by the wave that
fetched it.  Everything here goes through the operator entry eamm_op_conv with tile code 4002 (the final layer as the engine runs
it: split-bf16 products) or 4003 (fp32 products forced) and is compared with sigmoid(conv2d) in float64 on the CPU.

PARENT holds max |out - float64| of the fp32-MFMA kernel, measured with measure() below at tile code 4002 on a build of the commit
before this form existed (profiles/final_split_accuracy.txt keeps both columns).  The split form may take at most twice that: the
products drop terms <= 2^-24 relative, so what is left is summation order (K blocks of 16 instead of 1) and the MFMA's internal
rounding.  PARENT_SHA256 holds the SHA-256 of that build's output bytes: the fp32 form must not have changed.
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
    "one_tile":                  dict(B=1, H=16, W=16, C=32),     # prologue only, two 16-channel units, tile first and last of its row
    "one_tile_row":              dict(B=1, H=16, W=64, C=64),     # carries across four tiles
    "ragged":                    dict(B=3, H=20, W=24, C=64),     # partial last tile both ways
    "narrow":                    dict(B=2, H=40, W=12, C=64),
    "more_rows_than_workgroups": dict(B=20, H=256, W=16, C=32),   # 320 tile rows: a persistent workgroup walks two
    # input channel 5 x 1e4 with its weights x 1e-4, channel 9 x 1e-4 with its weights x 1e4: logits stay O(1), operands span 8 decades
    "ragged_adversarial":        dict(B=3, H=20, W=24, C=64, adversarial=True),
    "one_tile_row_adversarial":  dict(B=1, H=16, W=64, C=64, adversarial=True),
}

# max |out - float64| of the parent's fp32 kernel at tile code 4002 (see the module docstring)
PARENT = {
    "one_tile": 3.367077e-07,
    "one_tile_row": 5.627656e-07,
    "ragged": 4.371474e-07,
    "narrow": 4.399881e-07,
    "more_rows_than_workgroups": 4.650550e-07,
    "ragged_adversarial": 3.936485e-07,
    "one_tile_row_adversarial": 4.954875e-07,
}
# sha256 of the parent's output bytes (NCHW float32) at tile code 4002
PARENT_SHA256 = {
    "one_tile_row": "b8c9fd5a8bb5078fe8b9379e4de4523f8606c293a9a692a3000a9a663b562360",
    "ragged": "19501c9215e76c3ee11c3394c068ca6c8060cd56a0495edc6a399f9c628ebbcd",
    "more_rows_than_workgroups": "435aa1bd811bb3726eef77cc5e174ee81c135bbaf55ee56838ac4b92886c2dea",
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """Seeded inputs and the float64 reference of a case: (x [B, C, H, W], w, b, want float64 NCHW).  Computed once, never written."""
    c = CASES[name]
    g = torch.Generator().manual_seed(4000 + list(CASES).index(name))
    x = torch.randn(c["B"], c["C"], c["H"], c["W"], generator=g)
    w = torch.randn(3, c["C"], 7, 7, generator=g) * (2.0 / (c["C"] * 49)) ** 0.5
    b = 0.1 * torch.randn(3, generator=g)
    if c.get("adversarial"):
        x[:, 5] *= 1e4
        w[:, 5] *= 1e-4
        x[:, 9] *= 1e-4
        w[:, 9] *= 1e4
    return x, w, b, reference(x, w, b)


def reference(x, w, b):
    return torch.sigmoid(F.conv2d(x.double(), w.double(), b.double(), padding=3))


def launch(name, x=None, tile_n=4002, place=None):
    """One eamm_op_conv call of the case (optionally on another input / tile code) -> NCHW float32 output on the CPU."""
    c = CASES[name]
    x0, w, b, _ = problem(name)
    x = x0 if x is None else x
    dev = torch.device("cuda:0")
    place = place or Plain(dev)     # .to(dev) / torch.full(nan); tests/guarded.py's Arena puts the operands between guard bands
    d = place(x.permute(0, 2, 3, 1).contiguous(), "in", name="in0")
    out = place((c["B"], 3, c["H"], c["W"]), "out", name="out")
    wc, bc = w.contiguous(), b.contiguous()
    rc = _lib.lib().eamm_op_conv(0, d.data_ptr(), c["C"], None, 0, c["B"], c["H"], c["W"], 0, wc.data_ptr(), bc.data_ptr(), 3, 7, 7, 2,
                                 0, None, 0, tile_n, out.data_ptr(), 0, None, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None)
    torch.cuda.synchronize()
    return out.cpu()


def measure(name, tile_n=4002, place=None):
    """-> (max |out - float64|, output)"""
    out = launch(name, tile_n=tile_n, place=place)
    assert torch.isfinite(out).all(), "output has unwritten / non-finite elements"
    return float((out.double() - problem(name)[3]).abs().max()), out


def sha256(out):
    return hashlib.sha256(out.numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("name", list(CASES))
def test_split_accuracy_within_twice_the_fp32_kernel(name):
    err, _ = measure(name)
    print(f"{name}: max|out - f64| = {err:.4e} (parent fp32 kernel {PARENT[name]:.4e})")
    assert err <= 2.0 * PARENT[name], (name, err, PARENT[name])
    assert err <= 2e-6, (name, err)                           # the bound of tests/test_gpu_ops.py for tile code 4002


@pytest.mark.parametrize("name", list(PARENT_SHA256))
def test_fp32_form_is_bit_equal_to_the_parent(name):
    assert sha256(launch(name, tile_n=4003)) == PARENT_SHA256[name]


def window(name, bb, y, x):
    """The outputs a 7x7 filter gives pixel (y, x) of frame bb a share in: rows y-3 .. y+3 x columns x-3 .. x+3 of all three channels."""
    c = CASES[name]
    expect = torch.zeros(c["B"], 3, c["H"], c["W"], dtype=torch.bool)
    expect[bb, :, max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = True
    return expect


# an interior pixel on a tile boundary in both directions: last row / first column of a tile
NON_FINITE_AT = [("one_tile_row", 0, 15, 16), ("ragged", 1, 15, 16)]


@pytest.mark.parametrize("name,bb,y,x", NON_FINITE_AT)
def test_a_nan_input_reaches_exactly_its_7x7_window(name, bb, y, x):
    xin = problem(name)[0].clone()
    xin[bb, 7, y, x] = float("nan")
    for tile_n in (4002, 4003):
        assert torch.equal(torch.isnan(launch(name, x=xin, tile_n=tile_n)), window(name, bb, y, x)), tile_n


@pytest.mark.parametrize("name,bb,y,x", NON_FINITE_AT)
def test_an_inf_input_is_nan_in_the_split_form(name, bb, y, x):
    """inf splits into inf + NaN + NaN, so the split form gives NaN over the window; the fp32 form carries +-inf into the
    sigmoid and stores 0 or 1 there."""
    xin = problem(name)[0].clone()
    xin[bb, 40 % CASES[name]["C"], y, x] = float("inf")
    assert torch.equal(torch.isnan(launch(name, x=xin, tile_n=4002)), window(name, bb, y, x))
    fp32 = launch(name, x=xin, tile_n=4003)
    assert torch.isfinite(fp32).all()
    assert bool(((fp32 == 0) | (fp32 == 1))[window(name, bb, y, x)].all())


@pytest.mark.parametrize("name", ["one_tile_row", "more_rows_than_workgroups"])
def test_split_is_deterministic(name):
    first = launch(name)
    assert torch.equal(launch(name), first)
