"""eamm_op_conv_dev with a 1x1 filter (the discriminator's prediction layer: pad 0, one tap in the packed image), forward and --
``transposed = 1`` -- data gradient, against F.conv2d on the CPU in float64 at closeness.close's bar.  The cases are registered in
tests/guarded.py as ``train-conv_dev_1x1_<name>``: tests/test_gpu_guarded_ops.py runs each on plain tensors and between poisoned
bands at skew 0 and 16 (outputs bit-equal to the plain placement)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from eamm_amd import _lib, _op
from closeness import close
from guarded import case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, H, W, Cin, Cout, transposed): odd maps (raster order), an M tail, Cout off the 32-column tile, the prediction layer's widths
CASES = {"fwd_512_to_32": (2, 4, 3, 512, 32, 0), "fwd_odd_tail_cout36": (2, 5, 7, 64, 36, 0), "fwd_even_two_tiles": (1, 12, 14, 32, 64, 0),
         "dgrad_32_to_512": (2, 4, 3, 32, 512, 1), "dgrad_odd_tail": (1, 9, 15, 64, 96, 1)}


def run_case(name, place):
    b, h, w, cin, cout, transposed = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(b, h, w, cin, generator=g)
    wt = torch.randn(*((cin, cout) if transposed else (cout, cin)), 1, 1, generator=g) * math.sqrt(2.0 / cin)
    bias = None if transposed else 0.1 * torch.randn(cout, generator=g)
    want = []
    for dt in (torch.float64, torch.float32):
        xn = x.permute(0, 3, 1, 2).to(dt)
        y = F.conv_transpose2d(xn, wt.to(dt)) if transposed else F.conv2d(xn, wt.to(dt), bias.to(dt))
        want.append(y.permute(0, 2, 3, 1).contiguous())
    n = _lib.lib().eamm_op_conv_dev_workspace_floats(b, h, w, cin, cout, 1, 1)
    assert n > 0
    out = place((b, h, w, cout), "out", name="out")
    _op.call("conv_dev", torch.device(DEV), place(x, "in"), b, h, w, cin, place(wt, "in"), None if bias is None else place(bias, "in"),
             cout, 1, 1, transposed, out, work=place(n, "work"))
    close(out, want[0], want[1], "conv_dev 1x1 " + name)


for _n in sorted(CASES):
    case("train-conv_dev_1x1_" + _n, ["eamm_op_conv_dev"], functools.partial(run_case, _n))


def test_other_filter_sizes_stay_refused():
    assert _lib.lib().eamm_op_conv_dev_workspace_floats(1, 8, 8, 32, 32, 5, 5) == 0
    assert _lib.lib().eamm_op_conv_dev_workspace_floats(1, 8, 8, 32, 32, 1, 3) == 0
    assert _lib.lib().eamm_op_conv_dev_workspace_floats(1, 8, 8, 48, 32, 1, 1) == 0
