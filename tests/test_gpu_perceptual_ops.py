"""The perceptual loss's operators one by one (eamm_amd/perceptual_ops.py; csrc/perceptual.hip) against float64 torch on the CPU:
``vgg_input`` (pyramid level + normalisation + conv1_1's layout), ``relu_pool``, ``l1_pair``, the frozen convolution on the tiny deep
maps VGG19 ends in, and conv1_1's four-channel data gradient.  Bars: ``closeness.close`` -- 4 x ATen's own fp32 distance from
float64, at least 2e-5 of the tensor's largest value."""
import pytest
import torch
import torch.nn.functional as F

from eamm_amd import perceptual_ops as P
from eamm_amd.weights import antialias_kernel
from closeness import close
from perceptual_common import _MEAN, _STD, ref_level

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- vgg_input ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, inv", [((2, 3, 40, 24), 1), ((2, 3, 40, 24), 2), ((2, 3, 40, 24), 4), ((2, 3, 40, 24), 8),
                                        ((1, 3, 16, 48), 2)])
def test_vgg_input_forward_and_backward(shape, inv):
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(3))
    b, _, hh, ww = shape
    r = rnd(b, hh // inv, ww // inv, 32, seed=4)
    mean, std, k = torch.tensor(_MEAN), torch.tensor(_STD), antialias_kernel(3)
    want = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()
        norm = ((ref_level(xr, inv) - mean.to(dt).reshape(1, 3, 1, 1)) / std.to(dt).reshape(1, 3, 1, 1)).permute(0, 2, 3, 1)
        (norm * r[..., :3].to(dt)).sum().backward()
        want[dt] = (norm.detach(), xr.grad)
    xg = x.to(DEV).requires_grad_()
    (out,) = P.vgg_input(xg, k.to(DEV), mean.to(DEV), std.to(DEV), (inv,))
    assert tuple(out.shape) == (b, hh // inv, ww // inv, 32)
    assert int(torch.count_nonzero(out[..., 3:])) == 0                       # exact zeros in channels 3..31
    close(out[..., :3], want[torch.float64][0], want[torch.float32][0], f"vgg_input {shape} 1/{inv}")
    (out * r.to(DEV)).sum().backward()                                       # (channels 3..31 of the gradient are not read)
    close(xg.grad, want[torch.float64][1], want[torch.float32][1], f"vgg_input backward {shape} 1/{inv}")
    # the un-normalised NCHW level is bit for bit what gets normalised: mean 0 / std 1 leaves it as it is
    (level,) = P.pyramid_levels(x.to(DEV), k.to(DEV), (inv,))
    (plain,) = P.vgg_input(x.to(DEV), k.to(DEV), torch.zeros(3, device=DEV), torch.ones(3, device=DEV), (inv,))
    assert tuple(level.shape) == (b, 3, hh // inv, ww // inv) and torch.equal(level, plain[..., :3].permute(0, 3, 1, 2))
    close(level, ref_level(x.double(), inv), ref_level(x, inv), f"level {shape} 1/{inv}")


def test_pyramid_levels_are_one_node_and_their_gradients_add_up():
    x = torch.rand(2, 3, 40, 24, generator=torch.Generator().manual_seed(5))
    k = antialias_kernel(3)
    rs = [rnd(2, 3, 40 // i, 24 // i, seed=i) for i in (2, 4, 8)]
    want = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()
        sum((ref_level(xr, i) * r.to(dt)).sum() for i, r in zip((2, 4, 8), rs)).backward()
        want[dt] = xr.grad
    xg = x.to(DEV).requires_grad_()
    levels = P.pyramid_levels(xg, k.to(DEV), (2, 4, 8))
    assert levels[0].grad_fn is levels[2].grad_fn
    sum((lv * r.to(DEV)).sum() for lv, r in zip(levels, rs)).backward()
    close(xg.grad, want[torch.float64], want[torch.float32], "pyramid backward, three levels")


# ---- relu_pool ---------------------------------------------------------------------------------------------------------------
def planted(shape, seed):
    """Random values with exact zeros, ties between equal positives (one window of four), and a window with nothing positive."""
    x = rnd(*shape, seed=seed)
    b, h, w, c = shape
    x[0, 0, 0, : c // 2] = 0.0
    if h >= 2 and w >= 2:
        x[0, 0:2, 0:2, c // 2:] = 0.75                       # four equal positives: the first takes the pooled gradient
        x[-1, 0, 0:2, 0:8] = 1.5                             # a tie in the top row
        x[-1, 1, 0:2, 0:8] = -1.0
    if h >= 4 and w >= 4:
        x[0, 2:4, 2:4, :] = -x[0, 2:4, 2:4, :].abs()         # nothing positive: a tie at zero after the ReLU, killed by the mask
        x[0, 2, 3, 0:4] = 0.0
        x[0, 3, 2, 4:8] = 2.0
        x[0, 3, 3, 4:8] = 2.0                                # a tie in the bottom row
    return x


@pytest.mark.parametrize("mode", ["dy", "dp", "both"])
@pytest.mark.parametrize("shape", [(2, 6, 10, 64), (1, 7, 5, 32)])
def test_relu_pool(shape, mode):
    x = planted(shape, seed=6)
    b, h, w, c = shape
    ry, rp = rnd(*shape, seed=7), rnd(b, h // 2, w // 2, c, seed=8)
    want = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()
        y = F.relu(xr)
        p = F.max_pool2d(y.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        loss = (y * ry.to(dt)).sum() * (mode != "dp") + (p * rp.to(dt)).sum() * (mode != "dy")
        loss.backward()
        want[dt] = (y.detach(), p.detach(), xr.grad)
    xg = x.to(DEV).requires_grad_()
    y, p = P.relu_pool(xg * 1.0, True)
    assert tuple(p.shape) == (b, h // 2, w // 2, c)
    assert torch.equal(y.cpu(), want[torch.float32][0]) and torch.equal(p.cpu(), want[torch.float32][1])    # exact: no arithmetic
    loss = None
    if mode != "dp":
        loss = (y * ry.to(DEV)).sum()
    if mode != "dy":
        loss = (p * rp.to(DEV)).sum() + (0 if loss is None else loss)
    loss.backward()
    close(xg.grad, want[torch.float64][2], want[torch.float32][2], f"relu_pool backward {shape} {mode}")


def test_relu_without_pool_and_a_map_with_no_window():
    shape = (3, 1, 3, 96)
    x, ry = planted(shape, seed=9), rnd(*shape, seed=10)
    xr = x.double().requires_grad_()
    (F.relu(xr) * ry.double()).sum().backward()
    xg = x.to(DEV).requires_grad_()
    y = P.relu_pool(xg * 1.0, False)
    assert torch.equal(y.cpu(), F.relu(x))
    (y * ry.to(DEV)).sum().backward()
    assert torch.equal(xg.grad.cpu(), xr.grad.float())
    # H // 2 == 0: torch refuses the pooled form of this map, and so does the operator, by name
    with pytest.raises(RuntimeError):
        F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2)
    with pytest.raises(ValueError, match="relu_pool: a 1 x 3 map has no 2 x 2 pooling window"):
        P.relu_pool(x.to(DEV), True)
    with pytest.raises(ValueError, match="multiple of 32"):
        P.relu_pool(torch.zeros(1, 4, 4, 48, device=DEV), True)


# ---- l1_pair -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7, 11), (1100003,), (2, 3, 5, 64)])
def test_l1_pair(shape):
    """1155 elements: two workgroups and a tail of three behind the last float4; 1100003: beyond the capped grid, so the threads
    stride; [2,3,5,64] read through an NCHW view, as Vgg19 returns its taps."""
    a, b = rnd(*shape, seed=12), rnd(*shape, seed=13)
    a.reshape(-1)[::7] = b.reshape(-1)[::7]                       # planted a == b: sign(0) = 0
    w, n = 10.0, a.numel()
    want64 = w * (a.double() - b.double()).abs().mean()
    want32 = w * (a - b).abs().mean()
    g64 = (w / n) * torch.sign(a.double() - b.double())
    ag, bg = a.to(DEV).requires_grad_(), b.to(DEV)
    av, bv = (ag.permute(0, 3, 1, 2), bg.permute(0, 3, 1, 2)) if shape == (2, 3, 5, 64) else (ag, bg)
    value = P.l1_pair(av, bv, w)
    assert value.dim() == 0
    err, bar = abs(float(value) - float(want64)), max(4 * abs(float(want32) - float(want64)), 2e-5 * abs(float(want64)))
    print(f"  l1_pair {shape}: value err {err:.2e} bar {bar:.2e}")
    assert err <= bar
    (value * 3.0).backward()
    close(ag.grad, 3.0 * g64, (3.0 * g64).float(), f"l1_pair gradient {shape}")
    assert int(torch.count_nonzero(ag.grad.reshape(-1)[::7])) == 0
    again = P.l1_pair(av.detach(), bv, w)                         # fixed-order sum: the same bits on every run
    assert torch.equal(value.detach(), again)
    with pytest.raises(ValueError, match="one non-empty shape"):
        P.l1_pair(ag, bg.reshape(-1)[:5], w)


# ---- the frozen convolution on VGG19's tiny deep maps, and conv1_1's four-channel data gradient ------------------------------------
@pytest.mark.parametrize("shape, cout", [((1, 1, 1, 512), 512), ((2, 2, 3, 512), 512), ((1, 16, 24, 32), 64)])
def test_frozen_conv(shape, cout):
    b, h, w, cin = shape
    x, r = rnd(*shape, seed=14), rnd(b, h, w, cout, seed=15)
    wt, bias = rnd(cout, cin, 3, 3, seed=16) * (2.0 / (9 * cin)) ** 0.5, 0.05 * rnd(cout, seed=17)
    want = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()
        y = F.conv2d(xr.permute(0, 3, 1, 2), wt.to(dt), bias.to(dt), padding=1).permute(0, 2, 3, 1)
        (y * r.to(dt)).sum().backward()
        want[dt] = (y.detach(), xr.grad)
    xg = x.to(DEV).requires_grad_()
    y = P.frozen_conv3x3(xg, wt.to(DEV), bias.to(DEV))
    close(y, want[torch.float64][0], want[torch.float32][0], f"frozen conv {shape} -> {cout}")
    (y * r.to(DEV)).sum().backward()
    close(xg.grad, want[torch.float64][1], want[torch.float32][1], f"frozen conv data gradient {shape} -> {cout}")
    with pytest.raises(ValueError, match="must not require a gradient"):
        P.frozen_conv3x3(xg, wt.to(DEV).requires_grad_(), bias.to(DEV))


@pytest.mark.parametrize("inv", [1, 2])
def test_stem_four_channel_data_gradient_against_the_padded_form(inv):
    """vgg_stem (transposed call with Cout = 4) against vgg_input -> frozen_conv3x3 on the 32-channel padded filter, and float64."""
    x = torch.rand(2, 3, 20, 24, generator=torch.Generator().manual_seed(18))
    w3, bias, r = rnd(64, 3, 3, 3, seed=19) * (2.0 / 27) ** 0.5, 0.05 * rnd(64, seed=20), rnd(2, 20 // inv, 24 // inv, 64, seed=21)
    mean, std, k = torch.tensor(_MEAN), torch.tensor(_STD), antialias_kernel(3)
    want = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()
        norm = (ref_level(xr, inv) - mean.to(dt).reshape(1, 3, 1, 1)) / std.to(dt).reshape(1, 3, 1, 1)
        y = F.conv2d(norm, w3.to(dt), bias.to(dt), padding=1).permute(0, 2, 3, 1)
        (y * r.to(dt)).sum().backward()
        want[dt] = (y.detach(), xr.grad)
    w32 = F.pad(w3, (0, 0, 0, 0, 0, 29)).to(DEV)
    grads = []
    for stem in (True, False):
        xg = x.to(DEV).requires_grad_()
        if stem:
            (y,) = P.vgg_stem(xg, k.to(DEV), mean.to(DEV), std.to(DEV), w32, bias.to(DEV), (inv,))
        else:
            y = P.frozen_conv3x3(P.vgg_input(xg, k.to(DEV), mean.to(DEV), std.to(DEV), (inv,))[0], w32, bias.to(DEV))
        close(y, want[torch.float64][0], want[torch.float32][0], f"conv1_1 1/{inv} {'stem' if stem else 'padded'}")
        (y * r.to(DEV)).sum().backward()
        close(xg.grad, want[torch.float64][1], want[torch.float32][1], f"conv1_1 image gradient 1/{inv} {'stem' if stem else 'padded'}")
        grads.append(xg.grad)
    close(grads[0], grads[1].double(), grads[1], "four-channel against padded")
