"""What the perceptual-loss tests share: the seeded inputs and weights of their recipe, the float64 / ATen-fp32 oracle on the CPU
(plain torch: F.pad / F.conv2d / F.relu / F.max_pool2d).  The tolerance rules are tests/closeness.py's.

Recipe: ``generated`` uniform [0,1), ``real = clamp(generated + 0.1 randn, 0, 1)``, He-normal filters (std = sqrt(2 / (9 Cin))),
biases 0.05 randn, everything rounded to fp32 before the float64 oracle sees it -- both sides read identical values."""
import math

import torch
import torch.nn.functional as F

from eamm_amd.perceptual import _CONVS, _MEAN, _POOLS, _SLICES, _STD
from eamm_amd.weights import antialias_kernel

def vgg_state(seed=7):
    """A Vgg19 state dict in the reference module's layout, fp32."""
    g = torch.Generator().manual_seed(seed)
    sd = {"mean": torch.tensor(_MEAN).reshape(1, 3, 1, 1), "std": torch.tensor(_STD).reshape(1, 3, 1, 1)}
    for i, (cin, cout) in _CONVS.items():
        s = next(n for n, (lo, hi) in enumerate(_SLICES, 1) if lo <= i < hi)
        sd[f"slice{s}.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"slice{s}.{i}.bias"] = 0.05 * torch.randn(cout, generator=g)
    return sd


def image_pair(shape, seed=11):
    g = torch.Generator().manual_seed(seed)
    generated = torch.rand(*shape, generator=g)
    real = (generated + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return generated, real


def ref_level(x, inv):
    """AntiAliasInterpolation2d (reference modules/util.py:1044-1052) in x's dtype."""
    if inv == 1:
        return x
    k = antialias_kernel(3).to(x.dtype)
    return F.conv2d(F.pad(x, (6, 6, 6, 6)), k, groups=3)[:, :, ::inv, ::inv]


def ref_vgg(sd, x, taps=5):
    """Reference Vgg19.forward (modules/model.py:42-50) in x's dtype; NCHW taps."""
    dt = x.dtype
    h = (x - sd["mean"].to(dt)) / sd["std"].to(dt)
    out = []
    for s, (lo, hi) in enumerate(_SLICES[:taps], 1):
        for i in range(lo, hi):
            if i in _CONVS:
                h = F.conv2d(h, sd[f"slice{s}.{i}.weight"].to(dt), sd[f"slice{s}.{i}.bias"].to(dt), padding=1)
            elif i in _POOLS:
                h = F.max_pool2d(h, 2, 2)
            else:
                h = F.relu(h)
        out.append(h)
    return out


def ref_loss(sd, generated, real, scales, weights):
    """modules/model.py:239-248 in generated's dtype."""
    taps = max(i for i, w in enumerate(weights) if w) + 1
    total = 0
    for scale in scales:
        inv = int(round(1 / scale))
        fg = ref_vgg(sd, ref_level(generated, inv), taps)
        with torch.no_grad():
            fr = ref_vgg(sd, ref_level(real, inv), taps)
        for i in range(taps):
            if weights[i]:
                total = total + weights[i] * (fg[i] - fr[i]).abs().mean()
    return total


FRAGILE_REL = 1e-6   # about 8 fp32 ulps


def fragile_decisions(sd, x, rel=FRAGILE_REL):
    """How many discrete decisions of Vgg19 on ``x`` (float64) an fp32 forward may take the other way: pre-activations within
    ``rel`` x the layer's largest value of zero, and max-pool windows whose two largest values lie within ``rel`` of each other
    (relative).  The gradient is discontinuous there -- the whole receptive field of the unit moves, by a few per cent of the image
    gradient's scale when the unit is deep -- so at such an input the float64 gradient is one of two equally valid answers and
    no oracle.  The tests draw their images from the first seed at which this is zero (a property of the oracle alone)."""
    dt = torch.float64
    s = {k: v.to(dt) for k, v in sd.items()}
    with torch.no_grad():
        h = (x.to(dt) - s["mean"]) / s["std"]
        count = 0
        for sl, (lo, hi) in enumerate(_SLICES, 1):
            for i in range(lo, hi):
                if i in _CONVS:
                    h = F.conv2d(h, s[f"slice{sl}.{i}.weight"], s[f"slice{sl}.{i}.bias"], padding=1)
                    count += int((h.abs() < rel * h.abs().max()).sum())
                elif i in _POOLS:
                    b, c, hh, ww = h.shape
                    win = h[:, :, :hh // 2 * 2, :ww // 2 * 2].reshape(b, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, hh // 2, ww // 2, 4)
                    top = win.topk(2, dim=-1).values
                    count += int(((top[..., 0] > 0) & (top[..., 0] - top[..., 1] < rel * top[..., 0])).sum())
                    h = F.max_pool2d(h, 2, 2)
                else:
                    h = F.relu(h)
    return count
