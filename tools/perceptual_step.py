#!/usr/bin/env python
"""One perceptual-loss step (forward + backward to the generated images) for 8 pairs at 256x256, four scales [1, 0.5, 0.25, 0.125],
weights [10] * 5: ``eamm_amd.PerceptualLoss`` beside the SAME loss assembled from torch-ROCm's own F.conv2d / F.max_pool2d / F.relu
on the same GPU with the same weights -- the ATen composition is the yardstick, the code under test is never its own baseline.
HIP events, 3 warm-up iterations, median of 20.  Also the achieved share of the fp32 matrix peak over the DERIVED 1.58 TFLOP per
step (8 x 197 GFLOP: both forwards and the generated half's data gradient).  There is no pass mark.
``--only ours|aten`` and ``--iters N`` run one side alone (for a kernel trace).  Prints the lines kept in profiles/perceptual_loss.txt."""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eamm_amd import PerceptualLoss, Vgg19
from eamm_amd.perceptual import _CONVS, _POOLS, _SLICES
from eamm_amd.weights import antialias_kernel

WARM, REPS = 3, 20
PEAK_TF = 157.3          # fp32 matrix peak of one MI355X (v_mfma_f32_32x32x2_f32)
STEP_TFLOP = 1.58        # derived: 8 pairs x (131 GFLOP forwards + 66 GFLOP data gradient)
SCALES, WEIGHTS = [1, 0.5, 0.25, 0.125], [10.0] * 5


def state(seed=7):
    g = torch.Generator().manual_seed(seed)
    sd = Vgg19().state_dict()
    for i, (cin, cout) in _CONVS.items():
        s = next(n for n, (lo, hi) in enumerate(_SLICES, 1) if lo <= i < hi)
        sd[f"slice{s}.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"slice{s}.{i}.bias"] = 0.05 * torch.randn(cout, generator=g)
    return sd


def aten_loss(sd, generated, real):
    """modules/model.py:239-248 on torch's own operators."""
    k = antialias_kernel(3).to(generated.device)

    def level(x, inv):
        return x if inv == 1 else F.conv2d(F.pad(x, (6, 6, 6, 6)), k, groups=3)[:, :, ::inv, ::inv]

    def vgg(x):
        h = (x - sd["mean"]) / sd["std"]
        out = []
        for s, (lo, hi) in enumerate(_SLICES, 1):
            for i in range(lo, hi):
                if i in _CONVS:
                    h = F.conv2d(h, sd[f"slice{s}.{i}.weight"], sd[f"slice{s}.{i}.bias"], padding=1)
                elif i in _POOLS:
                    h = F.max_pool2d(h, 2, 2)
                else:
                    h = F.relu(h)
            out.append(h)
        return out

    total = 0
    for scale in SCALES:
        inv = int(round(1 / scale))
        fg = vgg(level(generated, inv))
        with torch.no_grad():
            fr = vgg(level(real, inv))
        for w, a, b in zip(WEIGHTS, fg, fr):
            total = total + w * (a - b).abs().mean()
    return total


def median_ms(step, warm, reps):
    for _ in range(warm):
        step()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("ours", "aten"))
    ap.add_argument("--iters", type=int, default=REPS)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    generated = torch.rand(a.pairs, 3, a.size, a.size, generator=g)
    real = (generated + 0.1 * torch.randn(generated.shape, generator=g)).clamp(0, 1).to(dev)
    generated = generated.to(dev).requires_grad_()
    sd = state()
    vgg = Vgg19()
    vgg.load_state_dict(sd, strict=True)
    crit = PerceptualLoss(SCALES, WEIGHTS, vgg=vgg).to(dev)
    sd = {k: v.to(dev) for k, v in sd.items()}
    values = {}

    def ours():
        generated.grad = None
        loss = crit(generated, real)
        loss.backward()
        values["ours"] = loss.detach()

    def aten():
        generated.grad = None
        loss = aten_loss(sd, generated, real)
        loss.backward()
        values["aten"] = loss.detach()

    what = f"{a.pairs} pairs at {a.size}x{a.size}, scales {SCALES}"
    res = {}
    for name, step in (("ours", ours), ("aten", aten)):
        if a.only in (None, name):
            res[name] = median_ms(step, WARM, a.iters)
            grad = generated.grad.clone()
            print(f"{'eamm_amd.PerceptualLoss' if name == 'ours' else 'ATen composition (F.conv2d / F.max_pool2d / F.relu)':54s} forward + backward, "
                  f"{what}: {res[name][0]:8.3f} ms (median of {a.iters} after {WARM} warm-up; best {res[name][1]:.3f}); loss {float(values[name]):.6f}; "
                  f"|grad|max {float(grad.abs().max()):.3e}")
    if "ours" in res and a.pairs == 8 and a.size == 256:
        tf = STEP_TFLOP / (res["ours"][0] * 1e-3)
        print(f"eamm_amd: {tf:.1f} TFLOP/s over the derived {STEP_TFLOP} TFLOP per step = {100 * tf / PEAK_TF:.1f} % of the fp32 matrix peak ({PEAK_TF} TFLOP/s)")
    if len(res) == 2:
        print(f"eamm_amd / ATen = {res['ours'][0] / res['aten'][0]:.2f} x the time")


if __name__ == "__main__":
    main()
