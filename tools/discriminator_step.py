#!/usr/bin/env python
"""The adversarial half of a training step for 8 pairs at 256x256 with the shipped discriminator (scales [1], block_expansion 32,
max_features 512, num_blocks 4, sn True):

* generator side      ``generator_gan_loss`` with a FROZEN discriminator: two forwards (generated, real), feature matching, backward to
                      the generated images;
* discriminator side  ``discriminator_gan_loss``: two forwards, backward to the discriminator's parameters.

``eamm_amd`` beside the SAME network and losses assembled from torch-ROCm's own operators (nn.Conv2d with torch's spectral_norm,
F.instance_norm, F.leaky_relu, F.avg_pool2d) on the same GPU in the same process with the same weights -- the ATen composition is the
yardstick, the code under test is never its own baseline.  HIP events, 3 warm-up iterations, median of 20.  Also the achieved share of
the fp32 matrix peak over the DERIVED arithmetic (10.73 GFLOP per image and forward; a data gradient costs the
same, a weight gradient too).  There is no pass mark.  ``--only ours|aten``, ``--side gen|disc`` and ``--iters N`` run a part alone
(for a kernel trace).  Prints the lines kept in profiles/discriminator_step.txt."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eamm_amd import ImagePyramide, MultiScaleDiscriminator, discriminator_gan_loss, generator_gan_loss

WARM, REPS = 3, 20
PEAK_TF = 157.3                     # fp32 matrix peak of one MI355X (v_mfma_f32_32x32x2_f32)
PARAMS = dict(scales=[1], block_expansion=32, max_features=512, num_blocks=4, sn=True)
FM = [10.0, 10.0, 10.0, 10.0]
FWD_GFLOP, FIRST_GFLOP = 10.73, 0.39            # per image: the four 4x4 convolutions; the first of them
# generator side: 2 forwards + the data gradients of one; discriminator side: 2 forwards + 2 weight gradients + 2 data gradients
# without the first layer's (the images need none)
STEP_TFLOP = {"gen": 8 * 3 * FWD_GFLOP / 1e3, "disc": 8 * (6 * FWD_GFLOP - 2 * FIRST_GFLOP) / 1e3}


class AtenDiscriminator(nn.Module):
    """The shipped discriminator on torch's own operators, with the state-dict layout of the reference."""

    def __init__(self, block_expansion=32, max_features=512, num_blocks=4):
        super().__init__()
        widths = [3] + [min(max_features, block_expansion * 2 ** (i + 1)) for i in range(num_blocks)]
        self.down_blocks = nn.ModuleList()
        for i in range(num_blocks):
            block = nn.Module()
            block.conv = nn.utils.spectral_norm(nn.Conv2d(widths[i], widths[i + 1], 4))
            if i:
                block.norm = nn.InstanceNorm2d(widths[i + 1], affine=True)
            self.down_blocks.append(block)
        self.conv = nn.utils.spectral_norm(nn.Conv2d(widths[-1], 1, 1))

    def forward(self, x):
        maps = []
        for i, block in enumerate(self.down_blocks):
            x = block.conv(x)
            if i:
                x = F.instance_norm(x, weight=block.norm.weight, bias=block.norm.bias)
            x = F.leaky_relu(x, 0.2)
            if i != len(self.down_blocks) - 1:
                x = F.avg_pool2d(x, 2)
            maps.append(x)
        return maps, self.conv(x)


def aten_gen_loss(net, generated, real):
    mg, pg = net(generated)
    mr, _ = net(real)
    total = ((1 - pg) ** 2).mean()
    for w, a, b in zip(FM, mr, mg):
        total = total + w * (a - b).abs().mean()
    return total


def aten_disc_loss(net, real, generated):
    _, pg = net(generated.detach())
    _, pr = net(real)
    return ((1 - pr) ** 2 + pg ** 2).mean()


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
    ap.add_argument("--side", choices=("gen", "disc"))
    ap.add_argument("--iters", type=int, default=REPS)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    generated = torch.rand(a.pairs, 3, a.size, a.size, generator=g)
    real = (generated + 0.1 * torch.randn(generated.shape, generator=g)).clamp(0, 1).to(dev)
    generated = generated.to(dev).requires_grad_()
    torch.manual_seed(1)
    aten = AtenDiscriminator().to(dev).train()
    ours = MultiScaleDiscriminator(**PARAMS)
    ours.load_state_dict({"discs.1." + k: v for k, v in aten.state_dict().items()}, strict=True)
    ours = ours.to(dev).train()
    pyr = ImagePyramide([1], 3).to(dev)
    values = {}

    def freeze(net, frozen):
        for p in net.parameters():
            p.requires_grad_(not frozen)
            p.grad = None

    def ours_gen():
        generated.grad = None
        v = generator_gan_loss(ours, pyr(generated), pyr(real), None, 1.0, FM)
        loss = v["gen_gan"] + v["feature_matching"]
        loss.backward()
        values["ours", "gen"] = loss.detach()

    def aten_gen():
        generated.grad = None
        loss = aten_gen_loss(aten, generated, real)
        loss.backward()
        values["aten", "gen"] = loss.detach()

    def ours_disc():
        ours.zero_grad(set_to_none=True)
        loss = discriminator_gan_loss(ours, pyr(real), pyr(generated), None, 1.0)["disc_gan"]
        loss.backward()
        values["ours", "disc"] = loss.detach()

    def aten_disc():
        aten.zero_grad(set_to_none=True)
        loss = aten_disc_loss(aten, real, generated)
        loss.backward()
        values["aten", "disc"] = loss.detach()

    steps = {("ours", "gen"): ours_gen, ("aten", "gen"): aten_gen, ("ours", "disc"): ours_disc, ("aten", "disc"): aten_disc}
    names = {"ours": "eamm_amd", "aten": "ATen composition (Conv2d / instance_norm / leaky_relu / avg_pool2d)"}
    sides = {"gen": "generator side (2 forwards, backward to the generated images, frozen discriminator)",
             "disc": "discriminator side (2 forwards, backward to the parameters)"}
    what = f"{a.pairs} pairs at {a.size}x{a.size}"
    res = {}
    for side in ("gen", "disc"):
        if a.side not in (None, side):
            continue
        for name in ("ours", "aten"):
            if a.only not in (None, name):
                continue
            freeze(ours if name == "ours" else aten, side == "gen")
            res[name, side] = median_ms(steps[name, side], WARM, a.iters)
            print(f"{names[name]:72s} {sides[side]}, {what}: {res[name, side][0]:8.3f} ms (median of {a.iters} after {WARM} warm-up; "
                  f"best {res[name, side][1]:.3f}); loss {float(values[name, side]):.6f}")
        if ("ours", side) in res and a.pairs == 8 and a.size == 256:
            tf = STEP_TFLOP[side] / (res["ours", side][0] * 1e-3)
            print(f"eamm_amd {side}: {tf:.1f} TFLOP/s over the derived {STEP_TFLOP[side]:.3f} TFLOP per step = {100 * tf / PEAK_TF:.1f} % of the "
                  f"fp32 matrix peak ({PEAK_TF} TFLOP/s)")
        if ("ours", side) in res and ("aten", side) in res:
            print(f"{side}: eamm_amd / ATen = {res['ours', side][0] / res['aten', side][0]:.2f} x the time")


if __name__ == "__main__":
    main()
