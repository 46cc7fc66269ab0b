#!/usr/bin/env python
"""The equivariance constraint for 8 frames at 256x256 with the shipped ``transform_params`` (sigma_affine 0.05, sigma_tps 0.005,
points_tps 5):

* frame  ``Transform.transform_frame`` alone (derived: 12.6 MB moved, 13.1 M logf);
* loss   the whole ``equivariance_loss`` (both weights 10), forward + backward, through the shipped-size ``KPDetector`` in ``.train()``:
         the detector on the driving frames, the frame warp, the detector on the warped frames, both terms, backward to the
         detector's parameters.

``eamm_amd`` beside the SAME computation written on torch-ROCm's own operators on the same GPU in the same process with the same
parameters: the reference's ``Transform`` (matmul, the [B, H W, P^2] distance tensor, ``F.grid_sample(padding_mode='reflection')``,
the jacobian by ``autograd.grad(create_graph=True)``) and its two loss terms (``torch.matmul``, a closed-form 2x2 inverse,
``abs().mean()``).  The ATen composition is the yardstick, the code under test is never its own baseline.  In the loss leg the
detector is this library's ``KPDetector`` on BOTH sides -- there is no ATen detector to race, and it is not what this tool measures
-- so that leg's difference is the transform's and the loss terms' alone.  HIP events, 3 warm-up iterations, median of 20.  There is
no pass mark.  ``--only ours|aten``, ``--leg frame|loss`` and ``--iters N`` run a part alone (for a kernel trace).  Prints the lines
kept in profiles/equivariance_step.txt."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eamm_amd import KPDetector, Transform, equivariance_loss, kp_detector_config
from eamm_amd.weights import kp_state_dict_spec, synthetic_source, synthetic_state_dict

WARM, REPS = 3, 20
SIGMA_AFFINE, SIGMA_TPS, POINTS = 0.05, 0.005, 5
WEIGHT = 10.0


def grid_of(h, w, device):
    x = 2 * (torch.arange(w, dtype=torch.float32, device=device) / (w - 1)) - 1
    y = 2 * (torch.arange(h, dtype=torch.float32, device=device) / (h - 1)) - 1
    return torch.stack([x.view(1, -1).repeat(h, 1), y.view(-1, 1).repeat(1, w)], dim=2)


class AtenTransform:
    """The reference's Transform on torch's own operators, with given parameters."""

    def __init__(self, theta, control_params, points):
        self.theta, self.control_params, self.bs = theta, control_params, theta.shape[0]
        self.control_points = grid_of(points, points, theta.device).view(1, 1, -1, 2)

    def warp_coordinates(self, c):
        theta = self.theta.unsqueeze(1)
        out = (torch.matmul(theta[:, :, :, :2], c.unsqueeze(-1)) + theta[:, :, :, 2:]).squeeze(-1)
        d = (c.view(c.shape[0], -1, 1, 2) - self.control_points).abs().sum(-1)
        r = (d ** 2 * torch.log(d + 1e-6) * self.control_params).sum(dim=2).view(self.bs, c.shape[1], 1)
        return out + r

    def transform_frame(self, frame):
        h, w = frame.shape[2:]
        grid = self.warp_coordinates(grid_of(h, w, frame.device).view(1, h * w, 2)).view(self.bs, h, w, 2)
        return F.grid_sample(frame, grid, padding_mode="reflection", align_corners=False)

    def jacobian(self, c):
        new = self.warp_coordinates(c)
        gx = torch.autograd.grad(new[..., 0].sum(), c, create_graph=True)[0]
        gy = torch.autograd.grad(new[..., 1].sum(), c, create_graph=True)[0]
        return torch.cat([gx.unsqueeze(-2), gy.unsqueeze(-2)], dim=-2)


def aten_inverse2(m):
    a, b, c, d = m[..., 0, 0], m[..., 0, 1], m[..., 1, 0], m[..., 1, 1]
    det = a * d - b * c
    return torch.stack([d / det, -b / det, -c / det, a / det], dim=-1).view(*m.shape[:-2], 2, 2)


def aten_loss(det, driving, kp_driving, t):
    frame = t.transform_frame(driving)
    kp = det(frame)
    value = WEIGHT * (kp_driving["value"] - t.warp_coordinates(kp["value"])).abs().mean()
    product = torch.matmul(aten_inverse2(kp_driving["jacobian"]), torch.matmul(t.jacobian(kp["value"]), kp["jacobian"]))
    eye = torch.eye(2, device=product.device).view(1, 1, 2, 2)
    return value + WEIGHT * (eye - product).abs().mean()


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
    ap.add_argument("--leg", choices=("frame", "loss"))
    ap.add_argument("--iters", type=int, default=REPS)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ours_t = Transform(a.frames, SIGMA_AFFINE, SIGMA_TPS, POINTS, device=dev)
    aten_t = AtenTransform(ours_t.theta, ours_t.control_params, POINTS)
    driving = synthetic_source(a.size, seed=3, batch=a.frames).to(dev)
    cfg = kp_detector_config()
    det = KPDetector(**cfg)
    det.load_state_dict(synthetic_state_dict(cfg, seed=77, spec=kp_state_dict_spec(cfg)))
    det = det.to(dev).requires_grad_(True).train()
    values = {}

    def ours_frame():
        values["ours", "frame"] = ours_t.transform_frame(driving)

    def aten_frame():
        values["aten", "frame"] = aten_t.transform_frame(driving)

    def ours_loss():
        det.zero_grad(set_to_none=True)
        v, _ = equivariance_loss(det, driving, det(driving), ours_t, WEIGHT, WEIGHT)
        loss = v["equivariance_value"] + v["equivariance_jacobian"]
        loss.backward()
        values["ours", "loss"] = loss.detach()

    def aten_loss_step():
        det.zero_grad(set_to_none=True)
        loss = aten_loss(det, driving, det(driving), aten_t)
        loss.backward()
        values["aten", "loss"] = loss.detach()

    steps = {("ours", "frame"): ours_frame, ("aten", "frame"): aten_frame, ("ours", "loss"): ours_loss, ("aten", "loss"): aten_loss_step}
    names = {"ours": "eamm_amd", "aten": "ATen composition (matmul / distance tensor / grid_sample / autograd.grad)"}
    legs = {"frame": "transform_frame", "loss": "equivariance_loss forward + backward through KPDetector (.train())"}
    what = f"{a.frames} frames at {a.size}x{a.size}, points_tps {POINTS}"
    res = {}
    for leg in ("frame", "loss"):
        if a.leg not in (None, leg):
            continue
        for name in ("ours", "aten"):
            if a.only not in (None, name):
                continue
            res[name, leg] = median_ms(steps[name, leg], WARM, a.iters)
            v = values[name, leg]
            shown = f"loss {float(v):.6f}" if leg == "loss" else f"mean {float(v.mean()):.6f}"
            print(f"{names[name]:76s} {legs[leg]}, {what}: {res[name, leg][0]:8.3f} ms (median of {a.iters} after {WARM} warm-up; "
                  f"best {res[name, leg][1]:.3f}); {shown}")
        if ("ours", leg) in res and ("aten", leg) in res:
            if leg == "frame":
                print(f"frame: largest difference between the two results {float((values['ours', leg] - values['aten', leg]).abs().max()):.2e}")
            ratio = res["ours", leg][0] / res["aten", leg][0]
            print(f"{leg}: eamm_amd / ATen = {ratio:.4f} x the time ({1 / ratio:.1f} x faster)" if ratio < 1 else
                  f"{leg}: eamm_amd / ATen = {ratio:.2f} x the time")
        if ("ours", leg) in res and leg == "frame":
            moved = 2 * driving.numel() * 4 / 1e6
            print(f"frame: {moved:.1f} MB moved (derived) in {res['ours', leg][0]:.3f} ms of call time (launch included) = "
                  f"{moved / res['ours', leg][0]:.0f} GB/s")


if __name__ == "__main__":
    main()
