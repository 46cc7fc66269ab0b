#!/usr/bin/env python
"""Training-path timings of the key-point detectors (HIP events, median after warm-up):
1. ``kp_ops.kp_head`` forward + backward at the shape TrainPart1Model calls the heads on (16 frames x batch 8 = [128,64,64,64],
   K = 10), against the same expression as torch-ROCm ops with ATen autograd;
2. one ``KPDetector`` step (forward + backward) on 8 x 256^2.
Prints the lines kept in profiles/kp_train_step.txt."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eamm_amd import KPDetector, kp_detector_config, kp_ops
from eamm_amd.weights import kp_state_dict_spec, synthetic_source, synthetic_state_dict

REPS, WARM = 30, 5


def median_ms(step):
    for _ in range(WARM):
        step()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0]


def aten_head(logits, K, njm, pad, temperature):
    """reference keypoint_detector.py:86-103 after the convolutions, on the same NHWC logits"""
    b, h, w, _ = logits.shape
    off = 3 - pad
    win = logits[:, off:h - off, off:w - off]
    hh, ww = win.shape[1:3]
    heat = torch.softmax(win[..., :K].permute(0, 3, 1, 2).reshape(b, K, -1) / temperature, dim=2).view(b, K, hh, ww)
    xs = 2 * (torch.arange(ww, device=logits.device).float() / (ww - 1)) - 1
    ys = 2 * (torch.arange(hh, device=logits.device).float() / (hh - 1)) - 1
    grid = torch.stack([xs[None, :].expand(hh, ww), ys[:, None].expand(hh, ww)], dim=2)
    jm = win[..., K:K + 4 * njm].permute(0, 3, 1, 2).reshape(b, njm, 4, hh, ww)
    return {"value": (heat[..., None] * grid[None, None]).sum(dim=(2, 3)), "heatmap": heat,
            "jacobian": (heat[:, :, None] * jm).reshape(b, K, 4, -1).sum(dim=-1).view(b, K, 2, 2)}


B, H, W, CS, K = 128, 64, 64, 64, 10
g = torch.Generator().manual_seed(0)
logits = torch.randn(B, H, W, CS, generator=g).cuda()
logits[..., :K] *= 0.05
logits.requires_grad_()
wts = {"value": torch.randn(B, K, 2, generator=g).cuda(), "jacobian": torch.randn(B, K, 2, 2, generator=g).cuda(),
       "heatmap": torch.randn(B, K, H - 6, W - 6, generator=g).cuda()}
for name, fn in (("HIP operator (kp_ops.kp_head)", lambda: kp_ops.kp_head(logits, K, K, 0, 0.1)), ("torch-ROCm ops + ATen autograd", lambda: aten_head(logits, K, K, 0, 0.1))):
    for keys in (("value", "jacobian"), ("value", "jacobian", "heatmap")):
        def step():
            logits.grad = None
            out = fn()
            sum((out[k] * wts[k]).sum() for k in keys).backward()
        med, best = median_ms(step)
        print(f"kp_head forward + backward [{B},{H},{W},{CS}] K={K}, loss on {'+'.join(keys)}: {name}: {med:.3f} ms (median of {REPS}; best {best:.3f})")

cfg = kp_detector_config()
det = KPDetector(**cfg)
det.load_state_dict(synthetic_state_dict(cfg, seed=77, spec=kp_state_dict_spec(cfg)))
det = det.cuda().train().requires_grad_(True)
x = synthetic_source(256, seed=3, batch=8).cuda()
wd = None


def det_step():
    global wd
    det.zero_grad(set_to_none=True)
    out = det(x)
    if wd is None:
        wd = {k: torch.randn(v.shape, generator=g).cuda() for k, v in out.items()}
    sum((out[k] * wd[k]).sum() for k in out).backward()


med, best = median_ms(det_step)
print(f"KPDetector step (forward + backward, .train()) on 8 x 256^2: {med:.3f} ms (median of {REPS}; best {best:.3f})")
