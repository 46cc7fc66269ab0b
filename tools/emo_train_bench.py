#!/usr/bin/env python
"""Training-path timings of the emotion detector (HIP events, median after warm-up):
1. each stride-2 entry (``eamm_op_conv_s2``, ``_dgrad``, ``_wgrad``) at the shapes of Emotion_k's trunk on 16 x 256^2 -- the first 3x3
   of layer2 / layer3 / layer4 and their 1x1 shortcuts: time, executed FLOP (``eamm_total_mfma_flops``: what the grids issue, padded
   tiles included) against algorithmic FLOP (2 B Ho Wo Cout Cin k^2), and the algorithmic rate's share of the fp32 matrix peak;
2. one ``EmotionDetector`` step (forward + backward, ``.train()``) on 16 x 256^2.
Prints the lines kept in profiles/emo_train_step.txt.  Nothing here is tuned: the figures are what the stated forms give."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eamm_amd import EmotionDetector, _lib, emotion_detector_config
from eamm_amd.weights import emotion_state_dict_spec, synthetic_keypoints, synthetic_source, synthetic_state_dict

REPS, WARM = 30, 5
PEAK_TF = 157.3      # fp32 matrix peak of one MI355X (v_mfma_f32_32x32x2_f32)
SHAPES = [(16, 32, 32, 64, 128), (16, 16, 16, 128, 256), (16, 8, 8, 256, 512)]


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


def p(t):
    return C.c_void_p(t.data_ptr())


def main():
    L = _lib.lib()
    g = torch.Generator().manual_seed(0)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in (3, 1):
        for b, h, w, cin, cout in SHAPES:
            x = torch.randn(b, h, w, cin, generator=g).cuda()
            wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).cuda()
            gy = torch.randn(b, h // 2, w // 2, cout, generator=g).cuda()
            y, dx, dw = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(wt)
            ws = {n: torch.empty(getattr(L, f"eamm_op_conv_s2{n}_workspace_floats")(b, h, w, cin, cout, k), device="cuda") for n in ("", "_dgrad", "_wgrad")}
            calls = {
                "forward": lambda: _lib.check(L.eamm_op_conv_s2(0, p(x), b, h, w, cin, p(wt), cout, k, p(y), p(ws[""]), ws[""].numel(), st())),
                "dgrad": lambda: _lib.check(L.eamm_op_conv_s2_dgrad(0, p(gy), b, h, w, cin, p(wt), cout, k, p(dx), p(ws["_dgrad"]), ws["_dgrad"].numel(), st())),
                "wgrad": lambda: _lib.check(L.eamm_op_conv_s2_wgrad(0, p(x), p(gy), b, h, w, cin, cout, k, p(dw), p(ws["_wgrad"]), ws["_wgrad"].numel(), st())),
            }
            algo = 2.0 * b * (h // 2) * (w // 2) * cout * cin * k * k
            for name, call in calls.items():
                f0 = L.eamm_total_mfma_flops()
                call()
                executed = L.eamm_total_mfma_flops() - f0
                med, best = median_ms(call)
                print(f"conv_s2 {name:7s} {k}x{k} [{b},{h},{w},{cin}]->{cout}: {med * 1e3:8.1f} us (median of {REPS}; best {best * 1e3:.1f}); "
                      f"executed {executed / 1e9:.3f} GFLOP vs algorithmic {algo / 1e9:.3f} ({executed / algo:.2f} x); "
                      f"{algo / med / 1e9:.2f} TFLOP/s algorithmic = {100 * algo / med / 1e9 / PEAK_TF:.1f} % of the fp32 matrix peak "
                      f"(filter packing and split reduction included)")

    cfg = emotion_detector_config()
    det = EmotionDetector(**cfg)
    det.load_state_dict(synthetic_state_dict(cfg, seed=4321, spec=emotion_state_dict_spec(cfg)))
    det = det.cuda().train().requires_grad_(True)
    n = 16
    x = synthetic_source(256, seed=11, batch=n).cuda()
    kp = {k: v.cuda() for k, v in synthetic_keypoints(n, 10, seed=40).items()}
    wd = {}

    def det_step():
        det.zero_grad(set_to_none=True)
        off, fake = det(x, kp["value"], kp["jacobian"])
        out = {"value": off["value"], "jacobian": off["jacobian"], "fake": fake}
        if not wd:
            wd.update({k: torch.randn(v.shape, generator=g).cuda() for k, v in out.items()})
        sum((out[k] * wd[k]).sum() for k in out).backward()

    med, best = median_ms(det_step)
    print(f"EmotionDetector step (forward + backward, .train()) on {n} x 256^2: {med:.3f} ms (median of {REPS}; best {best:.3f})")
    det.eval().requires_grad_(False)
    with torch.no_grad():
        med, best = median_ms(lambda: det(x, kp["value"], kp["jacobian"]))
    print(f"for scale: the frozen .eval() engine's forward on the same batch: {med:.3f} ms (median of {REPS}; best {best:.3f})")


if __name__ == "__main__":
    main()
