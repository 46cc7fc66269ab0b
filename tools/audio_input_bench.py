#!/usr/bin/env python
"""Cost of the waveform front end (eamm_amd.audio_input) on MI355X: one JSON line (also written with --out, e.g.
profiles/audio_input_bench.json) with, for the waveform of a T-step clip (T = 2048: 1 311 120 samples, 81.9 s at 16 kHz, 8217
MFCC frames):
  * mfcc_kernel_us: eamm_op_mfcc on the device (HIP events over --iters back-to-back calls, after warm-up), and the same with
    the windows' strided copy (mfcc_windows);
  * host_oracle_ms: mfcc_reference (float64 numpy) of the same waveform on this process's host CPUs, best of 3;
  * e2e: animate_from_audio frames/s against animate_from_features given the precomputed windows and pose track, both streamed,
    same session (one warm-up and two timed calls each).
Under rocprofv3 pass --no-e2e (the kernel-trace stats then hold the kernel alone).
Usage: python tools/audio_input_bench.py [--steps T] [--iters N] [--no-e2e] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eamm_amd import AudioFeatureNet, animate_from_audio, animate_from_features, mfcc, mfcc_reference, mfcc_windows, prepare_pose  # noqa: E402
from eamm_amd.audio_input import DEMO_PAD, mfcc_frames  # noqa: E402
from eamm_amd.weights import audio_feature_state_dict_spec, synthetic_state_dict  # noqa: E402


def event_us(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def speech_like(S, seed=0):
    """a voiced signal with pauses and a little noise (the MFCC's cost does not depend on the content)"""
    rs = np.random.RandomState(seed)
    t = np.arange(S) / 16000.0
    x = sum(0.2 / h * np.sin(2 * np.pi * 150 * h * t) for h in range(1, 9)) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.5 * t))
    x += 0.003 * rs.standard_normal(S)
    x[(t % 3.0) > 2.4] = 0.0
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, T = "cuda:0", args.steps
    S = (T + 6) * 4 * 160 + 400 - 2 * DEMO_PAD          # F = 4 T + 25 frames: T windows
    x = speech_like(S)
    w = torch.from_numpy(x).to(dev)
    F = mfcc_frames(S)
    res = {"metric": "audio_input", "steps": T, "samples": S, "seconds": round(S / 16000.0, 2), "frames": F, "iters": args.iters}
    res["mfcc_kernel_us"] = round(event_us(lambda: mfcc(w), args.iters), 2)
    res["mfcc_windows_us"] = round(event_us(lambda: mfcc_windows(w), args.iters), 2)
    got = mfcc(w).cpu().numpy()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        ref = mfcc_reference(x)
        best = min(best, time.perf_counter() - t0)
    res["host_oracle_ms"] = round(best * 1e3, 1)
    res["host_cpus"] = len(os.sched_getaffinity(0))
    res["max_abs_vs_oracle"] = float(np.abs(got - ref).max())
    if not args.no_e2e:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_gpu_pipeline import build
        _, _, _, _, _, _, _, (gen, kpd, _, kpa) = build()
        net = AudioFeatureNet()
        net.load_state_dict(synthetic_state_dict(None, seed=2468, spec=audio_feature_state_dict_spec()), strict=True)
        net = net.to(dev).eval()
        src = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(1))
        pose = np.random.RandomState(3).uniform(-0.3, 0.3, (300, 7))
        windows = mfcc_windows(w)
        pose_t = prepare_pose(pose, T)

        def wall(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / 2
        pre = wall(lambda: animate_from_features(gen, kpd, net.decon, kpa, src, None, audio_feature=net, audio=windows, pose=pose_t,
                                                 stream=True))
        full = wall(lambda: animate_from_audio(gen, kpd, net, kpa, src, x, pose, stream=True))
        res["e2e_precomputed_windows_frames_per_s"] = round(T / pre, 1)
        res["e2e_from_waveform_frames_per_s"] = round(T / full, 1)
        res["e2e_from_waveform_vs_precomputed"] = round(pre / full, 4)
    res["targets"] = {"mfcc_kernel_ms<=0.1": res["mfcc_kernel_us"] <= 100.0}
    if "e2e_from_waveform_vs_precomputed" in res:
        res["targets"]["e2e_ratio>=0.99"] = res["e2e_from_waveform_vs_precomputed"] >= 0.99
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
