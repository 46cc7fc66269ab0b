#!/usr/bin/env python
"""Cost of the emotion video's preprocessing (eamm_amd.video_input) on MI355X: one JSON line (also written with --out, e.g.
profiles/video_input_bench.json) with
  * per-frame device time of each kernel (HIP events over --iters back-to-back calls of --frames frames, after warm-up):
    resize_512_us (eamm_op_resize_aa, 512 x 512 -> 256 x 256), align_256_us / align_512_us (eamm_op_similarity_warp after it),
    augment_us (eamm_op_emotion_augment, one output frame);
  * host_oracle_ms_per_frame: the numpy oracle of S0..S6 for one 512 x 512 frame on this process's host CPUs;
  * e2e: a streamed animate_from_audio of a --steps clip with emotion_frames = EmotionVideo(...) against the same call with the
    materialised device tensor (one warm-up and two timed calls each, same session).
Under rocprofv3 pass --no-e2e.
Usage: python tools/video_input_bench.py [--steps T] [--frames N] [--iters K] [--no-e2e] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eamm_amd import (AudioFeatureNet, EmotionDetector, EmotionVideo, animate_from_audio, emotion_detector_config)  # noqa: E402
from eamm_amd import video_input as vi  # noqa: E402
from eamm_amd.weights import (audio_feature_state_dict_spec, emotion_state_dict_spec, synthetic_state_dict)  # noqa: E402


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


def frames(n, side, seed=0):
    rs = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    base = 0.5 + 0.3 * np.sin(2 * np.pi * 5 * x)[..., None] * np.cos(2 * np.pi * 3 * y)[..., None]
    return np.clip(base[None] + 0.1 * rs.standard_normal((n, side, side, 3)), 0, 1).__mul__(255).astype(np.uint8)


def landmarks(n, scale, seed=1):
    rs = np.random.RandomState(seed)
    base = rs.uniform(60, 196, (68, 2))
    out = []
    for _ in range(n):
        th, s, t = rs.uniform(-0.1, 0.1), rs.uniform(0.95, 1.05), rs.uniform(-5, 5, 2)
        R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        out.append((base - 128) @ (s * R).T + 128 + t)
    return np.stack(out) * scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, N = "cuda:0", args.frames
    res = {"metric": "video_input", "frames": N, "iters": args.iters}
    f256 = torch.from_numpy(frames(N, 256)).to(dev)
    f512 = torch.from_numpy(frames(N, 512)).to(dev)
    lm = landmarks(N, 1.0)
    maps = vi.alignment_maps(lm)
    r512 = vi._resize_device(f512)
    res["resize_512_us"] = round(event_us(lambda: vi._resize_device(f512), args.iters) / N, 3)
    res["align_256_us"] = round(event_us(lambda: vi._warp_device(f256, maps, 0), args.iters) / N, 3)
    res["align_512_us"] = round(res["resize_512_us"] + event_us(lambda: vi._warp_device(r512, maps, 0), args.iters) / N, 3)
    ev = EmotionVideo(f256, lm, seed=1, device=dev)
    res["augment_us"] = round(event_us(lambda: ev[0:N], args.iters) / N, 3)
    res["align_plus_augment_256_us"] = round(res["align_256_us"] + res["augment_us"], 3)
    host = frames(1, 512, seed=3)
    t0 = time.perf_counter()
    vi.emotion_video_reference(host, landmarks(1, 2.0), seed=1)
    res["host_oracle_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["host_cpus"] = len(os.sched_getaffinity(0))
    if not args.no_e2e:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_gpu_pipeline import build
        _, _, _, _, _, _, _, (gen, kpd, _, kpa) = build()
        net = AudioFeatureNet()
        net.load_state_dict(synthetic_state_dict(None, seed=2468, spec=audio_feature_state_dict_spec()), strict=True)
        net = net.to(dev).eval()
        cfg_e = emotion_detector_config()
        emo = EmotionDetector(**cfg_e)
        emo.load_state_dict(synthetic_state_dict(cfg_e, seed=4321, spec=emotion_state_dict_spec(cfg_e)), strict=True)
        emo = emo.to(dev).eval()
        T = args.steps
        S = (T + 6) * 4 * 160 + 400 - 2 * 1920
        t = np.arange(S) / 16000.0
        wave = (0.3 * np.sin(2 * np.pi * 150 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.5 * t))).astype(np.float32)
        pose = np.random.RandomState(3).uniform(-0.3, 0.3, (300, 7))
        src = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(1))
        mat = ev.materialize(T)

        def wall(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / 2
        run = lambda e: animate_from_audio(gen, kpd, net, kpa, src, wave, pose, stream=True, emo_detector=emo, emotion_frames=e)
        pre = wall(lambda: run(mat))
        lazy = wall(lambda: run(ev))
        pre2 = wall(lambda: run(mat))
        res["steps"] = T
        res["e2e_materialized_frames_per_s"] = [round(T / pre, 1), round(T / pre2, 1)]
        res["e2e_emotion_video_frames_per_s"] = round(T / lazy, 1)
        res["e2e_emotion_video_vs_materialized"] = round(min(pre, pre2) / lazy, 4)
    res["targets"] = {"align_plus_augment_us<=5": res["align_plus_augment_256_us"] <= 5.0}
    if "e2e_emotion_video_vs_materialized" in res:
        res["targets"]["e2e_ratio>=0.97"] = res["e2e_emotion_video_vs_materialized"] >= 0.97
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
