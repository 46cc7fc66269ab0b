#!/usr/bin/env python
"""Throughput of the emotion detector Emotion_k on MI355X: one JSON line with frames/s of EmotionDetector.detect at B = 16 / 64 /
256 (HIP events, warm-up, >= 50 timed calls), the executed matrix-core GFLOP per frame and the fraction of the fp32 matrix peak,
and animate_from_features on a 256x256 clip three ways: no emotion, emo_driving precomputed, emo_detector on the device.
Usage: python tools/emotion_bench.py [--iters N] [--clip-frames T] [--no-e2e]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eamm_amd import EmotionDetector, _lib, animate_from_features, emotion_detector_config  # noqa: E402
from eamm_amd.weights import emotion_state_dict_spec, synthetic_keypoints, synthetic_lstm_features, synthetic_source, synthetic_state_dict  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12


def event_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--clip-frames", type=int, default=2048)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = emotion_detector_config()
    sd = synthetic_state_dict(cfg, seed=4321, spec=emotion_state_dict_spec(cfg))
    res = {"metric": "emotion_detector", "iters": args.iters}
    L = _lib.lib()
    for B in (16, 64, 256):
        m = EmotionDetector(**cfg, max_batch=B)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        x = synthetic_source(256, seed=11, batch=B).to(dev)
        kp = {k: v.to(dev) for k, v in synthetic_keypoints(B, 10, seed=40).items()}
        call = lambda: m.detect(x, kp["value"], kp["jacobian"])
        call()
        torch.cuda.synchronize()
        f0 = L.eamm_total_mfma_flops()
        call()
        torch.cuda.synchronize()
        gflop = (L.eamm_total_mfma_flops() - f0) / B / 1e9
        ms = event_ms(call, args.iters)
        fps = B / (ms * 1e-3)
        res[f"b{B}_ms"] = round(ms, 4)
        res[f"b{B}_frames_per_s"] = round(fps, 1)
        res[f"b{B}_peak_frac"] = round(gflop * 1e9 * fps / PEAK_FP32_MATRIX, 4)
        res["executed_gflop_per_frame"] = round(gflop, 4)
        del m
        torch.cuda.empty_cache()
    if not args.no_e2e:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from test_gpu_pipeline import build
        _, _, _, _, _, _, _, (gen, kpd, tail, kpa) = build()
        T = args.clip_frames
        emo = EmotionDetector(**cfg, max_batch=256)
        emo.load_state_dict(sd, strict=True)
        emo = emo.to(dev).eval()
        src, feats = synthetic_source(256, seed=1), synthetic_lstm_features(T, seed=6)
        frames_e = synthetic_source(256, seed=9, batch=T).to(dev)
        _, _, kps = animate_from_features(gen, kpd, tail, kpa, src, feats, emo_detector=emo, emotion_frames=frames_e, return_keypoints=True)
        pre = {k: v.clone() for k, v in kps["emo_driving"].items()}

        def wall(**kw):
            animate_from_features(gen, kpd, tail, kpa, src, feats, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                animate_from_features(gen, kpd, tail, kpa, src, feats, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / 2
        for name, kw in (("none", {}), ("precomputed", {"emo_driving": pre}),
                         ("on_device", {"emo_detector": emo, "emotion_frames": frames_e})):
            t = wall(**kw)
            res[f"e2e_{name}_frames_per_s"] = round(T / t, 1)
        res["e2e_clip_frames"] = T
        res["e2e_on_device_vs_none"] = round(res["e2e_on_device_frames_per_s"] / res["e2e_none_frames_per_s"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
