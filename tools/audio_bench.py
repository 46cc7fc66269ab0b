#!/usr/bin/env python
"""Throughput of the audio network AT_net2 (AudioFeatureNet.lstm_features) on MI355X: one JSON line (also written to
profiles/audio_bench.json with --out) with, at T steps and N = 1 clip (HIP events, warm-up):
  * lstm_features ms in total, split by a kernel profile (torch.profiler) into the recurrence (lstm_rec_kernel: ms, us per step,
    us per step-layer) and everything else (the encoders and projections: ms, reference GFLOP per step, fraction of the fp32
    matrix peak at the reference's FLOP count and at the executed MFMA count);
  * the same network composed from stock torch.nn layers on the GPU (batched encoders, nn.LSTM) with the same weights, as the
    baseline, and its max distance from lstm_features;
  * animate_from_features frames/s from audio against the same call given precomputed lstm_features, both streamed.
Usage: python tools/audio_bench.py [--steps T] [--iters N] [--no-e2e] [--out profiles/audio_bench.json]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eamm_amd import AudioFeatureNet, _lib, animate_from_features  # noqa: E402
from eamm_amd.weights import audio_feature_state_dict_spec, synthetic_audio_inputs, synthetic_state_dict  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
# reference FLOPs per step (2 per multiply-add): audio_eocder on 28x12 then 26x5, audio_eocder_fc, pose MLP, LSTM input GEMMs
CNN_FLOP = 2 * (336 * 64 * 9 + 336 * 128 * 576 + 130 * 256 * 1152 + 130 * 256 * 2304 + 130 * 512 * 2304)
FC_FLOP = 2 * (12288 * 2048 + 2048 * 256 + 6 * 128 + 128 * 256)
PROJ_FLOP = 2 * (512 * 1024 + 2 * 256 * 1024)


def event_ms(fn, iters, warmup=2):
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


def torch_baseline(net, image, audio, pose, weight):
    """AT_net2's forward up to the LSTM from stock torch.nn layers (the module's own parameter holders), encoders batched."""
    n, t = audio.shape[:2]
    x = image
    for blk in net.down_blocks:
        x = F.avg_pool2d(F.relu(blk.norm(blk.conv(x))), 2)
    img = x.flatten(1)
    a = net.audio_eocder_fc(net.audio_eocder(audio.reshape(n * t, 1, 28, 12)).flatten(1)) * weight
    p = net.pose_encoder(pose.reshape(n * t, 6))
    inp = torch.cat([img[:, None].expand(n, t, 512), a.view(n, t, 256), p.view(n, t, 256)], dim=2)
    return net.lstm(inp)[0]


def kernel_split_ms(fn):
    """device ms of lstm_rec_kernel and of every other kernel in one call of fn (torch.profiler)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rec = other = 0.0
    for e in prof.events():
        us = getattr(e, "device_time", 0.0)
        if e.device_type != torch.autograd.DeviceType.CUDA or not us:
            continue
        if "lstm_rec_kernel" in e.name:
            rec += us
        elif "Memcpy" not in e.name and "Memset" not in e.name and "copyBuffer" not in e.name:
            other += us
    return rec / 1e3, other / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-split", action="store_true", help="skip the torch.profiler kernel split and the torch baseline (under rocprofv3)")
    args = ap.parse_args()
    dev, T, w = "cuda:0", args.steps, 1.6
    sd = synthetic_state_dict(None, seed=2468, spec=audio_feature_state_dict_spec())
    net = AudioFeatureNet()
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    image, audio, pose = (t.to(dev) for t in synthetic_audio_inputs(1, T, seed=31))
    call = lambda: net.lstm_features(image, audio, pose, w)
    out = call()
    torch.cuda.synchronize()
    L = _lib.lib()
    f0 = L.eamm_total_mfma_flops()
    call()
    torch.cuda.synchronize()
    executed = L.eamm_total_mfma_flops() - f0
    res = {"metric": "audio_feature", "steps": T, "clips": 1, "iters": args.iters}
    total = event_ms(call, args.iters)
    res["lstm_features_ms"] = round(total, 3)
    if args.no_split:
        print(json.dumps(res))
        return
    rec_ms, enc_ms = kernel_split_ms(call)
    res["recurrence_ms"] = round(rec_ms, 3)
    res["recurrence_us_per_step"] = round(rec_ms * 1e3 / T, 3)
    res["recurrence_us_per_step_layer"] = round(rec_ms * 1e3 / (3 * T), 3)
    res["encoder_ms"] = round(enc_ms, 3)
    ref_flop = T * (CNN_FLOP + FC_FLOP + PROJ_FLOP)
    res["encoder_ref_gflop_per_step"] = round((CNN_FLOP + FC_FLOP + PROJ_FLOP) / 1e9, 4)
    res["encoder_peak_frac"] = round(ref_flop / (enc_ms * 1e-3) / PEAK_FP32_MATRIX, 4) if enc_ms else None
    res["encoder_executed_peak_frac"] = round(executed / (enc_ms * 1e-3) / PEAK_FP32_MATRIX, 4) if enc_ms else None
    base = AudioFeatureNet()      # a second set of the same parameters; only its stock torch.nn sub-modules run
    base.load_state_dict(sd, strict=True)
    base = base.to(dev).eval()
    with torch.no_grad():
        ref = torch_baseline(base, image, audio, pose, w)
        res["torch_max_abs_diff"] = float((ref - out).abs().max())
        res["torch_baseline_ms"] = round(event_ms(lambda: torch_baseline(base, image, audio, pose, w), args.iters), 3)
    res["speedup_vs_torch"] = round(res["torch_baseline_ms"] / total, 3)
    del base
    if not args.no_e2e:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_gpu_pipeline import build
        _, _, _, _, _, _, _, (gen, kpd, tail, kpa) = build()
        src = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(1))
        feats = net.lstm_features(src.to(dev), audio, pose, w)[0]

        def wall(**kw):
            animate_from_features(gen, kpd, tail, kpa, src, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                animate_from_features(gen, kpd, tail, kpa, src, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / 2
        res["e2e_precomputed_frames_per_s"] = round(T / wall(lstm_features=feats, stream=True), 1)
        res["e2e_from_audio_frames_per_s"] = round(T / wall(lstm_features=None, audio_feature=net, audio=audio[0], pose=pose[0], stream=True), 1)
        res["e2e_from_audio_vs_precomputed"] = round(res["e2e_from_audio_frames_per_s"] / res["e2e_precomputed_frames_per_s"], 4)
    res["targets"] = {"encoder_peak_frac>=0.35": bool(res["encoder_peak_frac"] and res["encoder_peak_frac"] >= 0.35),
                      "recurrence_ms<=12": res["recurrence_ms"] <= 12.0}
    if "e2e_from_audio_vs_precomputed" in res:
        res["targets"]["e2e_ratio>=0.90"] = res["e2e_from_audio_vs_precomputed"] >= 0.90
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
