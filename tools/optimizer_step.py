#!/usr/bin/env python
"""The optimiser step of the reference's train.py, alone: ``optimizer.step()`` between two HIP events, over the parameter sets of the
shipped configurations --

  a  stage 1             AudioFeatureNet + KPDetector_a                              (optimizer_audio_feature)
  b  stage 1 fine-tune   a + OcclusionAwareGenerator                                 (+ optimizer_generator)
  c  stage 2             EmotionDetector                                             (optimizer_emo_detector)

-- for four contestants: ``eamm_amd.Adam``; ``torch.optim.Adam`` with default arguments (what train.py constructs: THE BAR);
``torch.optim.Adam(foreach=False)``; ``torch.optim.Adam(fused=True)`` ("unavailable" where this torch build refuses it).  All with
lr 2e-4, betas (0.5, 0.999).  The modules are only a source of parameter shapes: parameters and gradients are seeded random tensors,
no forward or backward runs.  Median of 30 steps after 5 warm-up steps, repeated five times so that the spread shows; beside each
figure the 28 bytes per parameter one fused pass moves (read p, g, m, v; write p, m, v) and the rate that implies, and the launches
per step: ours from the library's own plan, torch's counted by torch.profiler where it yields kernel records.

Without ``--set`` / ``--only`` every (set, contestant) pair runs in a child process of its own under ``timeout``; the driver stops at
the first child that does not end normally.  Prints the lines kept in profiles/optimizer_step.txt."""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, REPS, ROUNDS = 5, 30, 5
LR, BETAS = 2e-4, (0.5, 0.999)
BYTES_PER_PARAM = 28
CHILD_TIMEOUT = 240
SETS = {"a": "stage 1 (AudioFeatureNet + KPDetector_a)", "b": "stage 1 + generator (fine-tuning)", "c": "stage 2 (EmotionDetector)"}
CONTESTANTS = {"eamm": "eamm_amd.Adam", "default": "torch.optim.Adam (default arguments)", "single": "torch.optim.Adam(foreach=False)",
               "fused": "torch.optim.Adam(fused=True)"}


def shapes_of(which):
    import eamm_amd as E
    mods = []
    if which in ("a", "b"):
        mods += [E.AudioFeatureNet(), E.KPDetector_a(**E.kp_detector_a_config())]
    if which == "b":
        mods.append(E.OcclusionAwareGenerator(**E.hot_path_config()))
    if which == "c":
        mods.append(E.EmotionDetector(**E.emotion_detector_config()))
    return [tuple(p.shape) for m in mods for p in m.parameters()]


def make(name, params):
    if name == "eamm":
        from eamm_amd import Adam
        return Adam(params, lr=LR, betas=BETAS)
    kw = {"default": {}, "single": {"foreach": False}, "fused": {"fused": True}}[name]
    return torch.optim.Adam(params, lr=LR, betas=BETAS, **kw)


def launches(name, opt, params):
    if name == "eamm":
        from eamm_amd import optim_ops
        return str(sum(1 for _, _, blocks in optim_ops.plan([p.numel() for p in params])[0] if blocks)), "the library's plan"
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return (str(n), "torch.profiler") if n else ("not counted", "torch.profiler gave no kernel records")
    except Exception as exc:       # a count is a courtesy, a timing is the tool's purpose
        return "not counted", f"torch.profiler: {type(exc).__name__}"


def run_one(which, name):
    dev = torch.device("cuda:0")
    shapes = shapes_of(which)
    gen = torch.Generator(dev).manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    total = sum(p.numel() for p in params)
    head = f"set {which} [{SETS[which]}: {len(params)} tensors, {total / 1e6:.1f} M parameters] {CONTESTANTS[name]:38s}"
    try:
        opt = make(name, params)
        opt.step()
        torch.cuda.synchronize()
    except Exception as exc:
        if name != "fused":
            raise
        print(f"{head} unavailable ({type(exc).__name__}: {str(exc).splitlines()[0][:120]})")
        return
    medians = []
    for _ in range(ROUNDS):
        for _ in range(WARM):
            opt.step()
        times = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); opt.step(); e1.record(); e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        medians.append(times[len(times) // 2])
    count, how = launches(name, opt, params)
    mid = sorted(medians)[ROUNDS // 2]
    gb = BYTES_PER_PARAM * total / 1e9
    print(f"{head} {mid:8.3f} ms (five medians of {REPS}: {' '.join(f'{m:.3f}' for m in medians)}; spread {max(medians) - min(medians):.3f}); "
          f"launches per step {count} ({how}); {gb:.3f} GB at 28 B per parameter = {gb / mid:.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=sorted(SETS))
    ap.add_argument("--only", choices=sorted(CONTESTANTS))
    a = ap.parse_args()
    if a.set and a.only:
        run_one(a.set, a.only)
        return
    for which in ([a.set] if a.set else sorted(SETS)):
        for name in ([a.only] if a.only else list(CONTESTANTS)):
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--set", which, "--only", name], timeout=CHILD_TIMEOUT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            sys.stdout.flush()
            if rc != 0:
                sys.exit(f"set {which}, {CONTESTANTS[name]}: the run ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
