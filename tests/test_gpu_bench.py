"""bench.py contract on the GPU box: the JSON line at N=1 (plain and --full), and the N=2 code path (two ranks sharing GPU 0, gloo
collectives staged through the host -- the driver's real N>1 runs use one rank per GPU over RCCL)."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"}


def run(cmd, env=None):
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]   # exactly ONE JSON line, printed by rank 0
    return json.loads(lines[0])


def test_bench_single_gpu_line():
    d = run([sys.executable, "bench.py", "--steps", "10", "--warmup", "3", "--cpu-frames", "10", "--full"])
    assert REQUIRED <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 10 and d["warmup"] == 3 and d["scaling"] == "weak"
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 10 * 16 / (d["ms_per_step"] * 10e-3)) / d["value"] < 0.01   # value == frames / timed seconds
    r = d["roofline"]
    # everything under roofline is priced against the CHIP's fp32 matrix peak: frac = executed GEMM flops of all chains /
    # (wall time with any chain inside its bottleneck stage) / 157.3
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 157.3
    assert abs(r["achieved"] - r["bneck_executed_gflop_per_step"] / r["bneck_union_ms_per_step"]) / r["achieved"] < 0.01
    assert 0.2 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # the union of the chains' windows: at least the longest window, at most their sum and the step
    assert r["bneck_windows_sum_ms_per_step"] / r["pass_chains"] * 0.99 <= r["bneck_union_ms_per_step"] <= min(
        r["bneck_windows_sum_ms_per_step"], d["ms_per_step"]) * 1.01
    # executed GEMM flops: F(4x4) issues 36/144 of the reference's multiplies (tiles here are whole: no padding)
    assert abs(r["bneck_executed_gflop_per_step"] - r["algorithmic_gflop_per_step"] / 4) / r["bneck_executed_gflop_per_step"] < 0.01
    p = r["per_launch"]
    assert abs(p["achieved"] - p["executed_gflop"] / p["avg_launch_ms"]) / p["achieved"] < 0.01
    assert abs(p["frac_chip"] - p["achieved"] / 157.3) < 1e-3 and abs(p["frac_of_occupied_cus"] - p["frac_chip"] / p["cu_share"]) < 2e-3
    assert p["frames"] == 16 // r["chains"] and 0.1 < p["frac_chip"] <= p["frac_of_occupied_cus"] <= 1.0
    wp = r["whole_path"]
    assert 15.0 < wp["executed_gflop_per_frame"] < d["config"]["flops_per_frame"]       # fewer multiplies than the reference's 86.7
    assert abs(wp["frac_chip_executed"] - wp["executed_gflop_per_frame"] * d["value"] / 157.3e3) < 5e-3 and wp["frac_chip_executed"] <= 1.0
    assert abs(sum(d["stage_ms_per_step"].values()) - d["ms_per_step"]) / d["ms_per_step"] < 0.05  # events ~ wall clock
    # `value` is timed with the library's events OFF; the stage / roofline keys come from a second region of the same K steps
    # with them on: the two regions' wall clocks agree (the events cost next to nothing)
    assert abs(d["stage_region_ms_per_step"] - d["ms_per_step"]) / d["ms_per_step"] < 0.03
    w = d["roofline_warp"]
    assert w["bound"] == "hbm" and w["unit"] == "GB/s" and w["peak"] == 8000.0 and 0.1 < w["frac"] <= 1.0
    # bytes are those of the frames the TIMED launch covers (one chain's), 8.438 MB per frame
    assert w["frames_per_launch"] == 16 // r["pass_chains"] and w["algorithmic_bytes_per_launch"] == w["frames_per_launch"] * 8437760
    assert abs(w["achieved"] - w["algorithmic_bytes_per_launch"] / w["avg_launch_ms"] / 1e6) / w["achieved"] < 0.01
    wi = w["isolated"]
    assert wi["frames_per_launch"] == 16 and wi["algorithmic_bytes_per_launch"] == 16 * 8437760 and 0.3 < wi["frac"] <= 1.0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "frames/s" and c["cores"] >= 1 and c["value"] > 0
    assert len(c["passes"]) >= 5 and min(c["passes"]) <= c["value"] <= max(c["passes"])   # median of >= 5 passes
    # round 6: the box's physical cores, its logical CPUs and the threads the timed passes used are three separate fields
    assert c["threads_used"] == c["cores"] and 1 <= c["threads_used"] <= c["logical_cpus"] == os.cpu_count()
    assert c["physical_cores"] is None or 1 <= c["physical_cores"] <= c["logical_cpus"]
    # round 6: the FULL five-key forward timed beside the contract's prediction-only step ...
    a = d["all_outputs"]
    assert a["outputs"] == ["prediction", "mask", "sparse_deformed", "occlusion_map", "deformed"] and a["steps"] == 10
    assert abs(a["frames_per_s"] - 16 * 1e3 / a["ms_per_step"]) / a["frames_per_s"] < 0.01
    assert 0.75 * d["value"] <= a["frames_per_s"] <= 1.02 * d["value"] and a["prediction_max_abs_err_vs_fixture"] <= 1e-4
    # ... and ONE frame per call (BASELINE configs[1]): latency, executed-flop fraction, parity through that plan
    b1 = d["latency_b1"]
    assert 0.1 < b1["ms_per_frame"] < 2.0 and abs(b1["frames_per_s"] - 1e3 / b1["ms_per_frame"]) < 1.0
    assert 15.0 < b1["executed_gflop_per_frame"] < 40.0 and 0.0 < b1["frac_chip_executed"] < 1.0
    assert b1["parity_max_abs_err_vs_fixture"] <= 1e-4 and b1["plan"]["frames"] == 1
    assert d["value"] > 30 * c["value"]        # north_star target: >= 30x the CPU reference path
    # roofline.traffic: a committed PMC measurement of THIS kernel source at THIS (size, batch), or null with the reason
    assert (r["traffic"] is None or r["traffic"] > 0) and r["traffic_source"]
    # configs[3] leg: the whole 2048-frame clip (encode + compute) must run at the steady-state rate within a few %
    k = d["clip"]
    assert k["frames"] == 2048 and k["n_gpus"] == 1 and abs(k["frames_per_s"] - 2048 / k["seconds"]) < 1.0
    assert k["batch"] == 128         # the clip harness batches 128 frames per call = four chains of 32 (about 4 % over the contract line's 16)
    assert 0.9 * d["value"] <= k["frames_per_s"] <= 1.12 * d["value"], (k["frames_per_s"], d["value"])
    assert {"encode_ms", "compute_ms"} <= set(k["phases_ms_rank0"]) and len(k["phases_ms_per_rank"]) == 1
    # the clip leg looks at what its TIMED pass produced: fixture frames + spot frames recomputed under the
    # contract handle's plan; its own plan is the four-chain one
    v = k["verify"]
    assert v["ok"] is True and v["fixture"]["ok"] is True and v["fixture"]["max_abs_err"] <= 1e-4
    assert v["spot_frames"] == [0, 1024, 2047] and v["vs_contract_plan_max_abs"] <= 2e-5
    assert k["plan"]["pass_chains"] == 4 and k["plan"]["frames_per_chain"] == 32 and k["collectives_per_clip"] == 0
    # end-to-end leg: make_animation_smooth whole, frames delivered to pinned host memory
    e = d["e2e_clip"]
    assert e["frames"] == 2048 and e["verify"]["ok"] is True and e["verify"]["uint8_levels_vs_contract_plan"] <= 1
    assert e["verify"]["uint8_levels_streamed_vs_phased"] == 0        # streaming the front end changes no bit
    ph = e["phases_ms_rank0"]
    assert {"front_ms", "smooth_ms", "normalize_ms", "encode_ms", "compute_ms", "d2h_tail_ms"} <= set(ph)
    assert ph["smooth_ms"] <= 100.0, ph                # wall clock incl. a device sync (typically 0.7 ms, host jitter up to 10; the kernels' own time is
    # asserted with HIP events in tests/test_gpu_pipeline.py); the round-4 host loop: 608 ms
    assert e["host_bytes"] == 2048 * 256 * 256 * 3 and 0.5 * k["frames_per_s"] <= e["frames_per_s"] <= 1.25 * k["frames_per_s"]
    # the line says what it was measured under: parity at the timed geometry, knobs, launch plan
    pc = d["parity_check"]
    assert pc["ok"] is True and pc["fixture"] == "tests/golden/full256_clip2.npz" and pc["frames"] == 2 and pc["max_abs_err"] <= 1e-4
    kn = d["knobs"]
    assert kn["env"] == {} and kn["library"] == {} and kn["ignored"] == [] and kn["experiments_build"] == 0 and kn["library_defaults_read"] > 20
    assert kn["plan"]["frames"] == 16 and kn["plan"]["pass_chains"] == 2 and kn["plan"]["bottleneck_form"] == 4
    assert "executed" in r["flops_basis"] and "reference-equivalent" in r["algorithmic_note"]
    # N4 leg (not part of `value`): one fine-tuning step of 8 pairs, forward with autograd graph + loss.backward()
    t = d["train_step"]
    assert "error" not in t, t
    assert t["pairs"] == 8 and t["gradients_finite"] is True and t["step_ms"] > 0
    assert abs(t["pairs_per_s"] - 8 / t["step_ms"] * 1e3) / t["pairs_per_s"] < 0.01 and t["step_ms"] <= t["forward_ms"] + t["backward_ms"] + 5
    # every stage's fraction of the chip's matrix peak is in the line, consistent with the headline
    sr = d["stage_roofline"]
    assert {"hg_enc", "hg_dec", "head", "bneck", "up", "final"} <= set(sr)
    for k, v in sr.items():
        if k != "note":
            assert abs(v["tflops"] - v["executed_gflop_per_step"] / v["ms"]) / v["tflops"] < 0.01 and 0 < v["frac_chip"] <= 1.0, (k, v)
    assert abs(sr["bneck"]["executed_gflop_per_step"] - r["bneck_executed_gflop_per_step"]) / r["bneck_executed_gflop_per_step"] < 1e-3
    assert abs(sum(v["executed_gflop_per_step"] for k, v in sr.items() if k != "note") / 16 - wp["executed_gflop_per_frame"]) < 0.01
    assert abs(sr["bneck"]["frac_chip"] - r["frac"]) < 0.05      # main-stream stage time vs the union of the chains' windows
    _check_train_step_against_the_oracle(t)


def _check_train_step_against_the_oracle(t):
    """bench.py's training step prints its loss and gradient checksums; the same step (same seeds) through
    the CPU oracle's training branch, differentiated by autograd in DOUBLE, must give the same numbers."""
    import torch
    from bench import train_step_target
    from eamm_amd import hot_path_config
    from eamm_amd.weights import synthetic_keypoints, synthetic_source, synthetic_state_dict
    from oracle import eamm_oracle as orc
    cfg, pairs, size = hot_path_config(), t["pairs"], t["size"]
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    sd = synthetic_state_dict(cfg, seed=1234)
    leaf = lambda k, v: v.is_floating_point() and "running" not in k and "down.weight" not in k
    sdd = {k: (v.double().requires_grad_() if leaf(k, v) else v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    src = synthetic_source(size, seed=1, batch=pairs).double()
    kp_s = {k: v.double() for k, v in synthetic_keypoints(pairs, cfg["num_kp"], seed=0).items()}
    kp_d = {k: v.double().requires_grad_() for k, v in synthetic_keypoints(pairs, cfg["num_kp"], seed=2).items()}
    out, _ = orc.generator_forward_train(sdd, cfg, src, kp_d, kp_s, parallel=False)
    loss = (out["prediction"] - train_step_target(pairs, size).double()).abs().mean()
    loss.backward()
    want = {"loss": float(loss.detach()),
            "grad_l1/kp_driving.value": float(kp_d["value"].grad.abs().sum()),
            "grad_l1/final.weight": float(sdd["final.weight"].grad.abs().sum()),
            "grad_l1/bottleneck.r0.conv1.weight": float(sdd["bottleneck.r0.conv1.weight"].grad.abs().sum())}
    got = t["checks"]
    print("train_step checks: " + "  ".join(f"{k} {got[k]:.6g} (oracle64 {want[k]:.6g})" for k in want))
    assert abs(got["loss"] - want["loss"]) <= 2e-4 * abs(want["loss"]), (got["loss"], want["loss"])
    for k in want:   # L1 norms of whole gradient tensors: the per-element fp32 floor (a few 1e-3 at 8 pairs) averages out
        assert abs(got[k] - want[k]) <= 2e-2 * abs(want[k]), (k, got[k], want[k])


def test_bench_plain_run_prints_the_contract_line_only():
    """Without --full the run sets up, warms up, times the K steps and prints the contract line: the same headline keys as
    the --full line, the knobs and launch plan they were measured under, and none of the other legs' keys."""
    d = run([sys.executable, "bench.py", "--steps", "5", "--warmup", "2"])
    assert {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "knobs"} == set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "configs[2]" in d["config"]["workload"]
    assert d["metric"] == "256x256 frames/sec (dense-motion + generator forward)"
    assert abs(d["value"] - 5 * 16 / (d["ms_per_step"] * 5e-3)) / d["value"] < 0.01   # value == frames / timed seconds
    assert d["knobs"]["plan"]["frames"] == 16 and d["knobs"]["experiments_build"] == 0


def test_bench_512_batch8_line():
    """BASELINE configs[4]: --size 512 (batch 8 by default) prints the same line for the 512x512 workload."""
    d = run([sys.executable, "bench.py", "--size", "512", "--steps", "3", "--warmup", "1", "--cpu-frames", "0",
             "--clip-frames", "0", "--full"])
    assert "512x512" in d["config"]["workload"] and "configs[4]" in d["config"]["workload"]
    assert d["config"]["frames_per_step_per_gpu"] == 8 and d["clip"] is None and d["cpu_baseline"] is None
    assert abs(d["value"] - 3 * 8 / (d["ms_per_step"] * 3e-3)) / d["value"] < 0.01
    r = d["roofline"]
    assert 0.2 < r["frac"] <= 1.0 and "128x128" in r["kernel"] and r["peak"] == 157.3
    # here each chain runs the whole pass and its 4-frame bottleneck launches fill the chip: two such launches time-share it
    p = r["per_launch"]
    assert r["chains"] == 2 and p["launch_blocks"] >= r["cus"] and abs(p["cu_share"] - 1.0 / r["chains"]) < 1e-3
    assert d["roofline_warp"]["frames_per_launch"] == 8 // r["pass_chains"]


def test_bench_two_ranks_share_one_gpu():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    d = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
             "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--clip-frames", "70", "--clip-gather", "--e2e-frames", "0", "--full"],
            env={"EAMM_BENCH_BACKEND": "gloo"})
    assert d["n_gpus"] == 2 and d["cpu_baseline"] is None and "source_broadcast_ms" in d
    k = d["clip"]    # 70 frames over 2 ranks: 35 each, broadcast + compute + uint8 gather timed
    assert k["frames"] == 70 and k["n_gpus"] == 2 and k["shard_rank0"] == [0, 35] and k["frames_per_s"] > 0
    assert {"encode_ms", "broadcast_ms", "compute_ms", "gather_ms"} <= set(k["phases_ms_rank0"])
    assert abs(d["value"] - 2 * 3 * 16 / (d["ms_per_step"] * 3e-3)) / d["value"] < 0.01   # whole-job frames / max time


def test_bench_bare_gpus2_spawns_its_ranks():
    """The driver's command shape -- `python bench.py --gpus N` with no launcher and no WORLD_SIZE -- must start N ranks
    itself (it asserted).  Two ranks share this box's GPU under gloo; on a multi-GPU node the same command
    runs one rank per GPU over RCCL."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["EAMM_BENCH_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--clip-frames", "64", "--e2e-frames", "40", "--full"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["clip"]["n_gpus"] == 2 and d["clip"]["shard_rank0"] == [0, 32]
    k = d["clip"]      # both ranks verified their shard (spot frames under the contract plan), every rank's phases are in the line
    assert k["verify"]["ok"] is True and k["verify"]["spot_frames"] == [0, 16, 31] and k["collectives_per_clip"] == 2
    assert len(k["phases_ms_per_rank"]) == 2 and all(p["compute_ms"] > 0 for p in k["phases_ms_per_rank"])
    assert d["parity_check"]["ok"] is True and "rccl_warmup_ms" in d
    assert d["e2e_clip"]["frames"] == 40 and d["e2e_clip"]["n_gpus"] == 2 and d["e2e_clip"]["verify"]["ok"] is True
    assert abs(d["value"] - 2 * 3 * 16 / (d["ms_per_step"] * 3e-3)) / d["value"] < 0.01


def test_bench_rccl_path_single_rank():
    """The real backend (nccl = RCCL) with a one-rank group: init with device_id, broadcast of the source cache,
    barrier + all-reduce(MAX) around the timed region -- the calls the driver's N>1 runs make."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    d = run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--cpu-frames", "0", "--clip-frames", "64", "--e2e-frames", "0",
             "--full"],
            env={"EAMM_BENCH_FORCE_DIST": "1", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0",
                 "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    assert d["n_gpus"] == 1 and "source_broadcast_ms" in d and d["value"] > 0 and d["rccl_warmup_ms"] > 0
    assert d["clip"]["verify"]["ok"] is True and d["parity_check"]["ok"] is True


def test_bench_refuses_a_wrong_results_knob():
    """EAMM_WINO4_EPI_V=1 (a round-4 timing experiment that makes the bottleneck compute garbage) is compiled out of the product
    library: with it set, eamm_create fails loudly and bench.py prints no line."""
    out = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--cpu-frames", "0", "--clip-frames", "0",
                          "--train-pairs", "0", "--e2e-frames", "0"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env={**os.environ, "EAMM_WINO4_EPI_V": "1"})
    assert out.returncode != 0 and not [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert "EAMM_WINO4_EPI_V" in out.stderr and "EXPERIMENTS" in out.stderr
    d = run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--cpu-frames", "0", "--clip-frames", "0", "--train-pairs", "0", "--e2e-frames", "0",
             "--full"],
            env={"EAMM_PASS_CHAINS": "1", "EAMM_FINAL_FUSED_MIN_ROWS": "100000"})
    # a documented knob is honoured and recorded; a TUNING aid without EAMM_TUNING=1 is ignored (and reported as such): a stray
    # variable cannot change the plan silently
    assert d["knobs"]["env"] == {"EAMM_PASS_CHAINS": "1", "EAMM_FINAL_FUSED_MIN_ROWS": "100000"}
    assert d["knobs"]["library"] == {"EAMM_PASS_CHAINS": 1} and d["knobs"]["ignored"] == ["EAMM_FINAL_FUSED_MIN_ROWS"]
    assert d["knobs"]["plan"]["pass_chains"] == 1 and d["knobs"]["plan"]["bottleneck_chains"] == 2 and d["parity_check"]["ok"] is True
    assert d["knobs"]["plan"]["final"] == "col7q fused"


def test_bench_dump_outputs_are_the_timed_steps_outputs(tmp_path):
    """--dump-outputs DIR: the last timed step's `prediction` (this rank's 16 frames, float32) lands in DIR/prediction.npy,
    and its first frames are the committed reference fixture's (the timed launches use the fixture's seeds)."""
    import numpy as np
    d = run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--cpu-frames", "0", "--clip-frames", "0", "--train-pairs", "0",
             "--e2e-frames", "0", "--latency-frames", "0", "--no-all-outputs", "--dump-outputs", str(tmp_path / "out")])
    assert d["steps"] == 3 and d["dump_outputs"]["arrays"] == {"prediction": {"shape": [16, 3, 256, 256], "frames_of": 16}}
    assert sorted(os.listdir(tmp_path / "out")) == ["prediction.npy"]
    pred = np.load(tmp_path / "out" / "prediction.npy")
    assert pred.dtype == np.float32 and pred.shape == (16, 3, 256, 256) and np.isfinite(pred).all()
    z = np.load(os.path.join(ROOT, "tests", "golden", "full256_clip2.npz"))
    st, want = int(z["prediction_stride"]), z["prediction"]
    assert float(np.abs(pred[:want.shape[0], :, ::st, ::st] - want).max()) <= 1e-4
