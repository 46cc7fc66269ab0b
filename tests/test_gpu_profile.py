"""The stage profile of eamm_forward_frames (Engine.profile / Engine.profile_read, the 22 slots of Engine.STAGES) on the two
shapes of a call: ONE launch sequence (one frame: F(4x4) bottleneck with its point rows split over workgroups) and TWO
whole-pass chains (8 frames with EAMM_PASS_CHAINS=2: two chains of 4 frames, 64 tiles each).  A characterisation of what the
slots hold -- counts, signs, and the flop accounting against the process-wide counter -- with no assertion on a duration
beyond its sign; and profiling must not change a frame."""
import math

import pytest
import torch

from eamm_amd import OcclusionAwareGenerator, _lib, tiny_config
from eamm_amd.weights import synthetic_keypoints, synthetic_source, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GF = ("gf_front", "gf_hg_enc", "gf_hg_dec", "gf_head", "gf_warp", "gf_bneck", "gf_up", "gf_final")


@pytest.mark.parametrize("n,env,chains", [(1, {}, 1), (8, {"EAMM_PASS_CHAINS": "2"}, 2)])
def test_profile_slots_and_flop_accounting(n, env, chains, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = tiny_config()
    with torch.no_grad():
        gen = OcclusionAwareGenerator(**cfg, max_frames=8)
        gen.load_state_dict(synthetic_state_dict(cfg, seed=1234), strict=True)
        gen = gen.to(DEV).eval()
        eng = gen.encode_source(synthetic_source(64, seed=1).to(DEV), max_frames=8)
        assert eng.pass_chains(n) == chains and eng.bottleneck_form(n // chains) == 4
        plan = eng.describe_plan(n)
        assert plan["frames_per_chain"] == n // chains
        assert (plan["wino4_groups"] > 1) == (chains == 1)      # one frame: the point rows are split; chains never split them
        kd = {k: v.to(DEV) for k, v in synthetic_keypoints(n, cfg["num_kp"], seed=2).items()}
        ks = {k: v.to(DEV) for k, v in synthetic_keypoints(1, cfg["num_kp"], seed=0).items()}
        plain = eng.forward_frames(kd, ks)["prediction"].clone()
        torch.cuda.synchronize()

        eng.profile(True)
        flops0 = _lib.lib().eamm_total_mfma_flops()
        outs = [eng.forward_frames(kd, ks)["prediction"] for _ in range(3)]
        flops1 = _lib.lib().eamm_total_mfma_flops()
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o, plain)
        prof = eng.profile_read(reset=True)
        eng.profile(False)

    ms = prof["ms"]
    print("\n", n, "frames:", prof["calls"], prof["frames"], {k: round(v, 6) for k, v in ms.items()})
    assert prof["calls"] == 3 and prof["frames"] == 3 * n
    assert len(ms) == 22 and all(math.isfinite(v) for v in ms.values())
    assert ms["bneck_transform"] > 0 and ms["bneck_gemm_kernel"] > 0
    assert ms["bneck_windows"] >= ms["bneck_union"] > 0
    assert ms["exec_gflop"] > 0
    assert abs(sum(ms[k] for k in GF) - ms["exec_gflop"]) <= 1e-9 * ms["exec_gflop"]
    assert ms["bneck_exec_gflop"] == ms["gf_bneck"]
    assert abs(ms["exec_gflop"] * 1e9 - (flops1 - flops0)) <= 1e-9 * (flops1 - flops0)

    again = eng.profile_read(reset=True)
    assert again["calls"] == 0 and again["frames"] == 0 and all(v == 0 for v in again["ms"].values())
