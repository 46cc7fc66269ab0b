"""The MFCC kernel (eamm_op_mfcc, csrc/mfcc.hip) on the MI355X against the float64 oracle, its determinism (a frame's row
depends on its own samples only), the input_mfcc windows, and animate_from_audio equal to animate_from_features given the
same windows and pose track -- streamed or not, with the emotion detector, one rank or two."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from eamm_amd import (EmotionDetector, animate_from_audio, animate_from_features, emotion_detector_config, mfcc, mfcc_reference,
                      mfcc_windows, prepare_pose)
from eamm_amd.weights import emotion_state_dict_spec, synthetic_source, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2e-4
SR = 16000


def voiced_with_gaps(S, rs):
    t = np.arange(S) / SR
    f0 = 140 + 40 * np.sin(2 * np.pi * 0.7 * t)
    x = sum(0.25 / h * np.sin(2 * np.pi * h * np.cumsum(f0) / SR) for h in range(1, 12)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x += 0.003 * rs.standard_normal(S)
    for a in range(S // 7, S, S // 3):
        x[a:a + S // 10] = 0.0
    return x


def quantised_noise(S, rs):
    return np.round(rs.uniform(-1, 1, S) * 32767) / 32768


def quiet_noise(S, rs):
    return 3e-4 * rs.standard_normal(S)


def lowpassed_noise(S, rs):
    X = np.fft.rfft(rs.standard_normal(S))
    X[np.fft.rfftfreq(S, 1 / SR) > 1000] = 0          # brick wall at 1 kHz: the upper mel bands hold only frame leakage
    return 0.1 * np.fft.irfft(X, S)


def click(S, rs):
    x = np.zeros(S)
    x[S // 2] = 0.5
    return x


def tone(S, rs):
    return 0.4 * np.sin(2 * np.pi * 200 * np.arange(S) / SR)


SIGNALS = {f.__name__: f for f in (voiced_with_gaps, quantised_noise, quiet_noise, lowpassed_noise, click, tone)}
LONG = 82 * SR


def sig(name, S, seed=0):
    return SIGNALS[name](S, np.random.RandomState(seed)).astype(np.float32)


@pytest.mark.parametrize("pad", [0, 1920])
@pytest.mark.parametrize("S", [721, 16000, LONG])
@pytest.mark.parametrize("name", list(SIGNALS))
def test_kernel_against_the_oracle(name, S, pad):
    x = sig(name, S)
    got = mfcc(torch.from_numpy(x).to(DEV), pad=pad).cpu().numpy()
    ref = mfcc_reference(x, pad)
    assert got.shape == ref.shape and got.dtype == np.float32
    err = float(np.abs(got - ref).max())
    assert err <= TOL, (name, S, pad, err)


def test_batch_against_the_oracle_and_bit_identity():
    S = 16000
    xs = np.stack([sig("voiced_with_gaps", S, 1), sig("lowpassed_noise", S, 2), sig("click", S, 3)])
    w = torch.from_numpy(xs).to(DEV)
    got = mfcc(w)
    assert got.shape == (3, 123, 13)                                        # L = 16000 + 3840: 1 + ceil(19440 / 160)
    for i in range(3):
        assert float(np.abs(got[i].cpu().numpy() - mfcc_reference(xs[i])).max()) <= TOL, i
        assert torch.equal(got[i], mfcc(w[i])), i                         # a clip alone == the clip inside a 3-clip call
    assert torch.equal(got, mfcc(w))                                        # two calls agree


@pytest.mark.parametrize("pad", [0, 1920])
def test_rows_do_not_depend_on_clip_length_or_position(pad):
    long_ = torch.from_numpy(sig("voiced_with_gaps", 40000, 5)).to(DEV)
    full = mfcc(long_, pad=pad)
    for S in (721, 5000, 12345):
        part = mfcc(long_[:S], pad=pad)
        # rows whose frames end before the shorter clip's end (the trailing pad differs from the longer clip's samples)
        keep = max(0, (S + pad - 400) // 160 + 1)
        assert keep > 0 and torch.equal(part[:keep], full[:keep]), S
    # the same samples in another position of a 3-clip batch: a shift by a whole number of frames (160 samples) moves rows
    shift = 160 * 13
    a = long_[shift:shift + 20000]
    b = torch.stack([long_[:20000], long_[:20000], a])
    rows = mfcc(b, pad=0)
    first = mfcc(long_[:20000 + shift], pad=0)
    n = (20000 - 400) // 160 + 1
    assert torch.equal(rows[0], rows[1])
    # (frame 0 of the shifted clip differs: its first sample has no predecessor for the pre-emphasis)
    assert torch.equal(rows[2, 1:n], first[14:13 + n])


def test_windows_against_the_oracle():
    x = sig("voiced_with_gaps", 3 * SR, 7)
    got = mfcc_windows(torch.from_numpy(x).to(DEV))
    ref = mfcc_reference(x)
    T = ref.shape[0] // 4 - 6
    want = np.stack([ref[4 * t:4 * t + 28, 1:] for t in range(T)])
    assert tuple(got.shape) == (T, 28, 12) and got.is_contiguous()
    assert float(np.abs(got.cpu().numpy() - want).max()) <= TOL
    assert torch.equal(got, mfcc(torch.from_numpy(x).to(DEV))[:4 * T + 24].unfold(0, 28, 4)[:, 1:].permute(0, 2, 1))
    b = mfcc_windows(torch.from_numpy(np.stack([x, x])).to(DEV))
    assert tuple(b.shape) == (2, T, 28, 12) and torch.equal(b[1], got)


def test_errors_before_any_launch():
    with pytest.raises(ValueError, match="721"):
        mfcc_windows(torch.zeros(720, device=DEV))
    with pytest.raises(ValueError):
        mfcc(torch.zeros(1000, dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError):
        mfcc(torch.zeros(2, 2, 1000, device=DEV))
    with pytest.raises(ValueError):
        mfcc(torch.zeros(0, device=DEV))


def _nets():
    from test_gpu_audio_feature import _pipeline, net
    gen, kp, _, kpa = _pipeline()
    return gen, kp, kpa, net()


def _clip(T_target=40, seed=11):
    S = (T_target + 6) * 4 * 160 + 400 - 2 * 1920
    wave = torch.from_numpy(sig("voiced_with_gaps", S, seed))
    pose = np.random.RandomState(seed).uniform(-0.3, 0.3, (17, 7))
    return wave, pose


@pytest.mark.parametrize("with_emo", [False, True])
def test_animate_from_audio_is_animate_from_features_with_windows(with_emo):
    gen, kp, kpa, m = _nets()
    src = synthetic_source(256, seed=1)
    wave, pose = _clip()
    windows = mfcc_windows(wave.to(DEV))
    T = windows.shape[0]
    assert T == 40
    pose_t = prepare_pose(pose, T)
    kw = dict(batch=16, front_batch=16, uint8=False, to_host=True, return_keypoints=True)
    if with_emo:
        cfg_e = emotion_detector_config()
        emo = EmotionDetector(**cfg_e, max_batch=16)
        emo.load_state_dict(synthetic_state_dict(cfg_e, seed=4321, spec=emotion_state_dict_spec(cfg_e)), strict=True)
        kw.update(emo_detector=emo.to(DEV).eval(), emotion_frames=synthetic_source(256, seed=9, batch=T))
    for streamed in (False, True):
        f_ref, s_ref, k_ref = animate_from_features(gen, kp, m.decon, kpa, src, None, audio_feature=m, audio=windows, pose=pose_t,
                                                    stream=streamed, **kw)
        f_a, s_a, k_a = animate_from_audio(gen, kp, m, kpa, src, wave, pose, stream=streamed, **kw)
        assert s_a == s_ref == (0, T)
        assert k_a["mfcc"].shape == (4 * T + 25, 13) and torch.equal(k_a["mfcc"], mfcc(wave.to(DEV)))
        names = ["kp_driving_raw", "kp_norm"] + (["emo_driving"] if with_emo else [])
        for name in names:
            for k in ("value", "jacobian"):
                assert torch.equal(k_a[name][k], k_ref[name][k]), (streamed, name, k)
        assert torch.equal(k_a["lstm_features"], k_ref["lstm_features"]), streamed
        assert torch.equal(f_a, f_ref), streamed


def test_animate_from_audio_rejects_bad_input():
    gen, kp, kpa, m = _nets()
    src = synthetic_source(256, seed=1)
    wave, pose = _clip()
    with pytest.raises(ValueError, match="721"):
        animate_from_audio(gen, kp, m, kpa, src, wave[:700], pose)
    with pytest.raises(ValueError):
        animate_from_audio(gen, kp, m, kpa, src, torch.stack([wave, wave]), pose)
    with pytest.raises(ValueError):
        animate_from_audio(gen, kp, m, kpa, src, None, pose)


def _rank_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)                                   # both ranks share the one GPU of the box
    gen, kp, kpa, m = _nets()
    if rank == 0:
        src = synthetic_source(256, seed=1)
        wave, pose = _clip(T_target=9)
    else:
        src, wave, pose = None, None, None
    frames, _ = animate_from_audio(gen, kp, m, kpa, src, wave, pose, batch=4, front_batch=8, uint8=False, to_host=True)
    np.save(os.path.join(tmp, f"shard{rank}.npy"), frames.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_from_a_waveform_match_one_rank(tmp_path):
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = np.concatenate([np.load(tmp_path / f"shard{r}.npy") for r in range(world)], axis=0)
    gen, kp, kpa, m = _nets()
    wave, pose = _clip(T_target=9)
    ref, span = animate_from_audio(gen, kp, m, kpa, synthetic_source(256, seed=1), wave, pose, batch=4, front_batch=8, uint8=False,
                                   to_host=True, stream=False)
    assert span == (0, 9)
    # as test_gpu_audio_feature's two-rank case: a rank's batches start at its shard's first frame, equal to rounding
    assert got.shape == tuple(ref.shape) and np.abs(got - ref.cpu().numpy()).max() <= 2e-5
