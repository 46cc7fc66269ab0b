"""AudioFeatureNet on the MI355X: lstm_features and forward against the reference's fixtures (tools/make_audio_golden.py), the
chunked recurrence bit-identical to one launch, and animate_from_features from audio -- streamed or not, one rank or two --
equal to the same call given the precomputed features."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN
from eamm_amd import AudioFeatureNet, animate_from_features
from eamm_amd.weights import audio_feature_state_dict_spec, synthetic_audio_inputs, synthetic_source, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_NET = {}


def net(max_batch=256):
    if max_batch not in _NET:
        z = np.load(os.path.join(GOLDEN, "audio_small.npz"))
        m = AudioFeatureNet(max_batch=max_batch)
        m.load_state_dict(synthetic_state_dict(None, seed=int(z["weight_seed"]), spec=audio_feature_state_dict_spec()), strict=True)
        _NET[max_batch] = m.to(DEV).eval()
    return _NET[max_batch]


def inputs(z):
    return synthetic_audio_inputs(int(z["clips"]), int(z["steps"]), seed=int(z["input_seed"]))


def tol(z, key):
    return max(1e-4, 4 * float(z["floor_" + key]))


@pytest.mark.parametrize("name", ["audio_small", "audio_batch2", "audio_long"])
def test_lstm_features_against_the_reference(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    image, audio, pose = inputs(z)
    out = net().lstm_features(image.to(DEV), audio.to(DEV), pose.to(DEV), float(z["weight"])).cpu().numpy()
    assert out.shape == (int(z["clips"]), int(z["steps"]), 256)
    got = out[:, z["lstm_steps"]] if "lstm_steps" in z.files else out
    err = float(np.abs(got - z["lstm_out"]).max())
    assert err <= tol(z, "lstm_out"), (name, err, tol(z, "lstm_out"))


@pytest.mark.parametrize("name", ["audio_small", "audio_batch2"])
def test_forward_against_the_reference_and_decon(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    image, audio, pose = (t.to(DEV) for t in inputs(z))
    m = net()
    deco = m(image, audio, pose, "cnn", float(z["weight"]))
    n, t = int(z["clips"]), int(z["steps"])
    assert tuple(deco.shape) == (n, t, 35, 64, 64)
    err = float(np.abs(deco[:, :, ::5, ::7, ::7].cpu().numpy() - z["deco_sample"]).max())
    assert err <= tol(z, "deco_out"), (name, err)
    feats = m.lstm_features(image, audio, pose, float(z["weight"]))
    assert torch.equal(deco, m.decon(feats.reshape(n * t, 256)).view(n, t, 35, 64, 64))


@pytest.mark.parametrize("chunk", [7, 128])
def test_chunked_recurrence_is_bit_identical(chunk):
    image, audio, pose = (t.to(DEV) for t in synthetic_audio_inputs(2, 300, seed=8))
    m = net()
    whole = m.lstm_features(image, audio, pose)
    state, parts = {}, []
    for t0 in range(0, 300, chunk):
        parts.append(m.lstm_features(image, audio[:, t0:t0 + chunk], pose[:, t0:t0 + chunk], state=state))
    assert torch.equal(torch.cat(parts, dim=1), whole)
    assert state["h"].shape == (3, 2, 256) and torch.equal(state["h"][2], whole[:, -1])
    small = net(max_batch=16).lstm_features(image, audio, pose)     # 8 steps per pass instead of 128
    assert torch.equal(small, whole)
    m.check()


@pytest.mark.parametrize("clips", [5, 8])
def test_many_clips_equal_single_clip_calls(clips):
    """every clip of a 5- or 8-clip call (two gate rows per recurrence thread) equals its own one-clip call, bit for bit"""
    image, audio, pose = (t.to(DEV) for t in synthetic_audio_inputs(clips, 40, seed=15))
    m = net()
    many = m.lstm_features(image, audio, pose)
    for i in range(clips):
        one = m.lstm_features(image[i:i + 1], audio[i:i + 1], pose[i:i + 1])
        assert torch.equal(many[i:i + 1], one), i
    state, parts = {}, []
    for t0 in range(0, 40, 13):                                       # chunked, with the image encoded by the first call only
        parts.append(m.lstm_features(image, audio[:, t0:t0 + 13], pose[:, t0:t0 + 13], state=state))
    assert state["clip"].shape == (clips, 1024) and torch.equal(torch.cat(parts, dim=1), many)
    m.check()


def test_against_the_reference_with_eight_clips():
    """audio_batch2's two clips inside an 8-clip call (the other six: other inputs) still match the reference"""
    z = np.load(os.path.join(GOLDEN, "audio_batch2.npz"))
    image, audio, pose = inputs(z)
    xi, xa, xp = synthetic_audio_inputs(6, int(z["steps"]), seed=77)
    out = net().lstm_features(torch.cat([xi, image]).to(DEV), torch.cat([xa, audio]).to(DEV), torch.cat([xp, pose]).to(DEV),
                              float(z["weight"])).cpu().numpy()
    err = float(np.abs(out[6:] - z["lstm_out"]).max())
    assert err <= tol(z, "lstm_out"), err


def _pipeline():
    from test_gpu_pipeline import build
    mods = build()[-1]
    return mods


def test_animate_from_audio_matches_precomputed_features():
    gen, kp, tail, kpa = _pipeline()
    T, FB = 300, 128
    m = net()
    src = synthetic_source(256, seed=1)
    _, audio, pose = synthetic_audio_inputs(1, T, seed=12)
    feats = m.lstm_features(src.to(DEV), audio.to(DEV), pose.to(DEV))[0]
    kw = dict(batch=64, front_batch=FB, uint8=False, to_host=True, return_keypoints=True)
    f_pre, s_pre, k_pre = animate_from_features(gen, kp, tail, kpa, src, feats, stream=False, **kw)
    for streamed in (False, True):
        f_a, s_a, k_a = animate_from_features(gen, kp, tail, kpa, src, None, audio_feature=m, audio=audio, pose=pose, stream=streamed,
                                              **kw)
        assert s_a == s_pre == (0, T)
        assert torch.equal(k_a["lstm_features"], feats), streamed
        for name in ("kp_driving_raw", "kp_norm"):
            for k in ("value", "jacobian"):
                assert torch.equal(k_a[name][k], k_pre[name][k]), (streamed, name, k)
        assert torch.equal(f_a, f_pre), streamed


def _rank_worker(rank, world, port, T, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)                                   # both ranks share the one GPU of the box
    gen, kp, tail, kpa = _pipeline()
    if rank == 0:
        src = synthetic_source(256, seed=1)
        _, audio, pose = synthetic_audio_inputs(1, T, seed=12)
        args = dict(audio_feature=net(), audio=audio, pose=pose)
    else:
        src, args = None, {}
    frames, (a, b) = animate_from_features(gen, kp, tail, kpa, src, None, batch=4, front_batch=8, uint8=False, to_host=True, **args)
    np.save(os.path.join(tmp, f"shard{rank}.npy"), frames.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_from_audio_match_one_rank(tmp_path):
    T, world = 9, 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(world, port, T, str(tmp_path)), nprocs=world, join=True)
    got = np.concatenate([np.load(tmp_path / f"shard{r}.npy") for r in range(world)], axis=0)
    gen, kp, tail, kpa = _pipeline()
    src = synthetic_source(256, seed=1)
    _, audio, pose = synthetic_audio_inputs(1, T, seed=12)
    ref, span = animate_from_features(gen, kp, tail, kpa, src, None, audio_feature=net(), audio=audio, pose=pose, batch=4, front_batch=8,
                                      uint8=False, to_host=True, stream=False)
    # a rank's batches start at its shard's first frame (split-K plans of ragged batches differ): equal to rounding
    assert got.shape == tuple(ref.shape) and np.abs(got - ref.cpu().numpy()).max() <= 2e-5
