"""The emotion video's kernels (csrc/video_prep.hip: eamm_op_resize_aa, eamm_op_similarity_warp, eamm_op_emotion_augment) on the
MI355X against the float64 numpy oracle, the lazy EmotionVideo's chunking invariance, and EmotionVideo as ``emotion_frames`` of
animate_from_features / animate_from_audio, bit-identical to its materialised tensor."""
import math

import numpy as np
import pytest
import torch

from eamm_amd import (EmotionDetector, EmotionVideo, align_video, animate_from_audio, animate_from_features, crop_source,
                      crop_source_reference, emotion_detector_config, mfcc_windows, perspective_params, prepare_pose)
from eamm_amd import video_input as vi
from eamm_amd.weights import emotion_state_dict_spec, synthetic_source, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def smooth_frames(n, h, w, c=3, seed=0):
    """uint8 frames with structure at several scales (gradients, blobs, fine noise), so every interpolation weight matters"""
    rs = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = []
    for i in range(n):
        ch = []
        for k in range(c):
            f = rs.uniform(2, 9, 2)
            v = 0.5 + 0.3 * np.sin(2 * np.pi * (f[0] * x + 0.3 * i)) * np.cos(2 * np.pi * f[1] * y) + 0.1 * rs.standard_normal((h, w))
            ch.append(v)
        out.append(np.stack(ch, -1))
    return (np.clip(np.stack(out), 0, 1) * 255).astype(np.uint8)


def face_landmarks(n, scale=1.0, seed=10):
    """[N,68,2]: one point set, moved by a small similarity per frame"""
    rs = np.random.RandomState(seed)
    base = (rs.uniform(60, 196, (68, 2)) - 128) * scale + 128 * scale
    out = []
    for i in range(n):
        th, s, t = rs.uniform(-0.15, 0.15), rs.uniform(0.9, 1.1), rs.uniform(-8, 8, 2)
        R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        out.append((base - 128 * scale) @ (s * R).T + 128 * scale + t)
    return np.stack(out)


def assert_levels(got, want, what):
    """final uint8 levels k = 255 v: equal on >= 99.999 % of the values, never more than one apart"""
    kg = np.rint(np.asarray(got, np.float64) * 255).astype(np.int64)
    kw = np.rint(np.asarray(want, np.float64) * 255).astype(np.int64)
    diff = np.abs(kg - kw)
    assert diff.max() <= 1, (what, int(diff.max()))
    assert (diff == 0).mean() >= 0.99999, (what, float((diff == 0).mean()))


@pytest.mark.parametrize("shape", [(256, 256, 3), (512, 512, 3), (180, 320, 3), (256, 256, 4), (300, 200, 4)])
def test_resize_and_alignment_against_the_oracle(shape):
    f = smooth_frames(5, *shape, seed=shape[0])
    r = vi._resize_device(torch.from_numpy(f).to(DEV)).cpu().numpy()
    want = vi.resize_reference(f)
    assert r.shape == (5, 256, 256, 3) and r.dtype == np.uint8
    assert_levels(r / 255.0, want / 255.0, ("resize", shape))
    lm = face_landmarks(5)
    for emotion in (None, "surprised"):
        got = align_video(f, lm, emotion=emotion).cpu().numpy()
        ref = vi.align_reference(f, lm, emotion)
        assert got.shape == (5, 256, 256, 3) and got.dtype == np.float32
        np.testing.assert_array_max_ulp(got, ref, maxulp=1)
    assert not np.array_equal(align_video(f, lm).cpu().numpy(), align_video(f, lm, emotion="fear").cpu().numpy())
    plain = align_video(f, None).cpu().numpy()                        # landmarks None: the resized frames / 255
    np.testing.assert_array_equal(plain, (want / 255.0).astype(np.float32))


def _draw(n, angle, flip, p, e, noise=None, seed=7):
    d = {"flip": flip, "angle": angle, "pers": np.resize(np.asarray(p), n), "enlarge": np.resize(np.asarray(e), n)}
    if noise is None:
        d["noise_seed"] = seed
    else:
        d["noise"] = noise
    return d


CASES = [(0.0, False, [20], [20]), (30.0, True, [-29], [39]), (-30.0, False, [29, -20], [-39, 20]), (12.5, True, [-20, 25], [-20, -33])]


@pytest.mark.parametrize("host_noise", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_augmentation_against_the_oracle(case, host_noise):
    angle, flip, p, e = case
    n = 4
    f = smooth_frames(n, 256, 256, seed=3)
    lm = face_landmarks(n, seed=4)
    noise = np.random.RandomState(5).rand(n, 60, 100, 3).astype(np.float32) if host_noise else None
    ev = EmotionVideo(f, lm, draw=_draw(n, angle, flip, p, e, noise))
    got = ev.materialize(7).cpu().numpy()
    ref = vi.emotion_video_reference(f, lm, draw=ev.draw, T=7)
    assert got.shape == (7, 3, 256, 256) and got.dtype == np.float32
    assert_levels(got, ref, case)
    k = got.astype(np.float64) * 255
    assert np.array_equal(got, (np.rint(k) / 255).astype(np.float32))       # every value is float32(k / 255)


def test_seeded_clip_from_a_512_rgba_video():
    f = smooth_frames(3, 512, 512, 4, seed=6)
    lm = face_landmarks(3, seed=7)
    ev = EmotionVideo(f, lm, seed=2024)
    assert_levels(ev.materialize(5).cpu().numpy(), vi.emotion_video_reference(f, lm, seed=2024, T=5), "512 rgba")


def test_portrait_crop_against_the_oracle():
    img = smooth_frames(1, 400, 300, seed=8)[0]
    template = face_landmarks(1, seed=9)[0]
    lm = face_landmarks(1, scale=1.4, seed=9)[0] + np.array([10.0, -5.0])
    got = crop_source(img, lm, template).cpu().numpy()
    ref = crop_source_reference(img, lm, template)
    assert got.shape == (1, 3, 256, 256) and got.dtype == np.float32
    assert_levels(got, ref, "crop")
    assert np.array_equal(got, (np.rint(got.astype(np.float64) * 255) / 255).astype(np.float32))


def test_chunking_and_cyclic_invariance():
    n, T = 37, 230
    f = smooth_frames(n, 256, 256, seed=11)
    ev = EmotionVideo(f, face_landmarks(n, seed=12), seed=5)
    full = ev.materialize(T)
    assert torch.equal(torch.cat([ev[0:100], ev[100:T]]), full)
    assert torch.equal(full[3], full[3 + n]) and torch.equal(full[10:20], full[10 + 2 * n:20 + 2 * n])
    assert torch.equal(ev[T - 1], full[T - 1])
    assert torch.equal(ev[0:n], ev[n:2 * n])


def test_device_noise_and_explicit_noise():
    n = 3
    f = smooth_frames(n, 256, 256, seed=13)
    lm = face_landmarks(n, seed=14)
    same = vi.mouth_noise(42, range(n))
    dev = EmotionVideo(f, lm, draw=_draw(n, 17.0, True, [-23], [31], seed=42)).materialize(n)
    exp = EmotionVideo(f, lm, draw=_draw(n, 17.0, True, [-23], [31], noise=same)).materialize(n)
    assert torch.equal(dev, exp)                                     # the hash on the device is mouth_noise, bit for bit
    # no rotation, p = 0 (the identity homography): the noise stays in its (flipped) rectangle
    for flip in (False, True):
        a = EmotionVideo(f, lm, draw=_draw(n, 0.0, flip, [0], [20], seed=9)).materialize(n).cpu().numpy()
        b = EmotionVideo(f, lm, draw=_draw(n, 0.0, flip, [0], [20], noise=np.zeros((n, 60, 100, 3), np.float32))).materialize(n).cpu().numpy()
        cols = slice(256 - 185, 256 - 85) if flip else slice(85, 185)
        inside = np.zeros((256, 256), bool)
        inside[160:220, cols] = True
        assert np.array_equal(a[:, :, ~inside], b[:, :, ~inside]), flip
        assert np.all(b[:, :, inside] == 0)
        assert abs(float(a[:, :, inside].mean()) - 0.5) < 0.01, flip
    again = EmotionVideo(f, lm, draw=_draw(n, 0.0, False, [0], [20], seed=9)).materialize(n).cpu().numpy()
    other = EmotionVideo(f, lm, draw=_draw(n, 0.0, False, [0], [20], seed=10)).materialize(n).cpu().numpy()
    a = EmotionVideo(f, lm, draw=_draw(n, 0.0, False, [0], [20], seed=9)).materialize(n).cpu().numpy()
    assert np.array_equal(a, again) and not np.array_equal(a, other)


def test_bad_input_raises_before_any_launch():
    f = smooth_frames(2, 256, 256, seed=15)
    lm = face_landmarks(2)
    with pytest.raises(ValueError, match="uint8"):
        EmotionVideo(torch.from_numpy(f).to(DEV).float(), lm, seed=0)
    with pytest.raises(ValueError, match="C = 3 | 4"):
        EmotionVideo(torch.zeros(2, 256, 256, 2, dtype=torch.uint8, device=DEV), lm, seed=0)
    with pytest.raises(ValueError, match="landmarks"):
        EmotionVideo(f, lm[:1], seed=0)
    with pytest.raises(ValueError, match="empty"):
        EmotionVideo(np.zeros((0, 256, 256, 3), np.uint8), None, seed=0)
    with pytest.raises(ValueError, match="frame 1"):
        align_video(f, np.stack([lm[0], np.full((68, 2), 5.0)]))
    ev = EmotionVideo(f, lm, seed=0)
    with pytest.raises(ValueError):
        ev[-1]
    with pytest.raises(ValueError):
        ev[0:10:2]


def _nets():
    from test_gpu_audio_feature import _pipeline, net
    gen, kp, _, kpa = _pipeline()
    return gen, kp, kpa, net()


def test_emotion_video_drives_the_pipeline_like_its_materialised_tensor():
    gen, kp, kpa, m = _nets()
    src = synthetic_source(256, seed=1)
    from test_gpu_audio_input import _clip
    wave, pose = _clip()
    windows = mfcc_windows(wave.to(DEV))
    T = windows.shape[0]
    pose_t = prepare_pose(pose, T)
    n = 13                                                           # T = 40 > N, and 40 is not a multiple of front_batch 16
    ev = EmotionVideo(smooth_frames(n, 320, 240, seed=16), face_landmarks(n, seed=17), seed=77)
    cfg_e = emotion_detector_config()
    emo = EmotionDetector(**cfg_e, max_batch=16)
    emo.load_state_dict(synthetic_state_dict(cfg_e, seed=4321, spec=emotion_state_dict_spec(cfg_e)), strict=True)
    emo = emo.to(DEV).eval()
    kw = dict(batch=16, front_batch=16, uint8=False, to_host=True, return_keypoints=True, emo_detector=emo)
    mat = ev.materialize(T)
    for streamed in (False, True):
        f_ref, s_ref, k_ref = animate_from_features(gen, kp, m.decon, kpa, src, None, audio_feature=m, audio=windows, pose=pose_t,
                                                    stream=streamed, emotion_frames=mat, **kw)
        f_ev, s_ev, k_ev = animate_from_features(gen, kp, m.decon, kpa, src, None, audio_feature=m, audio=windows, pose=pose_t,
                                                 stream=streamed, emotion_frames=ev, **kw)
        assert s_ev == s_ref == (0, T)
        for name in ("emo_driving", "kp_norm"):
            for k in ("value", "jacobian"):
                assert torch.equal(k_ev[name][k], k_ref[name][k]), (streamed, name, k)
        assert torch.equal(k_ev["emotion_features"], k_ref["emotion_features"]), streamed
        assert torch.equal(f_ev, f_ref), streamed
        f_a, _, k_a = animate_from_audio(gen, kp, m, kpa, src, wave, pose, stream=streamed, emotion_frames=ev, **kw)
        assert torch.equal(f_a, f_ref), streamed
        assert torch.equal(k_a["emo_driving"]["value"], k_ref["emo_driving"]["value"]), streamed
