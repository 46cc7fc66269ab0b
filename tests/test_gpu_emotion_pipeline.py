"""animate_from_features with the emotion detector on the device (demo.py:221-228): emo_driving computed from the emotion frames
and the RAW driving key points, chunk by chunk, then smoothed and applied like a precomputed one."""
import pytest
import torch

from eamm_amd import EmotionDetector, animate_from_features, emotion_detector_config
from eamm_amd.weights import emotion_state_dict_spec, synthetic_lstm_features, synthetic_source, synthetic_state_dict

from test_gpu_pipeline import DEV, build

pytestmark = pytest.mark.gpu


def test_on_device_emotion_matches_precomputed_and_streaming():
    cfg, sd, cfg_k, sd_k, cfg_a, sd_a, sd_d, (gen, kp, tail, kpa) = build()
    T, FB = 300, 128                       # three front_batch chunks: 128, 128, 44
    cfg_e = emotion_detector_config()
    emo = EmotionDetector(**cfg_e, max_batch=FB)
    emo.load_state_dict(synthetic_state_dict(cfg_e, seed=4321, spec=emotion_state_dict_spec(cfg_e)), strict=True)
    emo = emo.to(DEV).eval()
    src, feats = synthetic_source(256, seed=1), synthetic_lstm_features(T, seed=6)
    frames_e = synthetic_source(256, seed=9, batch=T)
    kw = dict(batch=64, front_batch=FB, uint8=False, to_host=True, return_keypoints=True)
    f_dev, s_dev, k_dev = animate_from_features(gen, kp, tail, kpa, src, feats, emo_detector=emo, emotion_frames=frames_e,
                                                stream=False, **kw)
    raw = k_dev["kp_driving_raw"]
    pre = emo.detect(frames_e.to(DEV), raw["value"], raw["jacobian"])
    assert torch.equal(k_dev["emo_driving"]["value"], pre["value"]) and torch.equal(k_dev["emo_driving"]["jacobian"], pre["jacobian"])
    assert torch.equal(k_dev["emotion_features"], pre["feature"])
    f_pre, _, k_pre = animate_from_features(gen, kp, tail, kpa, src, feats, emo_driving={"value": pre["value"], "jacobian": pre["jacobian"]},
                                            stream=False, **kw)
    assert torch.equal(f_dev, f_pre)
    f_st, s_st, k_st = animate_from_features(gen, kp, tail, kpa, src, feats, emo_detector=emo, emotion_frames=frames_e, stream=True, **kw)
    assert s_st == s_dev == (0, T)
    for name in ("kp_driving_raw", "kp_driving_smoothed", "kp_norm", "emo_driving"):
        for k in ("value", "jacobian"):
            assert torch.equal(k_dev[name][k], k_st[name][k]), (name, k)
    assert torch.equal(k_dev["emotion_features"], k_st["emotion_features"])
    assert torch.equal(f_dev, f_st)
    f_neutral, _ = animate_from_features(gen, kp, tail, kpa, src, feats, stream=False, batch=64, front_batch=FB, uint8=False)
    assert float((f_neutral - f_dev).abs().max()) > 1e-3
