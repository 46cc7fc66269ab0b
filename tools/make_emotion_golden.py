"""Fixtures of the emotion detector (tests/golden/emotion_*.npz, emotion_keys.json), on the CPU from the reference itself.

Imports the reference's Emotion_k read-only (a stub cv2 on sys.path, as oracle/make_golden.py does), loads the seeded synthetic
weights strictly, runs forward + feature in eval mode and writes DATA only: seeds, config, the outputs, strided samples of the
hourglass and layer4 outputs (to localise a mismatch), and the reference's own fp32-vs-fp64 distance per output.  Images and key
points are regenerated from their seeds by the tests.  Usage: python tools/make_emotion_golden.py [reference checkout]
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eamm_amd.config import emotion_detector_config  # noqa: E402
from eamm_amd.weights import emotion_state_dict_spec, synthetic_keypoints, synthetic_source, synthetic_state_dict  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED, IMAGE_SEED, KP_SEED = 4321, 11, 40

CASES = {
    # name: (config overrides, size, frames, jacobian scale)
    "emotion_tiny128": ({"max_features": 256}, 128, 3, None),
    "emotion_full256": ({}, 256, 4, None),
    "emotion_full256_wide": ({}, 256, 2, 3.0),
}


def import_reference(path):
    stub = tempfile.mkdtemp(prefix="cv2stub_")
    open(os.path.join(stub, "cv2.py"), "w").close()
    sys.path[:0] = [stub, path]
    from modules.util import Emotion_k  # type: ignore
    return Emotion_k


def case_inputs(size, frames, jac_scale):
    """image [B,3,size,size] and key points [B,10,*]; jac_scale: jacobian entries uniform in +-jac_scale (sine range reduction)"""
    x = synthetic_source(size, seed=IMAGE_SEED, batch=frames)
    kp = synthetic_keypoints(frames, 10, seed=KP_SEED)
    if jac_scale is not None:
        rs = np.random.RandomState(KP_SEED + 1000)
        kp["jacobian"] = torch.from_numpy(rs.uniform(-jac_scale, jac_scale, (frames, 10, 2, 2)).astype(np.float32))
    return x, kp


def run(m, x, kp, hooks):
    with torch.no_grad():
        k, fake = m(x, kp["value"], kp["jacobian"])
        feat = m.feature(x)
    return {"value": k["value"], "jacobian": k["jacobian"], "fake": fake, "feature": feat}


def main():
    ref_path = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EAMM_REFERENCE", "reference")
    Emotion_k = import_reference(ref_path)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    keys_written = False
    for name, (over, size, frames, jac_scale) in CASES.items():
        cfg = {**emotion_detector_config(), **over}
        sd = synthetic_state_dict(cfg, seed=WEIGHT_SEED, spec=emotion_state_dict_spec(cfg))
        m = Emotion_k(**cfg).eval()
        m.load_state_dict(sd, strict=True)
        if not keys_written:
            ref_full = Emotion_k(**emotion_detector_config()).state_dict()
            with open(os.path.join(GOLDEN, "emotion_keys.json"), "w") as f:
                json.dump([[k, list(v.shape)] for k, v in ref_full.items()], f, indent=0)
                f.write("\n")
            keys_written = True
        x, kp = case_inputs(size, frames, jac_scale)
        taps = {}
        hs = [m.predictor.register_forward_hook(lambda mod, i, o: taps.__setitem__("hourglass", o)),
              m.layer4.register_forward_hook(lambda mod, i, o: taps.__setitem__("layer4", o))]
        out = run(m, x, kp, taps)
        for h in hs:
            h.remove()
        m64 = Emotion_k(**cfg).eval().double()
        m64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
        out64 = run(m64, x.double(), {k: v.double() for k, v in kp.items()}, None)
        rec = {"weight_seed": np.int64(WEIGHT_SEED), "image_seed": np.int64(IMAGE_SEED), "kp_seed": np.int64(KP_SEED),
               "size": np.int64(size), "frames": np.int64(frames), "jac_scale": np.float64(jac_scale or 0.0),
               "config": np.array(json.dumps(cfg))}
        for k, v in out.items():
            rec[k] = v.numpy().astype(np.float32)
            rec["floor_" + k] = np.float64((v.double() - out64[k]).abs().max())
        # strided samples: hourglass [B,35,h,w] every 7th pixel of every 5th channel, layer4 [B,512,s,s] every 3rd channel
        rec["hourglass_sample"] = taps["hourglass"][:, ::5, ::7, ::7].numpy().astype(np.float32)
        rec["layer4_sample"] = taps["layer4"][:, ::3].numpy().astype(np.float32)
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **rec)
        print(name, {k: float(rec["floor_" + k]) for k in out}, {k: float(v.abs().max()) for k, v in out.items()})


if __name__ == "__main__":
    main()
