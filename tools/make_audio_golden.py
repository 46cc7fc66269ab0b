"""Fixtures of the audio network AT_net2 (tests/golden/audio_*.npz, audio_keys.json), on the CPU from the reference itself.

Imports the reference's AT_net2 read-only (a stub cv2 on sys.path, as oracle/make_golden.py does), loads the seeded synthetic
weights (eamm_amd.weights.audio_feature_state_dict_spec) strictly, runs forward(..., 'cnn', 1.6) in eval mode in fp32 and again
in fp64 (default dtype float64, so that the reference's zero LSTM state is fp64 too) and writes DATA only: seeds, the LSTM output
(all of it, or every 8th step plus the last for the long clip), a strided sample of deco_out, the reference's own fp32-vs-fp64
distance per output, and lstm_out statistics that show the recurrence is neither saturated nor dead.  The inputs are regenerated
from their seeds by the tests.  Usage: python tools/make_audio_golden.py [reference checkout]
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
from eamm_amd.weights import audio_feature_state_dict_spec, synthetic_audio_inputs, synthetic_state_dict  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED, INPUT_SEED, WEIGHT = 2468, 31, 1.6
LONG_STRIDE = 8

CASES = {
    # name: (clips, steps, full lstm_out, deco_out sample)
    "audio_small": (1, 12, True, True),
    "audio_batch2": (2, 5, True, True),
    "audio_long": (1, 512, False, False),
}


def import_reference(path):
    stub = tempfile.mkdtemp(prefix="cv2stub_")
    open(os.path.join(stub, "cv2.py"), "w").close()
    sys.path[:0] = [stub, path]
    from modules.util import AT_net2  # type: ignore
    return AT_net2


def long_steps(t):
    """the steps audio_long keeps: every LONG_STRIDE-th and the last"""
    return sorted(set(range(0, t, LONG_STRIDE)) | {t - 1})


def run(AT_net2, sd, dtype, image, audio, pose):
    torch.set_default_dtype(dtype)
    try:
        m = AT_net2().eval().to(dtype)
        m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
        taps = {}
        m.lstm.register_forward_hook(lambda mod, i, o: taps.__setitem__("lstm_out", o[0]))
        cuda = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self   # util.py:581 moves the zero state with .cuda(); identity while it runs
        try:
            with torch.no_grad():
                deco = m(image.to(dtype), audio.to(dtype), pose.to(dtype), "cnn", WEIGHT)
        finally:
            torch.Tensor.cuda = cuda
        return taps["lstm_out"], deco
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    ref_path = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EAMM_REFERENCE", "reference")
    AT_net2 = import_reference(ref_path)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = synthetic_state_dict(None, seed=WEIGHT_SEED, spec=audio_feature_state_dict_spec())
    with open(os.path.join(GOLDEN, "audio_keys.json"), "w") as f:
        json.dump([[k, list(v.shape)] for k, v in AT_net2().state_dict().items()], f, indent=0)
        f.write("\n")
    for name, (n, t, full, with_deco) in CASES.items():
        image, audio, pose = synthetic_audio_inputs(n, t, seed=INPUT_SEED)
        lstm32, deco32 = run(AT_net2, sd, torch.float32, image, audio, pose)
        lstm64, deco64 = run(AT_net2, sd, torch.float64, image, audio, pose)
        rec = {"weight_seed": np.int64(WEIGHT_SEED), "input_seed": np.int64(INPUT_SEED), "clips": np.int64(n), "steps": np.int64(t),
               "weight": np.float64(WEIGHT), "floor_lstm_out": np.float64((lstm32.double() - lstm64).abs().max()),
               "lstm_std": np.float64(lstm32.std()), "lstm_saturated": np.float64((lstm32.abs() > 0.99).double().mean())}
        if full:
            rec["lstm_out"] = lstm32.numpy().astype(np.float32)
        else:
            steps = long_steps(t)
            rec["lstm_steps"] = np.array(steps, dtype=np.int64)
            rec["lstm_out"] = lstm32[:, steps].numpy().astype(np.float32)
        if with_deco:
            rec["deco_sample"] = deco32[:, :, ::5, ::7, ::7].numpy().astype(np.float32)
            rec["floor_deco_out"] = np.float64((deco32.double() - deco64).abs().max())
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **rec)
        print(name, {k: float(v) for k, v in rec.items() if k.startswith("floor") or k in ("lstm_std", "lstm_saturated")}, float(lstm32.abs().max()))


if __name__ == "__main__":
    main()
