"""Training fixture of the emotion detector (tests/golden/emotion_tiny128_train_backward.npz), on the CPU from the reference itself.

Imports the reference's Emotion_k read-only (tools/make_emotion_golden.py's stub-cv2 import), loads the seeded synthetic weights of
``emotion_tiny128`` strictly, and runs ONE training-mode forward + backward in float64 and in float32: ``.train()``, every
parameter, the image and the key points requiring a gradient, loss = sum(out * w) over ``value``, ``jacobian``, ``fake`` (in that
order) with w ~ N(0, 1) from ``torch.Generator().manual_seed(3)``.  Writes DATA only:

* ``out/<name>``               the float64 outputs, ``floor/<name>`` the reference's own fp32-vs-fp64 distance per output;
* ``grad/<tensor>``            the float64 gradient of every parameter that gets one, of ``input/image``, ``input/value`` and
                               ``input/jacobian``: at most 2048 strided samples of the flattened tensor (``stride/<tensor>``), with
                               ``gmax/<tensor>`` = the whole tensor's largest entry and ``dist/<tensor>`` = the whole tensor's
                               fp32-vs-fp64 distance (the reference's own rounding error: what the tests' bars start from);
* ``no_grad``                  the parameters the forward never touches (their ``.grad`` stays None);
* ``buf/<name>``               the BatchNorm buffers after the step (float64 run), sampled the same way (``bstride/<name>``).

Images and key points are regenerated from their seeds by the tests.  Usage: python tools/make_emotion_train_golden.py [reference checkout]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from eamm_amd.config import emotion_detector_config  # noqa: E402
from eamm_amd.weights import emotion_state_dict_spec, synthetic_state_dict  # noqa: E402
from make_emotion_golden import CASES, GOLDEN, WEIGHT_SEED, IMAGE_SEED, KP_SEED, case_inputs, import_reference  # noqa: E402

NAME, LOSS_SEED, MAX_SAMPLES = "emotion_tiny128", 3, 2048


def sample(t: torch.Tensor):
    flat = t.detach().double().reshape(-1)
    stride = max(1, -(-flat.numel() // MAX_SAMPLES))
    return flat[::stride].numpy().copy(), np.int64(stride)


def step(Emotion_k, cfg, sd, x, kp, dtype):
    m = Emotion_k(**cfg).train().to(dtype)
    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    leaves = {"image": x.to(dtype).requires_grad_(), "value": kp["value"].to(dtype).requires_grad_(),
              "jacobian": kp["jacobian"].to(dtype).requires_grad_()}
    k, fake = m(leaves["image"], leaves["value"], leaves["jacobian"])
    out = {"value": k["value"], "jacobian": k["jacobian"], "fake": fake}
    g = torch.Generator().manual_seed(LOSS_SEED)
    loss = sum((out[n] * torch.randn(out[n].shape, generator=g).to(dtype)).sum() for n in ("value", "jacobian", "fake"))
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    grads.update({"input/" + n: t.grad for n, t in leaves.items()})
    bufs = {n: b for n, b in m.named_buffers() if n.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    return out, grads, bufs


def main():
    ref_path = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EAMM_REFERENCE", "reference")
    Emotion_k = import_reference(ref_path)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    over, size, frames, jac_scale = CASES[NAME]
    cfg = {**emotion_detector_config(), **over}
    sd = synthetic_state_dict(cfg, seed=WEIGHT_SEED, spec=emotion_state_dict_spec(cfg))
    x, kp = case_inputs(size, frames, jac_scale)
    o64, g64, b64 = step(Emotion_k, cfg, sd, x, kp, torch.float64)
    o32, g32, _ = step(Emotion_k, cfg, sd, x, kp, torch.float32)
    rec = {"weight_seed": np.int64(WEIGHT_SEED), "image_seed": np.int64(IMAGE_SEED), "kp_seed": np.int64(KP_SEED), "loss_seed": np.int64(LOSS_SEED),
           "size": np.int64(size), "frames": np.int64(frames), "config": np.array(json.dumps(cfg)),
           "no_grad": np.array(json.dumps(sorted(n for n, v in g64.items() if v is None)))}
    for n, v in o64.items():
        rec["out/" + n] = v.detach().numpy()
        rec["floor/" + n] = np.float64((o32[n].detach().double() - v.detach()).abs().max())
    worst, gall = 0.0, max(float(v.abs().max()) for v in g64.values() if v is not None)
    for n, v in g64.items():
        if v is None:
            assert g32[n] is None, n
            continue
        rec["grad/" + n], rec["stride/" + n] = sample(v)
        rec["gmax/" + n] = np.float64(v.abs().max())
        rec["dist/" + n] = np.float64((g32[n].double() - v).abs().max())
        # (a gradient that is zero by construction -- a convolution bias in front of batch statistics -- on the largest tensor's scale)
        scale = float(rec["gmax/" + n]) if float(rec["gmax/" + n]) >= 1e-9 * gall else gall
        worst = max(worst, float(rec["dist/" + n]) / scale)
    for n, v in b64.items():
        rec["buf/" + n], rec["bstride/" + n] = sample(v)
    path = os.path.join(GOLDEN, NAME + "_train_backward.npz")
    np.savez_compressed(path, **rec)
    print(NAME, "tensors with a gradient:", sum(v is not None for v in g64.values()), "without:", json.loads(str(rec["no_grad"])))
    print("largest fp32-vs-fp64 distance of a gradient, relative to its tensor's largest entry:", worst)
    print({k: float(rec["floor/" + k]) for k in o64}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
