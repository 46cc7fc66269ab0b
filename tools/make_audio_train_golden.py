"""Training fixtures of the audio network AT_net2 (tests/golden/audio_train_backward.npz, audio_eval_backward.npz), on the CPU from the
reference itself.

Imports the reference's AT_net2 read-only (tools/make_audio_golden.py's stub-cv2 import and its ``.cuda()`` identity patch), loads
the seeded synthetic weights strictly and runs ONE forward(..., 'cnn', 1.6) + backward per mode (``.train()`` and ``.eval()``) in
float64 and in float32: 2 clips of 3 steps, every parameter, the image, ``audio`` and ``pose`` requiring a gradient,
loss = sum(deco_out * w) with w ~ N(0, 1) from ``torch.Generator().manual_seed(3)``.  Writes DATA only, per mode:

* ``out/deco_out``, ``out/lstm_out``   the float64 outputs, at most 2048 strided samples of the flattened tensor (``ostride/<name>``), and
                               ``floor/<name>`` = the reference's own fp32-vs-fp64 distance over the whole tensor;
* ``grad/<tensor>``            the float64 gradient of every parameter that gets one and of ``input/image``, ``input/audio``,
                               ``input/pose``, sampled the same way (``stride/<tensor>``), with ``gmax/<tensor>`` = the whole tensor's
                               largest entry and ``dist/<tensor>`` = the whole tensor's fp32-vs-fp64 distance (the reference's own
                               rounding error: what the tests' bars start from);
* ``no_grad``                  the parameters the forward never touches (``generator.*``: their ``.grad`` stays None);
* ``buf/<name>``               (training file only) every BatchNorm buffer after the step (float64 run), sampled (``bstride/<name>``).

The tool asserts that the reference's own fp32 run passes the tests' rule for the gradients (check_rule).  The inputs are
regenerated from their seeds by the tests.  Usage: python tools/make_audio_train_golden.py [reference checkout]
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
from eamm_amd.weights import audio_feature_state_dict_spec, synthetic_audio_inputs, synthetic_state_dict  # noqa: E402
from make_audio_golden import GOLDEN, INPUT_SEED, WEIGHT, WEIGHT_SEED, import_reference  # noqa: E402

CLIPS, STEPS, LOSS_SEED, MAX_SAMPLES = 2, 3, 3, 2048
FP32_MIN_REL = 5e-3       # tests/test_train_backward.py


def sample(t: torch.Tensor):
    flat = t.detach().double().reshape(-1)
    stride = max(1, -(-flat.numel() // MAX_SAMPLES))
    return flat[::stride].numpy().copy(), np.int64(stride)


def check_rule(got: np.ndarray, want: np.ndarray, dist: float, scale: float, what: str):
    """tests/test_gpu_emotion_backward.py's rule for a module's gradient: per-tensor bar max(4 dist, FP32_MIN_REL scale); at most
    max(2, n // 200) samples beyond it (one below 400 samples), none beyond 20 bars."""
    bar = max(4.0 * dist, FP32_MIN_REL * scale)
    err = np.abs(got - want)
    allowed = max(2, err.size // 200) if err.size >= 400 else 1
    assert int((err > bar).sum()) <= allowed and float(err.max(initial=0.0)) <= 20 * bar, (what, float(err.max()), bar)


def step(AT_net2, sd, image, audio, pose, dtype, train: bool):
    torch.set_default_dtype(dtype)     # the reference's zero LSTM state takes the default dtype (util.py:581)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self   # util.py:581 moves the zero state with .cuda(); identity while it runs
    try:
        m = AT_net2().to(dtype)
        m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
        m.train(train)
        taps = {}
        m.lstm.register_forward_hook(lambda mod, i, o: taps.__setitem__("lstm_out", o[0]))
        leaves = {n: v.detach().clone().to(dtype).requires_grad_() for n, v in (("image", image), ("audio", audio), ("pose", pose))}
        deco = m(leaves["image"], leaves["audio"], leaves["pose"], "cnn", WEIGHT)
        if isinstance(deco, (list, tuple)):
            deco = torch.stack(list(deco), dim=1)
        g = torch.Generator().manual_seed(LOSS_SEED)
        (deco * torch.randn(deco.shape, generator=g, dtype=torch.float32).to(dtype)).sum().backward()
        grads = {n: p.grad for n, p in m.named_parameters()}
        grads.update({"input/" + n: t.grad for n, t in leaves.items()})
        bufs = {n: b for n, b in m.named_buffers() if n.endswith(("running_mean", "running_var", "num_batches_tracked"))}
        return {"deco_out": deco.detach(), "lstm_out": taps["lstm_out"].detach()}, grads, bufs
    finally:
        torch.Tensor.cuda = cuda
        torch.set_default_dtype(torch.float32)


def main():
    ref_path = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EAMM_REFERENCE", "reference")
    AT_net2 = import_reference(ref_path)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = synthetic_state_dict(None, seed=WEIGHT_SEED, spec=audio_feature_state_dict_spec())
    image, audio, pose = synthetic_audio_inputs(CLIPS, STEPS, seed=INPUT_SEED)
    for mode, train in (("train", True), ("eval", False)):
        o64, g64, b64 = step(AT_net2, sd, image, audio, pose, torch.float64, train)
        o32, g32, _ = step(AT_net2, sd, image, audio, pose, torch.float32, train)
        rec = {"weight_seed": np.int64(WEIGHT_SEED), "input_seed": np.int64(INPUT_SEED), "loss_seed": np.int64(LOSS_SEED),
               "clips": np.int64(CLIPS), "steps": np.int64(STEPS), "weight": np.float64(WEIGHT),
               "no_grad": np.array(json.dumps(sorted(n for n, v in g64.items() if v is None)))}
        for n, v in o64.items():
            rec["out/" + n], rec["ostride/" + n] = sample(v)
            rec["floor/" + n] = np.float64((o32[n].double() - v).abs().max())
        worst, rms = 0.0, 0.0
        gall = max(float(v.abs().max()) for v in g64.values() if v is not None)
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
            rms = max(rms, float((g32[n].double() - v).pow(2).mean().sqrt()) / scale)
            check_rule(sample(g32[n])[0], rec["grad/" + n], float(rec["dist/" + n]), scale, n)
        if train:
            for n, v in b64.items():
                rec["buf/" + n], rec["bstride/" + n] = sample(v)
        path = os.path.join(GOLDEN, f"audio_{mode}_backward.npz")
        np.savez_compressed(path, **rec)
        print(mode, "tensors with a gradient:", sum(v is not None for v in g64.values()), "without:", sum(v is None for v in g64.values()))
        print("  largest fp32-vs-fp64 distance of a gradient, relative to its tensor's largest entry:", worst, " largest relative RMS:", rms)
        print("  ", {k: float(rec["floor/" + k]) for k in o64}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
