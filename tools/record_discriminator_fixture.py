#!/usr/bin/env python
"""Record tests/golden/disc_tiny.npz from the reference's own MultiScaleDiscriminator (modules/discriminator.py), on the CPU.

    python tools/record_discriminator_fixture.py --reference /path/to/EAMM [--out tests/golden/disc_tiny.npz]

The reference module is imported from its checkout (nothing of it is copied); third-party modules that its package imports at load
time but the discriminator never calls (cv2, ...) are replaced by empty stand-ins when they are not installed.  The network has the
shipped ``discriminator_params`` (scales [1], block_expansion 32, max_features 512, num_blocks 4, sn True), is in .train() (one
power iteration per forward, so that sigma is well conditioned whatever u and v start as) and sees one batch [2,3,80,72].

Recorded: the input and, from the reference module run in FLOAT64 (rounded once to fp32 for the file), feature maps 1..3, every
fourth channel of feature map 0, the prediction map and the image gradient of ``((1 - p)^2).mean() + sum_i |f_i|.mean()``; beside
each, ``aten_<name>``: the distance of the same module run in fp32 (ATen) from the float64 run, as a fraction of the tensor's scale.  The state dict (11 MB at these widths) is recorded as ``weight_seed``:
tests/discriminator_common.py's ``fixture_state(seed)`` rebuilds it bit for bit, as the other fixtures of this repository do, and ``state_checksum`` of the rebuilt
tensors is recorded so that a changed generator stream shows as such."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PARAMS = dict(scales=[1], block_expansion=32, max_features=512, num_blocks=4, sn=True)
SHAPE = (2, 3, 80, 72)
WEIGHT_SEED, INPUT_SEED = 20, 21
MAP0_STRIDE = 4


def import_reference(path):
    sys.path.insert(0, path)
    for _ in range(32):
        try:
            return importlib.import_module("modules.discriminator")
        except ModuleNotFoundError as e:
            name = e.name or ""
            if not name or os.path.exists(os.path.join(path, *name.split("."))) or os.path.exists(os.path.join(path, *name.split(".")) + ".py"):
                raise
            sys.modules[name] = types.ModuleType(name)      # not installed, and not called by the discriminator
            print(f"stand-in for the missing module {name!r}")
    raise RuntimeError("too many missing modules")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "disc_tiny.npz"))
    args = ap.parse_args()
    from discriminator_common import fixture_state, module_loss, state_checksum
    ref = import_reference(os.path.abspath(args.reference))
    sd = fixture_state(WEIGHT_SEED)
    x0 = torch.rand(*SHAPE, generator=torch.Generator().manual_seed(INPUT_SEED))

    def run(dtype):
        torch.manual_seed(0)
        net = ref.MultiScaleDiscriminator(**PARAMS)
        assert sorted(sd) == sorted(net.state_dict()), "the recipe's keys are the reference module's"
        net.load_state_dict(sd, strict=True)
        net = net.to(dtype).train()
        x = x0.clone().to(dtype).requires_grad_()
        out = net({"prediction_1": x})
        maps, pred = out["feature_maps_1"], out["prediction_map_1"]
        module_loss(maps, pred).backward()
        got = {f"feature_map_{i}": (m.detach()[:, ::MAP0_STRIDE].contiguous() if i == 0 else m.detach()) for i, m in enumerate(maps)}
        got.update(prediction_map=pred.detach(), image_grad=x.grad)
        return got

    r64, r32 = run(torch.float64), run(torch.float32)
    rec = dict(weight_seed=np.int64(WEIGHT_SEED), map0_stride=np.int64(MAP0_STRIDE), x=x0.numpy(),
               state_checksum=np.float64(state_checksum(sd)))
    for k, v in r64.items():
        rec[k] = v.float().numpy()                                     # the float64 result, rounded once to fp32
        rec["aten_" + k] = np.float64(float((r32[k].double() - v).abs().max()) / float(v.abs().max()))   # ATen fp32's distance, of scale
    np.savez(args.out, **rec)
    print(args.out, os.path.getsize(args.out), "bytes;", {k: v.shape for k, v in rec.items()})


if __name__ == "__main__":
    main()
