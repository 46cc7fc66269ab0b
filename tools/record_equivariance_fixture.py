#!/usr/bin/env python
"""Record tests/golden/equivariance_tiny.npz from the reference's own Transform (modules/model.py:71-152), on the CPU.

    python tools/record_equivariance_fixture.py --reference /path/to/EAMM [--out tests/golden/equivariance_tiny.npz]

The reference module is imported from its checkout (nothing of it is copied); third-party modules that its package imports at load
time but ``Transform`` never calls (torchvision, cv2, ...) are replaced by empty stand-ins when they are not installed.

One ``Transform(2, sigma_affine=0.3, sigma_tps=0.02, points_tps=5)`` is drawn under ``torch.manual_seed(TRANSFORM_SEED)`` -- wider
than the shipped sigmas, so that a third of the grid points leave the frame and the reflection rule is exercised.  Recorded, data
only: the seeds and sigmas, its ``theta`` and ``control_params`` (fp32, as drawn); a [2,3,16,24] frame and [2,10,2] coordinates
(fp32) with the weights ``a`` [2,10,2] and ``b`` [2,10,2,2]; and from the reference run in FLOAT64 on those fp32 values
``frame_out`` = transform_frame, ``coords_out`` = warp_coordinates, ``jacobian`` and ``coords_grad`` = the coordinate gradient of
``(out * a).sum() + (jacobian * b).sum()`` (float64 arrays), each with ``<name>_fp32``: the same call in fp32 (ATen).

The reference's ``inverse_warp_coordinates`` (and with it ``inverse_transform_frame``) moves a constant to the GPU with a hard-coded
``.cuda()`` and cannot run on a machine without one: it is NOT recorded.  The tests check the inverse forms against the float64
oracle of tests/equivariance_common.py instead."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BS, POINTS = 2, 5
SIGMA_AFFINE, SIGMA_TPS = 0.3, 0.02
FRAME, COORDS = (BS, 3, 16, 24), (BS, 10, 2)
TRANSFORM_SEED, DATA_SEED = 31, 32


def _empty_class(attr):
    if attr.startswith("__"):
        raise AttributeError(attr)
    return type(attr, (), {})


def import_reference(path):
    sys.path.insert(0, path)
    for _ in range(32):
        try:
            return importlib.import_module("modules.model")
        except ModuleNotFoundError as e:
            name = e.name or ""
            if not name or os.path.exists(os.path.join(path, *name.split("."))) or os.path.exists(os.path.join(path, *name.split(".")) + ".py"):
                raise
            stand_in = types.ModuleType(name)
            stand_in.__path__ = []                               # a package, so that its sub-modules get stand-ins too
            stand_in.__getattr__ = _empty_class                  # `from x import Name`: an empty class, never called
            sys.modules[name] = stand_in
            print(f"stand-in for the missing module {name!r}")
    raise RuntimeError("too many missing modules")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "equivariance_tiny.npz"))
    args = ap.parse_args()
    ref = import_reference(os.path.abspath(args.reference))
    torch.manual_seed(TRANSFORM_SEED)
    tr = ref.Transform(BS, sigma_affine=SIGMA_AFFINE, sigma_tps=SIGMA_TPS, points_tps=POINTS)
    assert tr.theta.dtype == torch.float32 and tuple(tr.control_params.shape) == (BS, 1, POINTS ** 2)
    g = torch.Generator().manual_seed(DATA_SEED)
    frame = torch.rand(*FRAME, generator=g)
    coords = torch.rand(*COORDS, generator=g) * 2.4 - 1.2
    a, b = torch.randn(*COORDS, generator=g), torch.randn(*COORDS, 2, generator=g)

    def run(dtype):
        c = coords.clone().to(dtype)
        jac = tr.jacobian(c)                                     # (sets c.requires_grad itself)
        out = tr.warp_coordinates(c)
        grad, = torch.autograd.grad((out * a.to(dtype)).sum() + (jac * b.to(dtype)).sum(), c)
        return dict(frame_out=tr.transform_frame(frame.clone().to(dtype)), coords_out=out.detach(), jacobian=jac.detach(), coords_grad=grad)

    r64, r32 = run(torch.float64), run(torch.float32)
    rec = dict(transform_seed=np.int64(TRANSFORM_SEED), data_seed=np.int64(DATA_SEED), sigma_affine=np.float64(SIGMA_AFFINE),
               sigma_tps=np.float64(SIGMA_TPS), points_tps=np.int64(POINTS), theta=tr.theta.numpy(),
               control_params=tr.control_params.numpy(), frame=frame.numpy(), coords=coords.numpy(), a=a.numpy(), b=b.numpy())
    for k, v in r64.items():
        assert v.dtype == torch.float64 and r32[k].dtype == torch.float32, k
        rec[k] = v.numpy()
        rec[k + "_fp32"] = r32[k].numpy()
    np.savez(args.out, **rec)
    print(args.out, os.path.getsize(args.out), "bytes;", {k: getattr(v, "shape", ()) for k, v in rec.items()})


if __name__ == "__main__":
    main()
