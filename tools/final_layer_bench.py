#!/usr/bin/env python
"""The final 7x7 layer (64 -> 3, + sigmoid) alone: eamm_op_conv tile 4002 = the fused column-patch kernel as the engine runs it
(split-bf16 products) beside tile 4003 = the same with fp32-MFMA products, timed with HIP events (20 launches).  Run once per
environment setting (the knob is read once per process; the diagnostic build's fp32 kernels honour it):
    EAMM_COL7_DBG=0|1|2|3   python tools/final_layer_bench.py [--tiles 4002,4003] [frames ...]"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eamm_amd import _lib  # noqa: E402
# diagnostics that compute wrong results live in the experiments build only (make -C eamm_amd/csrc EXPERIMENTS=1)
_exp = os.path.join(os.path.dirname(_lib.LIB_PATH), "libeamm_hip_exp.so")
if os.path.exists(_exp):
    _lib.LIB_PATH = _exp

argv = sys.argv[1:]
tiles = [4002, 4003]
if argv and argv[0] == "--tiles":
    tiles = [int(t) for t in argv[1].split(",")]
    argv = argv[2:]
L = _lib.lib()
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
tag = f"EAMM_COL7_DBG={os.environ['EAMM_COL7_DBG']}" if "EAMM_COL7_DBG" in os.environ else "default"
for B in [int(a) for a in argv] or [8, 16]:
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 256, 256, 64, generator=g).to(dev)
    w = (torch.randn(3, 64, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5).contiguous()
    b = torch.randn(3, generator=g) * 0.1
    ref = torch.sigmoid(torch.nn.functional.conv2d(x[:1].permute(0, 3, 1, 2).cpu(), w, b, padding=3))
    for tile in tiles:
        out = torch.empty(B, 3, 256, 256, device=dev)
        ms = C.c_float()
        _lib.check(L.eamm_op_conv(0, x.data_ptr(), 64, None, 0, B, 256, 256, 0, w.data_ptr(), b.data_ptr(), 3, 7, 7, 2, 0, None, 0, tile,
                                  out.data_ptr(), 20, C.byref(ms), st), None)
        err = float((out[:1].cpu() - ref).abs().max())
        algo = 2.0 * B * 256 * 256 * 3 * 64 * 49
        print(f"[{tag}] final layer, tile {tile}, {B} frames: {ms.value * 1e3:8.1f} us  {algo / ms.value / 1e9:6.1f} TF/s algorithmic  "
              f"max|hip - torch| {err:.2e}", flush=True)
