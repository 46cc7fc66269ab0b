"""Drop-in ``Emotion_k`` (reference modules/util.py:1223-1527) whose forward pass runs in libeamm_hip.so.

The reference's emotional pass (``demo.py:221-228``, ``--type linear_3``) calls ``emo_detector(frame, value, jacobian)`` and
``emo_detector.feature(frame)`` once per frame of the emotion video; both run the same anti-alias + hourglass + ResNet-18 trunk.
Here one ``eamm_emo_detect`` call computes the trunk once for a whole batch of frames and returns every output
(``detect``).  Same constructor keywords, same ``state_dict`` keys (the 223 entries of the reference, including the unused
``fc``, ``fc_n``, ``final_4`` and ``final_10``), same outputs.  The sub-modules only hold parameters; there is no PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import torch
from torch import nn

from . import _lib
from ._handle import HandleOwner, ptr, refuse_silent_detach, stream_ptr, weights_key
from .generator import _AntiAlias, _ConvNorm, _Stack
from .weights import hourglass_channels

NUM_KP = 10          # fc_p takes 10 x 126 embedded numbers (util.py:1251)
FEATURE = 512


class _BasicBlock(nn.Module):
    """Parameter holder named like BasicBlock (util.py:1069-1082)."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))


class _Classify(nn.Module):
    def __init__(self):
        super().__init__()
        self.last_fc = nn.Linear(512, 8)   # util.py:312: eight classes, whatever Emotion_k's num_classes


class EmotionDetector(HandleOwner, nn.Module):
    """reference util.py:1223 ``Emotion_k`` (forward = util.py:1498-1527, feature = :1477-1496), inference only."""
    _prefix = "eamm_emo_"

    def __init__(self, block_expansion, num_channels, max_features, num_blocks, scale_factor=1, num_classes=8, max_batch=64):
        super().__init__()
        inv = int(round(1.0 / scale_factor)) if scale_factor > 0 else 0
        if inv not in (1, 2, 4) or abs(inv * scale_factor - 1.0) > 1e-9:
            raise ValueError(f"EmotionDetector: scale_factor must be 1, 0.5 or 0.25 (got {scale_factor})")
        enc, dec, out_filters = hourglass_channels(block_expansion, num_channels, num_blocks, max_features)
        pred = nn.Module()
        pred.encoder = _Stack("down_blocks", [_ConvNorm(ci, co, 3) for ci, co in enc])
        pred.decoder = _Stack("up_blocks", [_ConvNorm(ci, co, 3) for ci, co in dec])
        self.predictor = pred
        self.scale_factor = scale_factor
        if scale_factor != 1:
            self.down = _AntiAlias(num_channels)
        self.conv1 = nn.Conv2d(out_filters, 64, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, planes in enumerate((64, 128, 256, 512)):
            stride = 1 if i == 0 else 2
            setattr(self, f"layer{i + 1}", nn.Sequential(_BasicBlock(cin, planes, stride), _BasicBlock(planes, planes, 1)))
            cin = planes
        self.fc = nn.Linear(512, num_classes)
        self.fc_p = nn.Sequential(nn.Linear(NUM_KP * 126, 1024), nn.ReLU(True), nn.Linear(1024, 512), nn.ReLU(True))
        self.fc_n = nn.Sequential(nn.Linear(NUM_KP * 6, 128), nn.ReLU(True), nn.Linear(128, 512), nn.ReLU(True))
        self.fc_all = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(True), nn.Linear(512, 256), nn.ReLU(True), nn.Linear(256, 64),
                                    nn.ReLU(True))
        self.final = nn.Sequential(nn.Conv1d(1, 2, 4, 2, 1), nn.MaxPool1d(2, stride=2), nn.ReLU(True), nn.Conv1d(2, 4, 4, 2, 1),
                                   nn.ReLU(True), nn.Conv1d(4, 4, 3))
        self.final_4 = nn.Sequential(nn.Conv1d(4, 4, 3, 1, 1), nn.MaxPool1d(2, stride=2), nn.ReLU(True), nn.Conv1d(4, 4, 3, 1))
        self.final_10 = nn.Sequential(nn.Conv1d(4, 8, 3, 1, 1), nn.MaxPool1d(2, stride=2), nn.ReLU(True), nn.Conv1d(8, 10, 3, 1))
        self.classify = _Classify()
        self._cfg = dict(block_expansion=int(block_expansion), num_channels=int(num_channels), max_features=int(max_features),
                         num_blocks=int(num_blocks), inv_scale=inv, num_classes=8)
        self.max_batch = int(max_batch)
        for p in self.parameters():
            p.requires_grad_(False)

    # -- handle management ----------------------------------------------------------------------------------
    def _ensure(self, height: int, width: int):
        dev = self._inference_device(self.conv1.weight)
        named = list(self.state_dict(keep_vars=True).items())
        key = (dev, height, width, weights_key(t for _, t in named), self.max_batch)
        if self._has_handle(key):
            return
        cs = _lib.EammEmoConfig(**self._cfg)
        cs.height, cs.width = int(height), int(width)
        cs.max_batch = self.max_batch
        self._rebuild_handle(key, self.max_batch, cs, dev, named)

    # -- forward ----------------------------------------------------------------------------------------------
    def _check_inputs(self, x, value, jacobian):
        nc = self._cfg["num_channels"]
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != nc or x.dtype != torch.float32:
            raise RuntimeError(f"expected a float32 [B,{nc},H,W] image batch, got {tuple(getattr(x, 'shape', ()))} "
                               f"{getattr(x, 'dtype', type(x))}")
        if value is None:
            return
        b = x.shape[0]
        if value.dim() != 3 or value.shape[1] != NUM_KP or value.shape[2] != 2 or value.shape[0] != b:
            raise ValueError(f"EmotionDetector: value must be [B,{NUM_KP},2] (num_kp {NUM_KP}: fc_p takes {NUM_KP} x 126 inputs), "
                             f"got {tuple(value.shape)}")
        if jacobian is None or tuple(jacobian.shape) != (b, NUM_KP, 2, 2):
            raise ValueError(f"EmotionDetector: jacobian must be [B,{NUM_KP},2,2] (num_kp {NUM_KP}), got "
                             f"{None if jacobian is None else tuple(jacobian.shape)}")

    def _detect(self, x, value, jacobian, want: Tuple[str, ...]) -> Dict[str, torch.Tensor]:
        self._check_inputs(x, value, jacobian)
        b, _, hh, ww = x.shape
        self._ensure(hh, ww)
        dev = x.device
        shapes = {"value": (4, 2), "jacobian": (4, 2, 2), "fake": (self._cfg["num_classes"],), "feature": (FEATURE,)}
        out = {k: torch.empty(b, *shapes[k], device=dev) for k in want}
        x = x.contiguous()
        v = value.to(dev, torch.float32).contiguous() if value is not None else None
        j = jacobian.to(dev, torch.float32).contiguous() if jacobian is not None else None
        for s in range(0, b, self._cap):
            e = min(b, s + self._cap)
            o = _lib.EammEmoOutputs(**{k: t[s:e].data_ptr() for k, t in out.items()})
            self._handle.call("detect", ptr(x[s:e]), ptr(v[s:e] if v is not None else None), ptr(j[s:e] if j is not None else None),
                              e - s, C.byref(o), stream_ptr(dev))
        return out

    def detect(self, x: torch.Tensor, value: torch.Tensor, jacobian: torch.Tensor) -> Dict[str, torch.Tensor]:
        """forward and feature in one pass: {'value' [B,4,2], 'jacobian' [B,4,2,2], 'fake' [B,8], 'feature' [B,512]}."""
        refuse_silent_detach(self, x)
        with torch.no_grad():
            return self._detect(x, value, jacobian, ("value", "jacobian", "fake", "feature"))

    def forward(self, x: torch.Tensor, value: torch.Tensor, jacobian: torch.Tensor):
        """util.py:1498-1527 -> ({'value', 'jacobian'}, fake)."""
        refuse_silent_detach(self, x)
        with torch.no_grad():
            out = self._detect(x, value, jacobian, ("value", "jacobian", "fake"))
        return {"value": out["value"], "jacobian": out["jacobian"]}, out["fake"]

    def feature(self, x: torch.Tensor) -> torch.Tensor:
        """util.py:1477-1496 -> [B,512]."""
        refuse_silent_detach(self, x)
        with torch.no_grad():
            return self._detect(x, None, None, ("feature",))["feature"]
