"""Drop-in ``KPDetector`` / ``KPDetector_a`` whose forward passes run in libeamm_hip.so.

Mirrors reference modules/keypoint_detector.py: same constructor keywords (``demo.py:59-72`` splats
``kp_detector_params`` with ``common_params`` / ``audio_params``), same ``state_dict`` keys, same output dict
(``value`` [B,K,2], ``heatmap`` [B,K,h-6,w-6], ``jacobian`` [B,K,2,2]).  ``KPDetector.forward(image)`` runs
anti-alias down-sampling + hourglass + heads (once per clip on the source, demo.py:206); ``KPDetector_a.
forward(feature_map)`` runs only the heads on the audio-driven feature map (once per frame, demo.py:219) -- its
``predictor`` hourglass is part of the checkpoint but unused by the reference's forward, and here too.
The sub-modules only hold parameters; there is no PyTorch fallback.

Training.  The parameters are frozen at construction, and a frozen detector in ``.eval()`` runs the graph-free inference engine.
``mod.requires_grad_(True)`` opts into training (reference modules/model.py:187-279 trains ``kp_extractor_a`` against
``kp_extractor``; ``GeneratorFullModel`` back-propagates the reconstruction loss into the detector): ``forward`` is
differentiable exactly when gradients are enabled and the input or a parameter requires one, or when the module is in
``.train()`` -- the rule of ``OcclusionAwareGenerator.forward``.  It is then the composition of differentiable HIP operators:
``motion_ops.antialias_down``, ``train_graph._Graph.hourglass`` (convolutions and BatchNorm + ReLU, batch statistics and
running-statistics updates in ``.train()``, running statistics in ``.eval()``), ONE 7x7 convolution with the ``kp`` and
``jacobian`` filters stacked, and ``kp_ops.kp_head`` (softmax / soft-argmax / jacobian reduction, HIP forward and backward).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from ._handle import HandleOwner, ptr, stream_ptr, weights_key
from .generator import _AntiAlias, _ConvNorm, _Stack
from .weights import hourglass_channels



class _KPBase(HandleOwner, nn.Module):
    _prefix = "eamm_kp_"
    _with_predictor = True

    def __init__(self, block_expansion, num_kp, num_channels, max_features, num_blocks, temperature,
                 estimate_jacobian=False, scale_factor=1, single_jacobian_map=False, pad=0, in_features=None,
                 max_batch=16):
        super().__init__()
        in_features = num_channels if in_features is None else in_features
        enc, dec, out_filters = hourglass_channels(block_expansion, in_features, num_blocks, max_features)
        pred = nn.Module()
        pred.encoder = _Stack("down_blocks", [_ConvNorm(ci, co, 3) for ci, co in enc])
        pred.decoder = _Stack("up_blocks", [_ConvNorm(ci, co, 3) for ci, co in dec])
        self.predictor = pred
        self.kp = nn.Conv2d(out_filters, num_kp, kernel_size=(7, 7), padding=pad)
        if estimate_jacobian:
            self.num_jacobian_maps = 1 if single_jacobian_map else num_kp
            self.jacobian = nn.Conv2d(out_filters, 4 * self.num_jacobian_maps, kernel_size=(7, 7), padding=pad)
            self.jacobian.weight.data.zero_()      # reference init: identity jacobians (keypoint_detector.py:27-28)
            self.jacobian.bias.data.copy_(torch.tensor([1, 0, 0, 1] * self.num_jacobian_maps, dtype=torch.float))
        else:
            self.jacobian = None
        self.temperature, self.scale_factor = temperature, scale_factor
        if scale_factor != 1:
            self.down = _AntiAlias(num_channels)
        self._cfg = dict(num_kp=num_kp, num_channels=num_channels, in_features=in_features,
                         block_expansion=block_expansion, max_features=max_features, num_blocks=num_blocks,
                         temperature=float(temperature), estimate_jacobian=int(bool(estimate_jacobian)),
                         single_jacobian_map=int(bool(single_jacobian_map)),
                         inv_scale=int(round(1.0 / scale_factor)), pad=int(pad))
        self.out_filters = out_filters
        self.max_batch = int(max_batch)
        # what train_graph._Graph reads for the BatchNorms' replicas (as OcclusionAwareGenerator: None = one process's statistics)
        self.process_group = None
        self.sync_batchnorm: Optional[bool] = None
        for p in self.parameters():          # frozen: training is opted into with mod.requires_grad_(True)
            p.requires_grad_(False)

    # -- handle management ----------------------------------------------------------------------------------
    def _ensure(self, height: int, width: int, batch: int):
        dev = self._inference_device(self.kp.weight)
        needed = ("kp.", "jacobian.") + (("predictor.", "down.") if self._with_predictor else ())
        named = [(name, t) for name, t in self.state_dict(keep_vars=True).items() if name.startswith(needed)]
        key = (dev, height, width, weights_key(t for _, t in named))
        if self._has_handle(key, batch):
            return
        cs = _lib.EammKpConfig(**self._cfg)
        cs.height, cs.width = int(height), int(width)
        cs.max_batch = max(batch, self.max_batch)
        cs.with_predictor = int(self._with_predictor)
        self._rebuild_handle(key, cs.max_batch, cs, dev, named)

    # -- differentiable path --------------------------------------------------------------------------------
    def _wants_graph(self, x: torch.Tensor) -> bool:
        """OcclusionAwareGenerator.forward's rule: ``.train()`` (batch statistics are the training composition's, with or without
        gradients), or gradients enabled and the input or a parameter requiring one."""
        if self.training:
            return True
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _heads_graph(self, feat_nhwc: torch.Tensor) -> Dict[str, torch.Tensor]:
        """keypoint_detector.py:86-103 on NHWC features: the ``kp`` and ``jacobian`` 7x7 convolutions read the same features, so they
        run as ONE "same"-padded convolution with the filters stacked (as the flow head's mask + occlusion in ``train_graph``; autograd
        splits the stacked gradient back onto the two modules); ``pad`` only moves the window ``kp_head`` reads."""
        from . import kp_ops, train_graph
        k = self._cfg["num_kp"]
        njm = self.num_jacobian_maps if self.jacobian is not None else 0
        w, b = self.kp.weight, self.kp.bias
        if njm:
            w, b = torch.cat([w, self.jacobian.weight], dim=0), torch.cat([b, self.jacobian.bias])
        logits = train_graph.conv_wb(feat_nhwc, w, b, keep_padded=True)
        return kp_ops.kp_head(logits, k, njm, self._cfg["pad"], self.temperature, want_heatmap=self._want_heatmap)

    def _need_gpu(self, x: torch.Tensor):
        if self.kp.weight.device.type != "cuda" or x.device.type != "cuda":
            raise RuntimeError(f"eamm_amd.{type(self).__name__} runs only on a ROCm GPU (no CPU fallback): call .cuda()")

    _want_heatmap = True      # detect(..., heatmap=False) clears it for one call: the clip harness never reads the heat-maps (demo.py:219-281)

    def detect(self, x, heatmap: bool = True) -> Dict[str, torch.Tensor]:
        """``forward`` with the heat-maps optional: ``heatmap=False`` returns {'value', 'jacobian'} only and skips the heat-map pass
        (K x 58 x 58 floats per frame written for nobody: ``demo.py`` never reads them; ``driving_keypoints`` calls this)."""
        self._want_heatmap = bool(heatmap)
        try:
            return self(x)
        finally:
            self._want_heatmap = True

    def _outputs(self, b: int, hm_h: int, hm_w: int, dev):
        """The output dict of one call and the ``EammKpOutputs`` that points into it."""
        k = self._cfg["num_kp"]
        out = {"value": torch.empty(b, k, 2, device=dev)}
        if self._want_heatmap:
            out["heatmap"] = torch.empty(b, k, hm_h, hm_w, device=dev)
        if self.jacobian is not None:
            out["jacobian"] = torch.empty(b, k, 2, 2, device=dev)
        return out, _lib.EammKpOutputs(**{name: t.data_ptr() for name, t in out.items()})

    def _run(self, x: torch.Tensor, fn_name: str, hm_h: int, hm_w: int) -> Dict[str, torch.Tensor]:
        out, o = self._outputs(x.shape[0], hm_h, hm_w, x.device)
        self._handle.call(fn_name, ptr(x), x.shape[0], C.byref(o), stream_ptr(x.device))
        return out


class KPDetector(_KPBase):
    """reference keypoint_detector.py:7-105"""

    _with_predictor = True

    def __init__(self, block_expansion, num_kp, num_channels, max_features, num_blocks, temperature,
                 estimate_jacobian=False, scale_factor=1, single_jacobian_map=False, pad=0, max_batch=16):
        super().__init__(block_expansion, num_kp, num_channels, max_features, num_blocks, temperature,
                         estimate_jacobian, scale_factor, single_jacobian_map, pad, None, max_batch)

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """A frozen detector in ``.eval()`` (the state after construction) runs the inference engine and returns tensors without
        a graph.  After ``requires_grad_(True)`` (or with an input that requires a gradient, or in ``.train()``) the outputs carry
        an autograd graph through HIP operators, as the reference module's do."""
        if self._wants_graph(x):
            return self._forward_graph(x)
        with torch.no_grad():
            return self._forward(x)

    def _check_image(self, x: torch.Tensor):
        nc = self._cfg["num_channels"]
        if x.dim() != 4 or x.shape[1] != nc or x.dtype != torch.float32:
            raise RuntimeError(f"expected a float32 [B,{nc},H,W] image batch, got {tuple(x.shape)} {x.dtype}")

    def _forward_graph(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        from . import motion_ops, train_graph
        self._check_image(x)
        self._need_gpu(x)
        inv = self._cfg["inv_scale"]
        if x.shape[1] == 3 and abs(1.0 / self.scale_factor - inv) < 1e-6 and inv in (1, 4) and x.shape[2] % inv == 0 and x.shape[3] % inv == 0:
            # NHWC [B,h,w,4] = RGB + a zero channel; the hourglass's last concatenation wants the three real ones
            small = motion_ops.antialias_down(x, self.down.weight if self.scale_factor != 1 else None, self.scale_factor)[..., :3]
        else:
            small = (train_graph._antialias_down(x, self.down.weight, self.scale_factor) if self.scale_factor != 1 else x).permute(0, 2, 3, 1)
        return self._heads_graph(train_graph._Graph(self).hourglass(small, self.predictor))

    def _forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        self._check_image(x)
        b, _, hh, ww = x.shape
        self._ensure(hh, ww, b)
        inv, pad = self._cfg["inv_scale"], self._cfg["pad"]
        return self._run(x.contiguous(), "detect", hh // inv - 6 + 2 * pad, ww // inv - 6 + 2 * pad)


class KPDetector_a(_KPBase):
    """reference keypoint_detector.py:110-205 (forward takes the feature map, not an image)"""

    _with_predictor = False

    def __init__(self, block_expansion, num_kp, num_channels, num_channels_a, max_features, num_blocks, temperature,
                 estimate_jacobian=False, scale_factor=1, single_jacobian_map=False, pad=0, max_batch=16):
        super().__init__(block_expansion, num_kp, num_channels, max_features, num_blocks, temperature,
                         estimate_jacobian, scale_factor, single_jacobian_map, pad, num_channels_a, max_batch)

    def forward(self, feature_map) -> Dict[str, torch.Tensor]:
        """``feature_map``: the reference's float32 [B, C, h, w] tensor, or (round 6) the ``SplitFeatureMap`` ``DeconvTail.forward_split``
        hands over (same values, the layout the heads read)."""
        if self._wants_graph(feature_map if torch.is_tensor(feature_map) else feature_map.wide):
            return self._forward_graph(feature_map)
        with torch.no_grad():
            return self._forward(feature_map)

    def _forward_graph(self, feature_map) -> Dict[str, torch.Tensor]:
        """The heads on the given feature map with an autograd graph (the unused ``predictor`` gets no gradient, as in the reference)."""
        if not torch.is_tensor(feature_map) and hasattr(feature_map, "to_nchw"):
            feature_map = feature_map.to_nchw()
        self._check_features(feature_map)
        self._need_gpu(feature_map)
        return self._heads_graph(feature_map.permute(0, 2, 3, 1))

    def _check_features(self, feature_map):
        if feature_map.dim() != 4 or feature_map.shape[1] != self.out_filters or feature_map.dtype != torch.float32:
            raise RuntimeError(f"expected a float32 [B,{self.out_filters},h,w] feature map, got "
                               f"{tuple(feature_map.shape)} {feature_map.dtype}")

    def accepts_split(self, height: int, width: int, batch: int = 1) -> int:
        """``wide`` channel count of the split feature map these heads read directly (``DeconvTail.forward_split``), 0 if they do
        not run in the wide + thin form (round 6: the private NHWC hand-over).  Builds the handle for (height, width) maps."""
        inv = self._cfg["inv_scale"]
        self._ensure(height * inv, width * inv, batch)
        return int(_lib.lib().eamm_kp_split_channels(self._handle.ptr))

    def _forward(self, feature_map) -> Dict[str, torch.Tensor]:
        if not torch.is_tensor(feature_map) and hasattr(feature_map, "wide") and hasattr(feature_map, "thin"):
            return self._forward_split(feature_map)
        self._check_features(feature_map)
        b, _, h, w = feature_map.shape
        inv, pad = self._cfg["inv_scale"], self._cfg["pad"]
        self._ensure(h * inv, w * inv, b)
        return self._run(feature_map.contiguous(), "detect_features", h - 6 + 2 * pad, w - 6 + 2 * pad)

    def _forward_split(self, fm) -> Dict[str, torch.Tensor]:
        b, c, h, w = fm.shape
        if c != self.out_filters:
            raise RuntimeError(f"expected a split [B,{self.out_filters},h,w] feature map, got {tuple(fm.shape)}")
        inv, pad = self._cfg["inv_scale"], self._cfg["pad"]
        self._ensure(h * inv, w * inv, b)
        if int(_lib.lib().eamm_kp_split_channels(self._handle.ptr)) != c - 3:
            return self._forward(fm.to_nchw())          # heads not in the wide + thin form: the reference's tensor
        wide, thin = fm.wide.contiguous(), fm.thin.contiguous()
        out, o = self._outputs(b, h - 6 + 2 * pad, w - 6 + 2 * pad, wide.device)
        self._handle.call("detect_features_split", ptr(wide), ptr(thin), b, C.byref(o), stream_ptr(wide.device))
        return out
