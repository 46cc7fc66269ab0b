"""Drop-in for the ``decon`` tail of the audio-to-feature network.

The reference's ``AT_net2.decon`` (modules/util.py:559-576) is an ``nn.Sequential`` of five ConvTranspose2d layers
(+ BatchNorm2d + ReLU) that turns one LSTM output vector into the [35,64,64] feature maps ``KPDetector_a`` reads; the
reference calls it once per frame with batch 1 (util.py:604-607).  ``DeconvTail`` is an ``nn.Sequential`` with the same
children indices -- so ``audio_feature.decon = DeconvTail()`` before ``audio_feature.load_state_dict(...)``
(demo.py:93) picks up the checkpoint's ``decon.N.*`` entries unchanged -- whose forward runs in libeamm_hip.so for
any batch, so a whole clip's frames go through in one call.  The children only hold parameters; there is no PyTorch
fallback.

Training.  ``decon`` is part of what the reference's first stage trains (train.py ``train_part1``: the L1 loss on the audio-driven
key points reaches it through ``KPDetector_a``).  The parameters are frozen at construction and a frozen tail runs the graph-free
engine whatever ``.training`` says; ``mod.requires_grad_(True)`` opts in.  ``forward`` is then differentiable when the module is in
``.train()``, or gradients are enabled (a parameter requires one) -- as the composition of differentiable operators: layer 0 (k6 on
a 1x1 map: a linear map of the inner 4x4 taps, a torch matmul; the border taps get a zero gradient, as in the reference),
``audio_ops.conv_transpose4s2_nhwc`` for the other layers (HIP forward, data, weight and bias gradients) and
``train_graph._Graph.norm`` (plain ``nn.BatchNorm2d``: batch statistics and a running-statistics update in ``.train()``, running
statistics in ``.eval()``).  ``forward_split`` stays an inference entry.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from . import _lib
from ._handle import HandleOwner, ptr, refuse_silent_detach, stream_ptr, weights_key
from .weights import DECONV_CHANNELS


class SplitFeatureMap:
    """A [B, 32 m + 3, S, S] feature map in the layout ``KPDetector_a``'s heads read: ``wide`` NHWC [B,S,S,32 m] and ``thin``
    [B,S,S,4] (channels 32 m .. 32 m + 2 and a zero).  Produced by ``DeconvTail.forward_split``, accepted by ``KPDetector_a``."""
    __slots__ = ("wide", "thin")

    def __init__(self, wide: torch.Tensor, thin: torch.Tensor):
        if (wide.dim() != 4 or thin.dim() != 4 or thin.shape[-1] != 4 or wide.shape[:3] != thin.shape[:3] or wide.dtype != torch.float32
                or thin.dtype != torch.float32 or wide.device != thin.device):
            raise RuntimeError(f"SplitFeatureMap: wide {tuple(wide.shape)} / thin {tuple(thin.shape)} do not belong together")
        self.wide, self.thin = wide, thin

    @property
    def shape(self):
        b, h, w, c = self.wide.shape
        return (b, c + 3, h, w)

    @property
    def device(self):
        return self.wide.device

    def to_nchw(self) -> torch.Tensor:
        """The reference's tensor (util.py:604-607 `deco_out[:, t]`): [B, 32 m + 3, S, S]."""
        return torch.cat([self.wide, self.thin[..., :3]], dim=-1).permute(0, 3, 1, 2).contiguous()


class DeconvTail(HandleOwner, nn.Sequential):
    """MI355X-native stand-in for reference modules/util.py:559-576 (``AT_net2.decon``)."""
    _prefix = "eamm_deconv_"

    def __init__(self, channels: Sequence[int] = DECONV_CHANNELS, max_batch: int = 64):
        layers = []
        n = len(channels) - 1
        if not 2 <= n <= 8:
            raise ValueError("between 2 and 8 layers")
        for i in range(n):
            layers.append(nn.ConvTranspose2d(channels[i], channels[i + 1], kernel_size=6 if i == 0 else 4, stride=2,
                                             padding=1, bias=True))
            if i + 1 < n:
                layers += [nn.BatchNorm2d(channels[i + 1]), nn.ReLU(True)]
        super().__init__(*layers)
        self.channels = tuple(int(c) for c in channels)
        self.max_batch = int(max_batch)
        for p in self.parameters():
            p.requires_grad_(False)

    def _ensure(self, batch: int):
        dev = self._inference_device(self[0].weight)
        named = list(self.state_dict(keep_vars=True).items())
        key = (dev, weights_key(t for _, t in named))
        if self._has_handle(key, batch):
            return
        cs = _lib.EammDeconvConfig(num_layers=len(self.channels) - 1, max_batch=max(batch, self.max_batch))
        cs.channels[:len(self.channels)] = self.channels
        self._rebuild_handle(key, cs.max_batch, cs, dev, named)

    def _wants_graph(self) -> bool:
        """Opted in (``requires_grad_(True)``: a parameter requires a gradient) and either in ``.train()`` or with gradients enabled.
        A frozen tail never takes the graph route: a fresh ``nn.Module`` is in training mode and runs the engine."""
        return any(p.requires_grad for p in self.parameters()) and (self.training or torch.is_grad_enabled())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [B,C0,1,1] (the reference's call, util.py:603-607) or [B,C0]; returns [B,C_last,S,S].  A frozen tail runs the
        inference engine; an opted-in one (see the module's docstring) returns a tensor with an autograd graph through HIP
        operators, every BatchNorm over the whole batch B as ``nn.Sequential`` would."""
        if self._wants_graph():
            return self._forward_graph(x)
        refuse_silent_detach(self, x)
        with torch.no_grad():
            return self._forward(x)

    def _forward_graph(self, x: torch.Tensor, steps: int = 1) -> torch.Tensor:
        """util.py:559-576 as a composition of differentiable operators (NHWC between them).  ``steps`` > 1: x is TIME-MAJOR
        [steps * N, C0] and, in ``.train()``, every BatchNorm takes its batch statistics over the N rows of one step and updates
        its running statistics once per step, in step order -- the reference calls ``decon`` once per step (util.py:601-607).
        The transposed convolutions are batched over all rows either way."""
        from . import audio_ops, train_graph
        if x.dim() == 4 and x.shape[2:] == (1, 1):
            x = x.flatten(1)
        if x.dim() != 2 or x.shape[1] != self.channels[0] or x.dtype != torch.float32:
            raise RuntimeError(f"expected float32 [B,{self.channels[0]}(,1,1)], got {tuple(x.shape)} {x.dtype}")
        if self[0].weight.device.type != "cuda" or x.device.type != "cuda":
            raise RuntimeError("eamm_amd.DeconvTail runs only on a ROCm GPU (no CPU fallback): call .cuda()")
        g = train_graph._Graph(self)
        b = x.shape[0]
        if b % steps:
            raise ValueError(f"DeconvTail: {b} rows are not {steps} steps of equal size")
        per_step = g.training and steps > 1
        n = b // steps

        def norm(y, holder):
            if not per_step:
                return g.norm(y, holder, relu=True)
            return torch.cat([g.norm(y[s * n:(s + 1) * n], holder, relu=True) for s in range(steps)], dim=0)

        nl = len(self.channels) - 1
        c1 = self.channels[1]
        # layer 0: k6, s2, p1 on a 1x1 map -> out[Y][X] = in * w[Y+1][X+1] for Y, X in 0..3; the border taps never touch the output
        w0 = self[0].weight[:, :, 1:5, 1:5].permute(0, 2, 3, 1).reshape(self.channels[0], 16 * c1)
        y = (torch.matmul(x, w0).view(b, 4, 4, c1) + self[0].bias)
        y = norm(y, self[1])
        for i in range(1, nl):
            last = i + 1 == nl
            y = audio_ops.conv_transpose4s2_nhwc(y, self[3 * i].weight, self[3 * i].bias, bias_grad_is_zero=g.training and not last)
            if not last:
                y = norm(y, self[3 * i + 1])
        return y.permute(0, 3, 1, 2).contiguous()

    def forward_split(self, x: torch.Tensor) -> "SplitFeatureMap":
        """The same layers, the result in the PRIVATE layout ``KPDetector_a``'s heads read (round 6): ``wide`` NHWC
        [B,S,S,C_last - 3] + ``thin`` [B,S,S,4] (the last three channels and a zero) instead of the reference's NCHW
        [B,C_last,S,S] (util.py:604-607) -- both ends of that tensor live in this library, so the clip harness
        (``driving_keypoints``) skips the NCHW round trip.  Only when C_last = 32 m + 3 (the shipped 35); the values are
        those of ``forward`` bit for bit (``SplitFeatureMap.to_nchw()`` gives the reference's tensor back)."""
        refuse_silent_detach(self, x)
        with torch.no_grad():
            return self._forward(x, split=True)

    def split_channels(self) -> int:
        """``wide`` channel count of ``forward_split`` (0: this tail's output has no 32 m + 3 split)."""
        wide = self.channels[-1] - 3
        return wide if wide >= 32 and wide % 32 == 0 else 0

    def _forward(self, x: torch.Tensor, split: bool = False):
        if x.dim() == 4 and x.shape[2:] == (1, 1):
            x = x.flatten(1)
        if x.dim() != 2 or x.shape[1] != self.channels[0] or x.dtype != torch.float32:
            raise RuntimeError(f"expected float32 [B,{self.channels[0]}(,1,1)], got {tuple(x.shape)} {x.dtype}")
        b = x.shape[0]
        self._ensure(b)
        x = x.contiguous()
        side = 4 << (len(self.channels) - 2)
        if split:
            wide_c = self.split_channels()
            if not wide_c:
                raise RuntimeError(f"forward_split needs 32 m + 3 output channels, this tail has {self.channels[-1]}")
            wide = torch.empty(b, side, side, wide_c, device=x.device)
            thin = torch.empty(b, side, side, 4, device=x.device)
            self._handle.call("forward_split", ptr(x), b, ptr(wide), ptr(thin), stream_ptr(x.device))
            return SplitFeatureMap(wide, thin)
        out = torch.empty(b, self.channels[-1], side, side, device=x.device)
        self._handle.call("forward", ptr(x), b, ptr(out), stream_ptr(x.device))
        return out
