"""The multi-scale discriminator (reference modules/discriminator.py), trainable: every block's 4x4 convolution, InstanceNorm,
LeakyReLU and average pool run on the kernels of ``disc_ops`` (csrc/disc_conv4.hip, csrc/disc_norm.hip), the 1x1 prediction layer on
the library's convolution operator (``eamm_op_conv_dev`` / ``eamm_op_conv_wgrad``) with its filter zero-padded to 32 outputs.
Spectral normalisation (8 MB of filter at most) and the key-point heat maps are small torch compositions in front of the kernels.

The modules keep the reference's constructor arguments, ``forward`` contract and ``state_dict`` layout (``down_blocks.<i>.conv`` /
``.norm``, ``conv``; with ``sn=True`` torch's ``spectral_norm`` keys ``weight_orig``, ``weight_u``, ``weight_v``), loaded strictly.
GPU only: no CPU fallback."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _op
from . import disc_ops as D
from ._op import CHANNEL_GRANULE
from .autograd_ops import _Conv2dSameFunction

_SN_EPS = 1e-12   # torch.nn.utils.spectral_norm's default


class _Conv(nn.Module):
    """``nn.Conv2d``'s parameters (``weight`` / ``bias``), or with ``sn`` those of ``torch.nn.utils.spectral_norm(nn.Conv2d)``:
    ``bias``, ``weight_orig`` and the buffers ``weight_u`` / ``weight_v`` -- in that order, as the hook-based torch module lists
    them.  ``filter()`` is the convolution's weight for this call."""

    def __init__(self, cin: int, cout: int, k: int, sn: bool):
        super().__init__()
        self.in_channels, self.out_channels, self.sn = cin, cout, bool(sn)
        ref = nn.Conv2d(cin, cout, k)   # nn.Conv2d's own initialisation
        if sn:
            self.bias = nn.Parameter(ref.bias.detach().clone())
            self.weight_orig = nn.Parameter(ref.weight.detach().clone())
            self.register_buffer("weight_u", F.normalize(torch.randn(cout), dim=0, eps=_SN_EPS))
            self.register_buffer("weight_v", F.normalize(torch.randn(cin * k * k), dim=0, eps=_SN_EPS))
        else:
            self.weight = nn.Parameter(ref.weight.detach().clone())
            self.bias = nn.Parameter(ref.bias.detach().clone())

    def filter(self) -> torch.Tensor:
        """``weight``; with ``sn``: ``weight_orig / sigma``, ``sigma = u^T W v`` with ``u`` and ``v`` constants, after -- in
        ``.train()`` -- one power iteration that updates ``weight_u`` / ``weight_v`` in place.  The gradient reaches ``weight_orig``
        through ``sigma`` as well: ``(dW - <dW, W> u v^T) / sigma``."""
        if not self.sn:
            return self.weight
        w = self.weight_orig
        mat = w.reshape(w.shape[0], -1)
        if self.training:
            with torch.no_grad():
                self.weight_v.copy_(F.normalize(torch.mv(mat.t(), self.weight_u), dim=0, eps=_SN_EPS))
                self.weight_u.copy_(F.normalize(torch.mv(mat, self.weight_v), dim=0, eps=_SN_EPS))
        u, v = self.weight_u.clone(), self.weight_v.clone()   # the graph keeps this call's vectors; the next call updates the buffers
        sigma = torch.dot(u, torch.mv(mat, v))
        return w / sigma


class DownBlock2d(nn.Module):
    """conv4x4 (valid) -> InstanceNorm2d(affine)? -> LeakyReLU(0.2) -> AvgPool2d(2)? on NHWC tensors."""

    def __init__(self, in_features: int, out_features: int, norm: bool = False, kernel_size: int = 4, pool: bool = False, sn: bool = False):
        super().__init__()
        if kernel_size != 4:
            raise ValueError(f"DownBlock2d: kernel_size must be 4, got {kernel_size}")
        self.conv = _Conv(in_features, out_features, 4, sn)
        self.norm = nn.InstanceNorm2d(out_features, affine=True) if norm else None
        self.pool = bool(pool)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        w = self.conv.filter()
        if x.shape[3] > w.shape[1] > D.THIN_MAX:
            # 17 or more real channels off the 32-channel granule (use_kp with many key points): the ordinary path on a filter
            # zero-padded to the input's channels; autograd cuts the gradient back to the real ones
            w = F.pad(w, (0, 0, 0, 0, 0, x.shape[3] - w.shape[1]))
        y = D.conv4_valid(x, w, self.conv.bias)
        if self.norm is not None:
            return D.norm_act_pool(y, self.norm.weight, self.norm.bias, self.pool)
        return D.norm_act_pool(y, None, None, self.pool)


def kp2gaussian(kp_value: torch.Tensor, spatial_size: Tuple[int, int], kp_variance: float) -> torch.Tensor:
    """[B,K,2] key points in [-1,1] (x, y) -> Gaussian heat maps [B,K,H,W] on the reference's coordinate grid (modules/util.py:815-836)."""
    h, w = spatial_size
    xs = 2 * (torch.arange(w, dtype=kp_value.dtype, device=kp_value.device) / (w - 1)) - 1
    ys = 2 * (torch.arange(h, dtype=kp_value.dtype, device=kp_value.device) / (h - 1)) - 1
    dx = xs.view(1, 1, 1, w) - kp_value[..., 0].reshape(*kp_value.shape[:2], 1, 1)
    dy = ys.view(1, 1, h, 1) - kp_value[..., 1].reshape(*kp_value.shape[:2], 1, 1)
    return torch.exp(-0.5 * (dx ** 2 + dy ** 2) / kp_variance)


class Discriminator(nn.Module):
    """``Discriminator`` of the reference (modules/discriminator.py:36-71).  ``forward(x, kp=None)`` takes NCHW [B,num_channels,H,W]
    and returns ``(feature_maps, prediction_map)``: the blocks' outputs and the [B,1,h,w] prediction as NCHW-shaped views of the
    kernels' NHWC buffers (no copy).  Block widths ``min(max_features, block_expansion * 2**(i+1))`` must be multiples of 32."""

    def __init__(self, num_channels: int = 3, block_expansion: int = 64, num_blocks: int = 4, max_features: int = 512, sn: bool = False,
                 use_kp: bool = False, num_kp: int = 10, kp_variance: float = 0.01, **kwargs):
        super().__init__()
        if num_blocks < 1:
            raise ValueError(f"Discriminator: num_blocks must be at least 1, got {num_blocks}")
        blocks = []
        for i in range(num_blocks):
            cin = num_channels + num_kp * use_kp if i == 0 else min(max_features, block_expansion * (2 ** i))
            cout = min(max_features, block_expansion * (2 ** (i + 1)))
            if cout % CHANNEL_GRANULE:
                raise ValueError(f"Discriminator: down_blocks.{i} has {cout} output channels (block_expansion {block_expansion}, "
                                 f"max_features {max_features}); widths must be multiples of {CHANNEL_GRANULE}")
            blocks.append(DownBlock2d(cin, cout, norm=(i != 0), kernel_size=4, pool=(i != num_blocks - 1), sn=sn))
        self.down_blocks = nn.ModuleList(blocks)
        self.conv = _Conv(blocks[-1].conv.out_channels, 1, 1, sn)
        self.use_kp = bool(use_kp)
        self.kp_variance = kp_variance
        self.in_channels = num_channels + num_kp * use_kp

    def _input_nhwc(self, x: torch.Tensor, kp) -> torch.Tensor:
        """NCHW image (and the heat maps of the detached key points) -> NHWC with ``thin_channels`` floats per pixel, zeros above."""
        if self.use_kp:
            if kp is None:
                raise ValueError("Discriminator: use_kp=True needs kp={'value': [B,num_kp,2]}")
            x = torch.cat([x, kp2gaussian(kp["value"], x.shape[2:], self.kp_variance)], dim=1)
        if x.shape[1] != self.in_channels:
            raise ValueError(f"Discriminator: {self.in_channels} input channels expected, got {tuple(x.shape)}")
        return F.pad(x.permute(0, 2, 3, 1), (0, D.thin_channels(self.in_channels) - self.in_channels))

    def _prediction(self, out: torch.Tensor) -> torch.Tensor:
        """The 1x1 convolution to one channel on the library's convolution operator, its filter zero-padded to 32 outputs."""
        pad = CHANNEL_GRANULE - 1
        w32 = F.pad(self.conv.filter(), (0, 0, 0, 0, 0, 0, 0, pad))
        b32 = F.pad(self.conv.bias, (0, pad))
        return _Conv2dSameFunction.apply(out, w32, b32)[..., :1].permute(0, 3, 1, 2)

    def forward(self, x: torch.Tensor, kp=None):
        _op.need_gpu(x, "discriminator", "Discriminator")
        if x.dim() != 4:
            raise ValueError(f"Discriminator: an NCHW batch is required, got {tuple(x.shape)}")
        out = self._input_nhwc(x, kp)
        feature_maps: List[torch.Tensor] = []
        for i, block in enumerate(self.down_blocks):
            if out.shape[1] < 4 or out.shape[2] < 4:
                raise ValueError(f"Discriminator: the {out.shape[1]} x {out.shape[2]} map in front of down_blocks.{i} is smaller than "
                                 f"its 4 x 4 filter (input {tuple(x.shape)})")
            out = block(out)
            feature_maps.append(out.permute(0, 3, 1, 2))
        return feature_maps, self._prediction(out)


class MultiScaleDiscriminator(nn.Module):
    """``MultiScaleDiscriminator`` of the reference (modules/discriminator.py:74-95): one ``Discriminator`` per scale under
    ``discs.<scale with '.' -> '-'>``.  ``forward(x, kp=None)`` takes the pyramid dict (``prediction_<scale>``: ``ImagePyramide``'s
    output) and returns ``feature_maps_<scale>`` (a list) and ``prediction_map_<scale>`` ([B,1,h,w])."""

    def __init__(self, scales: Sequence[float] = (), **kwargs):
        super().__init__()
        self.scales = scales
        self.discs = nn.ModuleDict({str(scale).replace(".", "-"): Discriminator(**kwargs) for scale in scales})

    def forward(self, x: Dict[str, torch.Tensor], kp=None) -> Dict[str, object]:
        out_dict: Dict[str, object] = {}
        for name, disc in self.discs.items():
            scale = name.replace("-", ".")
            key = "prediction_" + scale
            if key not in x:
                raise KeyError(f"MultiScaleDiscriminator: the pyramid has no level {key!r} (levels: {sorted(x)})")
            feature_maps, prediction_map = disc(x[key], kp)
            out_dict["feature_maps_" + scale] = feature_maps
            out_dict["prediction_map_" + scale] = prediction_map
        return out_dict
