"""The pyramid perceptual loss (reference modules/model.py:10-68 ``Vgg19`` / ``ImagePyramide``, applied as in model.py:236-248) --
the one loss term that reaches the generator's pixels in every shipped configuration.  The thirteen 3x3 convolutions of VGG19 run
on the library's convolution operator (``eamm_op_conv_dev``: the fp32 gather-GEMM, F(4x4,3x3) Winograd above 2048 tiles); the pyramid
with VGG's normalisation, ReLU with max-pool and the L1 reduction are the kernels of csrc/perceptual.hip (``perceptual_ops``).

Weights are the user's to bring (``Vgg19.load_state_dict`` in the reference module's layout, or ``Vgg19.from_torchvision`` on a
torchvision ``vgg19`` checkpoint): nothing here downloads any.  GPU only: no CPU fallback."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _op
from . import perceptual_ops as P
from ._op import CHANNEL_GRANULE
from .weights import antialias_kernel

# torchvision's vgg19().features up to relu5_1 (index 29): the convolutions' indices with (Cin, Cout), the max-pools' indices, and the
# reference's five slices [0,2) [2,7) [7,12) [12,21) [21,30), each ending in the ReLU that is its tap
_CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256), 16: (256, 256),
          19: (256, 512), 21: (512, 512), 23: (512, 512), 25: (512, 512), 28: (512, 512)}
_POOLS = (4, 9, 18, 27)
_SLICES = ((0, 2), (2, 7), (7, 12), (12, 21), (21, 30))
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MIN_SIDE = 16   # four 2x2 max-pools: below this side nn.MaxPool2d fails in the reference


class Vgg19(nn.Module):
    """``Vgg19`` of the reference (modules/model.py:10-50): ``forward(X)`` takes NCHW [B,3,H,W] in [0,1] and returns
    ``[relu1_1, relu2_1, relu3_1, relu4_1, relu5_1]`` as NCHW tensors (views of the kernels' NHWC results), differentiable in ``X``.
    State dict: the reference module's 28 keys (``slice1.0``, ``slice2.{2,5}``, ``slice3.{7,10}``, ``slice4.{12,14,16,19}``,
    ``slice5.{21,23,25,28}`` ``.weight`` / ``.bias``, ``mean``, ``std``); every parameter is frozen."""

    def __init__(self, requires_grad: bool = False):
        super().__init__()
        if requires_grad:
            raise ValueError("Vgg19: requires_grad=True is not supported (the weight gradient of VGG is out of scope: the network "
                             "is a frozen feature extractor)")
        for s, (lo, hi) in enumerate(_SLICES, 1):
            seq = nn.Sequential()
            for i in range(lo, hi):
                if i in _CONVS:
                    seq.add_module(str(i), nn.Conv2d(*_CONVS[i], kernel_size=3, padding=1))
                elif i in _POOLS:
                    seq.add_module(str(i), nn.MaxPool2d(kernel_size=2, stride=2))
                else:
                    seq.add_module(str(i), nn.ReLU(inplace=True))
            setattr(self, f"slice{s}", seq)
        self.mean = nn.Parameter(torch.tensor(_MEAN, dtype=torch.float32).reshape(1, 3, 1, 1), requires_grad=False)
        self.std = nn.Parameter(torch.tensor(_STD, dtype=torch.float32).reshape(1, 3, 1, 1), requires_grad=False)
        for p in self.parameters():
            p.requires_grad = False
        self._first_key = None
        self._first = None

    @classmethod
    def from_torchvision(cls, state_dict: Dict[str, torch.Tensor]) -> "Vgg19":
        """From a torchvision ``vgg19`` checkpoint: ``features.N.weight`` / ``features.N.bias`` (or bare ``N.*``, the state dict of
        ``.features``); ``classifier.*`` and the feature layers at index 30 and above are ignored."""
        own = {}
        for key, value in state_dict.items():
            name = key[len("features."):] if key.startswith("features.") else key
            idx, _, leaf = name.partition(".")
            if key.startswith("classifier.") or not idx.isdigit() or leaf not in ("weight", "bias"):
                if key.startswith("classifier.") or (idx.isdigit() and int(idx) >= 30):
                    continue
                raise KeyError(f"Vgg19.from_torchvision: unexpected key {key!r}")
            if int(idx) >= 30:
                continue
            if int(idx) not in _CONVS:
                raise KeyError(f"Vgg19.from_torchvision: {key!r} is no convolution of vgg19.features")
            s = next(n for n, (lo, hi) in enumerate(_SLICES, 1) if lo <= int(idx) < hi)
            own[f"slice{s}.{idx}.{leaf}"] = value
        net = cls()
        own["mean"], own["std"] = net.mean.data, net.std.data
        net.load_state_dict(own, strict=True)
        return net

    def _conv(self, i: int) -> nn.Conv2d:
        s = next(n for n, (lo, hi) in enumerate(_SLICES, 1) if lo <= i < hi)
        return getattr(getattr(self, f"slice{s}"), str(i))

    def _first_filter(self) -> torch.Tensor:
        """conv1_1's filter padded with zeros to the 32 input channels the convolution kernels read."""
        w = self._conv(0).weight
        key = (w.data_ptr(), w._version, w.device)
        if self._first_key != key:
            self._first = torch.nn.functional.pad(w.detach(), (0, 0, 0, 0, 0, CHANNEL_GRANULE - 3)).contiguous()
            self._first_key = key
        return self._first

    def _frozen(self):
        for name, p in self.named_parameters():
            if p.requires_grad:
                raise ValueError(f"Vgg19: parameter {name} requires a gradient; the network is frozen (the weight gradient of VGG is "
                                 "out of scope)")

    def stems(self, image: torch.Tensor, aa_weight: Optional[torch.Tensor], inv_scales: Sequence[int]):
        """conv1_1's output NHWC (before its ReLU) on the pyramid levels ``inv_scales`` of ``image``: ``perceptual_ops.vgg_stem``."""
        self._frozen()
        return P.vgg_stem(image, aa_weight, self.mean, self.std, self._first_filter(), self._conv(0).bias, inv_scales)

    def features_nhwc(self, stem: torch.Tensor, taps: int = 5) -> List[torch.Tensor]:
        """The first ``taps`` taps as NHWC tensors from conv1_1's output ``stem`` (``stems``; rectified in place here); layers behind
        the last tap asked for are not evaluated."""
        if not 1 <= taps <= 5:
            raise ValueError(f"Vgg19: taps must be 1..5, got {taps}")
        self._frozen()
        out = []
        h = stem
        for i in sorted(_CONVS):
            if i >= _SLICES[taps - 1][1]:
                break
            if i:
                conv = self._conv(i)
                h = P.frozen_conv3x3(h, conv.weight, conv.bias)
            if i + 2 in _POOLS:
                if h.shape[1] < 2 or h.shape[2] < 2:
                    raise ValueError(f"Vgg19: the {h.shape[1]} x {h.shape[2]} map in front of max-pool {i + 2} has no 2 x 2 window "
                                     f"(input sides of at least {MIN_SIDE} are needed for all five taps)")
                h = P.relu_pool(h, True)[1]
            else:
                h = P.relu_pool(h, False)
                if any(i + 2 == hi for _, hi in _SLICES):
                    out.append(h)
        return out

    def forward(self, X: torch.Tensor) -> List[torch.Tensor]:
        _op.need_gpu(X, "perceptual", "Vgg19")
        (stem,) = self.stems(X, None, (1,))
        return [t.permute(0, 3, 1, 2) for t in self.features_nhwc(stem)]


def _scale_name(scale) -> str:
    return str(scale).replace(".", "-")


class _Down(nn.Module):
    """AntiAliasInterpolation2d's state (modules/util.py:1005-1042): the [3,1,13,13] sigma-1.5 buffer, the same at every scale."""

    def __init__(self, scale):
        super().__init__()
        self.register_buffer("weight", antialias_kernel(3))
        self.scale = scale
        self.int_inv_scale = P.inv_scale_of(float(scale), "ImagePyramide")


class ImagePyramide(nn.Module):
    """``ImagePyramide`` of the reference (modules/model.py:53-68): ``forward(x)`` returns ``{'prediction_' + str(scale): level}``
    with NCHW levels; scale 1 returns its input.  Buffers ``downs.<scale with '.' -> '-'>.weight``, one for scale 1 too.
    Differentiable; all levels are ONE autograd node (their gradients are added in the order of ``scales``)."""

    def __init__(self, scales: Sequence[float], num_channels: int = 3):
        super().__init__()
        if num_channels != 3:
            raise ValueError(f"ImagePyramide: num_channels must be 3 (RGB), got {num_channels}")
        self.downs = nn.ModuleDict({_scale_name(s): _Down(s) for s in scales})

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        _op.need_gpu(x, "perceptual", "ImagePyramide")
        downs = [(name, d) for name, d in self.downs.items()]
        for name, d in downs:
            if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % d.int_inv_scale or x.shape[3] % d.int_inv_scale:
                raise ValueError(f"ImagePyramide: scale {d.scale}: 1 / scale must divide H and W of an RGB NCHW batch, got {tuple(x.shape)}")
        small = [(name, d) for name, d in downs if d.int_inv_scale != 1]
        levels = P.pyramid_levels(x, small[0][1].weight, [d.int_inv_scale for _, d in small]) if small else ()
        by_name = {name: level for (name, _), level in zip(small, levels)}
        return {"prediction_" + name.replace("-", "."): by_name.get(name, x) for name, _ in downs}


class PerceptualLoss(nn.Module):
    """The pyramid perceptual loss of modules/model.py:239-248 for one frame pair batch:
    ``sum over scales, sum over i of loss_weights[i] * mean|vgg_i(pyr_s(generated)) - vgg_i(pyr_s(real)).detach()|``.
    The real branch is a pass of its own without a graph; layers behind the last non-zero weight are not evaluated.  (The
    reference's ``/ length`` over frames 0, 4, 8, 12 is the caller's loop.)"""

    def __init__(self, scales: Sequence[float], loss_weights: Sequence[float], vgg: Optional[Vgg19] = None):
        super().__init__()
        weights = [float(w) for w in loss_weights]
        if len(weights) != 5:
            raise ValueError(f"PerceptualLoss: loss_weights must hold five values (relu1_1 .. relu5_1), got {len(weights)}")
        if not any(weights):
            raise ValueError("PerceptualLoss: all loss_weights are zero")
        if not len(scales):
            raise ValueError("PerceptualLoss: scales is empty")
        self.scales = list(scales)
        self.loss_weights = weights
        self.taps = max(i for i, w in enumerate(weights) if w != 0) + 1
        self.pyramid = ImagePyramide(scales, 3)
        self.vgg = vgg if vgg is not None else Vgg19()

    def forward(self, generated: torch.Tensor, real: torch.Tensor) -> torch.Tensor:
        _op.need_gpu(generated, "perceptual", "PerceptualLoss")
        _op.need_gpu(real, "perceptual", "PerceptualLoss")
        if generated.shape != real.shape or generated.dim() != 4 or generated.shape[1] != 3:
            raise ValueError(f"PerceptualLoss: generated {tuple(generated.shape)} and real {tuple(real.shape)} must be one RGB NCHW shape")
        downs = list(self.pyramid.downs.values())
        for d in downs:
            inv = d.int_inv_scale
            if generated.shape[2] % inv or generated.shape[3] % inv:
                raise ValueError(f"PerceptualLoss: scale {d.scale}: 1 / scale must divide H and W of {tuple(generated.shape)}")
            if min(generated.shape[2], generated.shape[3]) // inv < MIN_SIDE:
                raise ValueError(f"PerceptualLoss: scale {d.scale} leaves a {generated.shape[2] // inv} x {generated.shape[3] // inv} "
                                 f"level of {tuple(generated.shape)}; VGG19's four max-pools need sides of at least {MIN_SIDE}")
        invs = [d.int_inv_scale for d in downs]
        weight = downs[0].weight
        # scale 1 is the image itself (a node of its own, as when Vgg19 is applied to ImagePyramide's scale-1 output); the other
        # levels are one node, as ImagePyramide's
        small = [inv for inv in invs if inv != 1]
        gen_small = dict(zip(small, self.vgg.stems(generated, weight, small))) if small else {}
        total = None
        for inv in invs:
            with torch.no_grad():
                fr = self.vgg.features_nhwc(self.vgg.stems(real, weight, (inv,))[0], self.taps)
            fg = self.vgg.features_nhwc(gen_small[inv] if inv != 1 else self.vgg.stems(generated, None, (1,))[0], self.taps)
            for i in range(self.taps):
                if self.loss_weights[i] == 0:
                    continue
                value = P.l1_pair(fg[i], fr[i], self.loss_weights[i])
                total = value if total is None else total + value
        return total
