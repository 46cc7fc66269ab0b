"""The pyramid perceptual loss's operators (reference modules/model.py:10-68 and :236-248) -- ``torch.autograd.Function``s whose
forward AND backward are libeamm_hip.so kernels (csrc/perceptual.hip; C ABI ``eamm_op_vgg_input``, ``eamm_op_relu_pool``,
``eamm_op_l1_pair`` and their ``_backward`` entries), and the frozen variant of the convolution operator VGG19's thirteen layers run
on (``eamm_op_conv_dev``, as ``autograd_ops.conv2d_same_nhwc``, but keeping the filter only: no weight gradient is ever asked for).

* ``vgg_input(image, weight, mean, std, inv_scales)``  one call per pyramid level: anti-aliased down-sampling, ``(x - mean) / std``
  and the 32-channel NHWC layout ``conv1_1`` reads; ``pyramid_levels`` is the same node writing the un-normalised NCHW levels.
* ``relu_pool(x, pool)``                               ``F.relu`` in place and, where asked, ``F.max_pool2d(., 2, 2)`` of it.
* ``l1_pair(a, b, weight)``                            ``weight * (a - b.detach()).abs().mean()``, its gradient written in the same pass.
* ``frozen_conv3x3(x, weight, bias)``                  ``F.conv2d(padding=1)`` on NHWC, differentiable in ``x`` alone.
* ``vgg_stem(image, ..., conv_weight, conv_bias, inv_scales)``  ``vgg_input`` and conv1_1 as one node (four-channel data gradient).

GPU only: no CPU fallback."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _op
from ._op import CHANNEL_GRANULE
from .autograd_ops import _Conv2dSameFunction

_MODULE = "perceptual_ops"


def _check_image(image: torch.Tensor, what: str):
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"{what}: an RGB NCHW batch [B,3,H,W] is required, got {tuple(image.shape)}")


def inv_scale_of(scale: float, what: str = "scale") -> int:
    """1 / scale as the integer the kernels take; anything else is refused by name."""
    if not scale > 0:
        raise ValueError(f"{what}: scale {scale} must be positive")
    inv = int(round(1.0 / scale))
    if inv < 1 or abs(inv * scale - 1.0) > 1e-6:
        raise ValueError(f"{what}: 1 / scale must be an integer, got scale {scale}")
    return inv


def _check_levels(image: torch.Tensor, weight, inv_scales: Sequence[int], what: str):
    _check_image(image, what)
    for inv in inv_scales:
        if int(inv) != inv or inv < 1 or image.shape[2] % inv or image.shape[3] % inv:
            raise ValueError(f"{what}: inv_scale {inv} must be an integer >= 1 dividing H and W of {tuple(image.shape)}")
    if any(inv != 1 for inv in inv_scales) and (weight is None or tuple(weight.shape) != (3, 1, 13, 13)):
        raise ValueError(f"{what}: the [3,1,13,13] Gaussian buffer is required")


class _PyramidFunction(torch.autograd.Function):
    """image NCHW [B,3,H,W] -> one tensor per entry of ``invs``: the normalised NHWC [B,h,w,32] input of conv1_1 (``normalised``) or
    the un-normalised NCHW level.  ONE node for all levels, so that the image gradient is the levels' gradients added in the order of
    ``invs`` whatever graph surrounds it."""

    @staticmethod
    def forward(ctx, image, weight, mean, std, invs, normalised):
        b, _, hh, ww = image.shape
        outs = []
        for inv in invs:
            h, w = hh // inv, ww // inv
            if normalised:
                out = torch.empty(b, h, w, CHANNEL_GRANULE, dtype=torch.float32, device=image.device)
                _op.call("vgg_input", image.device, image, weight, mean, std, b, hh, ww, inv, out, None)
            else:
                out = torch.empty(b, 3, h, w, dtype=torch.float32, device=image.device)
                _op.call("vgg_input", image.device, image, weight, None, None, b, hh, ww, inv, None, out)
            outs.append(out)
        ctx.save_for_backward(weight, std)
        ctx.shape, ctx.invs, ctx.normalised = (b, hh, ww), invs, normalised
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        weight, std = ctx.saved_tensors
        b, hh, ww = ctx.shape
        total = None
        for inv, g in zip(ctx.invs, grads):
            if g is None:
                continue
            g = _op.dense(g)
            grad = torch.empty(b, 3, hh, ww, dtype=torch.float32, device=g.device)
            if ctx.normalised:
                _op.call("vgg_input_backward", g.device, g, g.shape[3], None, weight, std, b, hh, ww, inv, grad)
            else:
                _op.call("vgg_input_backward", g.device, None, 0, g, weight, None, b, hh, ww, inv, grad)
            total = grad if total is None else total.add_(grad)
        return (total,) + (None,) * 5


def vgg_input(image: torch.Tensor, weight: Optional[torch.Tensor], mean: torch.Tensor, std: torch.Tensor,
              inv_scales: Sequence[int] = (1,)) -> Tuple[torch.Tensor, ...]:
    """Per entry of ``inv_scales`` the pyramid level of ``image`` (NCHW [B,3,H,W]; AntiAliasInterpolation2d of the reference's
    modules/util.py:1005-1052 with ``weight`` its [3,1,13,13] buffer; 1: the image itself) normalised as modules/model.py:43 does,
    as NHWC [B,H/inv,W/inv,32] with exact zeros in channels 3..31.  ``mean`` / ``std``: three values each.  Differentiable in ``image``."""
    _op.operands(_MODULE, "vgg_input", image, weight, mean, std)
    invs = tuple(int(i) if int(i) == i else i for i in inv_scales)
    _check_levels(image, weight, invs, "vgg_input")
    if mean.numel() != 3 or std.numel() != 3:
        raise ValueError(f"vgg_input: mean / std must hold three values, got {tuple(mean.shape)} / {tuple(std.shape)}")
    return _PyramidFunction.apply(_op.dense(image), None if weight is None else _op.dense(weight.detach()),
                                  _op.dense(mean.detach().reshape(3)), _op.dense(std.detach().reshape(3)), invs, True)


def pyramid_levels(image: torch.Tensor, weight: torch.Tensor, inv_scales: Sequence[int]) -> Tuple[torch.Tensor, ...]:
    """The un-normalised pyramid levels NCHW [B,3,H/inv,W/inv] of ``image`` -- bit for bit what ``vgg_input`` normalises."""
    _op.operands(_MODULE, "pyramid_levels", image, weight)
    invs = tuple(int(i) if int(i) == i else i for i in inv_scales)
    _check_levels(image, weight, invs, "pyramid_levels")
    return _PyramidFunction.apply(_op.dense(image), None if weight is None else _op.dense(weight.detach()), None, None, invs, False)


class _ReluPoolFunction(torch.autograd.Function):
    """x NHWC [B,H,W,C] -> (relu(x) written over x, MaxPool2d(2, 2) of it or None)."""

    @staticmethod
    def forward(ctx, x, pool):
        b, h, w, c = x.shape
        pooled = torch.empty(b, h // 2, w // 2, c, dtype=torch.float32, device=x.device) if pool else None
        y = _op.dense(x)          # x itself, unless it starts off a 16-byte boundary: then the kernel runs on a copy ...
        _op.call("relu_pool", x.device, y, b, h, w, c, pooled)
        if y is not x:
            x.copy_(y)            # ... and x still ends up holding relu(x)
        ctx.mark_dirty(x)
        ctx.save_for_backward(y)
        ctx.set_materialize_grads(False)
        return x, pooled

    @staticmethod
    def backward(ctx, dy, dp):
        if not ctx.needs_input_grad[0] or (dy is None and dp is None):
            return None, None
        (y,) = ctx.saved_tensors
        b, h, w, c = y.shape
        dy = None if dy is None else _op.dense(dy)
        dp = None if dp is None else _op.dense(dp)
        dx = torch.empty_like(y)
        _op.call("relu_pool_backward", y.device, y, dy, dp, b, h, w, c, dx)
        return dx, None


def relu_pool(x: torch.Tensor, pool: bool = True):
    """``y = F.relu(x)`` written IN PLACE over ``x`` (NHWC [B,H,W,C], C a multiple of 32: a convolution's output with its bias added)
    and, with ``pool``, ``p = F.max_pool2d(y, 2, 2)`` on the same layout, [B,H//2,W//2,C].  Returns ``(y, p)``, or ``y`` alone without
    ``pool``.  Both backwards are one kernel: ``dx = (y > 0) * (dy + dp at its window's first maximum)``."""
    _op.need_gpu(x, _MODULE, "relu_pool")
    if x.dim() != 4 or x.shape[3] % CHANNEL_GRANULE or x.shape[3] < CHANNEL_GRANULE or not x.is_contiguous():
        raise ValueError(f"relu_pool: a contiguous NHWC tensor with channels a multiple of {CHANNEL_GRANULE} is required, got "
                         f"{tuple(x.shape)}")
    if pool and (x.shape[1] < 2 or x.shape[2] < 2):
        raise ValueError(f"relu_pool: a {x.shape[1]} x {x.shape[2]} map has no 2 x 2 pooling window")
    if x.is_leaf and x.requires_grad:
        raise ValueError("relu_pool: writes in place, so its input cannot be a leaf that requires a gradient")
    y, p = _ReluPoolFunction.apply(x, bool(pool))
    return (y, p) if pool else y


class _L1PairFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, weight):
        n = a.numel()
        value = torch.empty((), dtype=torch.float32, device=a.device)
        g = torch.empty_like(a)
        work = _op.workspace("l1_pair", a.device, n)
        _op.call("l1_pair", a.device, a, b, n, float(weight), value, g, work=work)
        ctx.save_for_backward(g)
        return value

    @staticmethod
    def backward(ctx, grad_value):
        (g,) = ctx.saved_tensors
        ga = gb = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ga = torch.empty_like(g)
            _op.call("l1_pair_backward", g.device, g, g.numel(), _op.dense(grad_value), ga)
            if ctx.needs_input_grad[1]:
                gb = -ga
            if not ctx.needs_input_grad[0]:
                ga = None
        return ga, gb, None


def l1_pair(a: torch.Tensor, b: torch.Tensor, weight: float = 1.0) -> torch.Tensor:
    """``weight * (a - b).abs().mean()`` as a scalar tensor, summed in a fixed order (the same bits on every run); the gradient
    ``(weight / N) * sign(a - b)`` (``sign(0) = 0``, ``torch.abs``'s own subgradient) is written in the same pass.  ``a`` and ``b``:
    equal shapes; NCHW views of NHWC tensors (what ``Vgg19`` returns) are read where they lie."""
    _op.operands(_MODULE, "l1_pair", a, b)
    if a.shape != b.shape or a.numel() < 1:
        raise ValueError(f"l1_pair: a and b must have one non-empty shape, got {tuple(a.shape)} / {tuple(b.shape)}")
    if a.dim() == 4 and not a.is_contiguous() and a.permute(0, 2, 3, 1).is_contiguous() and b.permute(0, 2, 3, 1).is_contiguous():
        a, b = a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1)
    return _L1PairFunction.apply(_op.dense(a), _op.dense(b), float(weight))


class _FrozenConvFunction(torch.autograd.Function):
    """``autograd_ops._Conv2dSameFunction`` for a frozen filter: only the weight is kept, only the data gradient exists."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(weight)
        return _Conv2dSameFunction._conv(x, weight, bias)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (weight,) = ctx.saved_tensors
        return _Conv2dSameFunction._conv(_op.dense(grad_out), weight, None, transposed=True), None, None


def frozen_conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """``F.conv2d(x, weight, bias, padding=1)`` on NHWC x [B,H,W,Cin] -> [B,H,W,Cout] with a FROZEN 3x3 filter (channels multiples
    of 32): differentiable in ``x`` only -- a parameter that requires a gradient is refused."""
    _op.operands(_MODULE, "frozen_conv3x3", x, weight, bias)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.dim() != 4 or x.shape[3] != weight.shape[1] or \
            weight.shape[1] % CHANNEL_GRANULE or weight.shape[0] % CHANNEL_GRANULE:
        raise ValueError(f"frozen_conv3x3: weight {tuple(weight.shape)} / input {tuple(x.shape)} unsupported "
                         f"(3x3, channels multiples of {CHANNEL_GRANULE})")
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise ValueError("frozen_conv3x3: weight and bias must not require a gradient (the weight gradient of VGG is out of scope)")
    return _FrozenConvFunction.apply(_op.dense(x), weight, bias)


class _VggStemFunction(torch.autograd.Function):
    """image NCHW [B,3,H,W] -> per entry of ``invs`` conv1_1's output NHWC [B,h,w,Cout] (bias added, no ReLU) on that pyramid level.
    One node from the image to conv1_1's output, because the 32-channel padded input exists in the forward only: the data gradient
    is taken with the filter cut to FOUR input channels (a transposed call with Cout = 4, 1/8 of the padded form) and gathered back
    through the Gaussian from there.  The levels' image gradients are added in the order of ``invs``."""

    @staticmethod
    def forward(ctx, image, aa_weight, mean, std, w32, bias, invs):
        b, _, hh, ww = image.shape
        outs = []
        for inv in invs:
            x32 = torch.empty(b, hh // inv, ww // inv, CHANNEL_GRANULE, dtype=torch.float32, device=image.device)
            _op.call("vgg_input", image.device, image, aa_weight, mean, std, b, hh, ww, inv, x32, None)
            outs.append(_Conv2dSameFunction._conv(x32, w32, bias))
        ctx.save_for_backward(aa_weight, std, w32[:, :4].contiguous() if ctx.needs_input_grad[0] else None)
        ctx.shape, ctx.invs = (b, hh, ww), invs
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        aa_weight, std, w4 = ctx.saved_tensors
        b, hh, ww = ctx.shape
        total = None
        for inv, g in zip(ctx.invs, grads):
            if g is None:
                continue
            g4 = _Conv2dSameFunction._conv(_op.dense(g), w4, None, transposed=True)      # [B,h,w,4]: channels 0..2 + a zero
            grad = torch.empty(b, 3, hh, ww, dtype=torch.float32, device=g.device)
            _op.call("vgg_input_backward", g.device, g4, 4, None, aa_weight, std, b, hh, ww, inv, grad)
            total = grad if total is None else total.add_(grad)
        return (total,) + (None,) * 6


def vgg_stem(image: torch.Tensor, weight: Optional[torch.Tensor], mean: torch.Tensor, std: torch.Tensor, conv_weight: torch.Tensor,
             conv_bias: torch.Tensor, inv_scales: Sequence[int] = (1,)) -> Tuple[torch.Tensor, ...]:
    """``frozen_conv3x3(vgg_input(image, ...)[k], conv_weight, conv_bias)`` per entry of ``inv_scales`` as ONE node: ``conv_weight``
    is conv1_1's filter [Cout,3,3,3] padded with zeros to [Cout,32,3,3]; the image gradient goes through its first four input
    channels only.  Same values as the composition, at 1/8 of its data-gradient arithmetic."""
    _op.operands(_MODULE, "vgg_stem", image, weight, mean, std, conv_weight, conv_bias)
    invs = tuple(int(i) if int(i) == i else i for i in inv_scales)
    _check_levels(image, weight, invs, "vgg_stem")
    if mean.numel() != 3 or std.numel() != 3:
        raise ValueError(f"vgg_stem: mean / std must hold three values, got {tuple(mean.shape)} / {tuple(std.shape)}")
    if conv_weight.dim() != 4 or tuple(conv_weight.shape[1:]) != (CHANNEL_GRANULE, 3, 3) or conv_weight.shape[0] % CHANNEL_GRANULE or \
            conv_bias is None or tuple(conv_bias.shape) != (conv_weight.shape[0],):
        raise ValueError(f"vgg_stem: conv_weight must be [Cout,{CHANNEL_GRANULE},3,3] (conv1_1's filter padded) with a [Cout] bias, got "
                         f"{tuple(conv_weight.shape)}")
    if conv_weight.requires_grad or conv_bias.requires_grad:
        raise ValueError("vgg_stem: conv_weight and conv_bias must not require a gradient (the weight gradient of VGG is out of scope)")
    return _VggStemFunction.apply(_op.dense(image), None if weight is None else _op.dense(weight.detach()),
                                  _op.dense(mean.detach().reshape(3)), _op.dense(std.detach().reshape(3)),
                                  _op.dense(conv_weight), _op.dense(conv_bias), invs)
