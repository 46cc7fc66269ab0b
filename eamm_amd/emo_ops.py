"""The operators that make Emotion_k's ResNet-18 trunk differentiable -- ``torch.autograd.Function`` wrappers whose forward AND
backward are libeamm_hip.so kernels (csrc/conv_s2.hip, conv_s2_backward.hip, emotion.hip, emotion_backward.hip):

* ``conv2d_s2_nhwc(x, weight)``  =  ``F.conv2d(x, weight, stride=2, padding=k // 2)`` for the trunk's 3x3 / 1x1 filters on NHWC
  (reference modules/util.py:1069-1099: the first convolution of a down-sampling ``BasicBlock`` and its ``downsample`` shortcut);
  C ABI ``eamm_op_conv_s2`` / ``_dgrad`` / ``_wgrad``;
* ``maxpool3s2_nhwc(x)``  =  ``F.max_pool2d(x, 3, 2, 1)`` on NHWC (util.py:1245), the first maximum of a window taking the gradient
  as in ATen; ``eamm_op_emo_maxpool`` / ``_backward``;
* ``emo_final(a, w98)``  =  the ``final`` Conv1d / MaxPool1d / ReLU stack (util.py:1287-1295) on the [B,64] output of ``fc_all``;
  ``eamm_op_emo_final`` / ``_backward``.

``train_graph._Graph.basic_block`` and ``EmotionDetector.forward`` compose them (with the stride-1 convolutions and BatchNorm of
``autograd_ops`` / ``sync_batchnorm``) into the trainable detector of the reference's second training stage (model.py:312-413).
OP-LEVEL like ``autograd_ops``: every call packs its filter again on the device.  GPU only: no CPU fallback.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import _lib, _op
from ._op import CHANNEL_GRANULE


class _ConvS2Function(torch.autograd.Function):
    """NHWC x [B,Hin,Win,Cin], OIHW weight [Cout,Cin,k,k] -> NHWC [B,Hin/2,Win/2,Cout]."""

    @staticmethod
    def forward(ctx, x, weight):
        b, h, w, cin = x.shape
        cout, _, k, _ = weight.shape
        dev = x.device
        out = torch.empty(b, h // 2, w // 2, cout, dtype=torch.float32, device=dev)
        work = _op.workspace("conv_s2", dev, b, h, w, cin, cout, k)
        wt = _op.dense(weight.detach())
        _op.call("conv_s2", dev, x, b, h, w, cin, wt, cout, k, out, work=work)
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        b, h, w, cin = x.shape
        cout, _, k, _ = weight.shape
        dev = x.device
        grad_out = _op.dense(grad_out)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            work = _op.workspace("conv_s2_dgrad", dev, b, h, w, cin, cout, k)
            wt = _op.dense(weight.detach())
            _op.call("conv_s2_dgrad", dev, grad_out, b, h, w, cin, wt, cout, k, gx, work=work)
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            work = _op.workspace("conv_s2_wgrad", dev, b, h, w, cin, cout, k)
            _op.call("conv_s2_wgrad", dev, x, grad_out, b, h, w, cin, cout, k, gw, work=work)
        return gx, gw


class _MaxPoolFunction(torch.autograd.Function):
    """NHWC [B,H,W,C] -> [B,H/2,W/2,C]; only x is kept: the backward recomputes each window's winner."""

    @staticmethod
    def forward(ctx, x):
        b, h, w, c = x.shape
        out = torch.empty(b, h // 2, w // 2, c, dtype=torch.float32, device=x.device)
        _op.call("emo_maxpool", x.device, x, b, h, w, c, out)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        b, h, w, c = x.shape
        grad_out = _op.dense(grad_out)
        gx = torch.empty_like(x)
        _op.call("emo_maxpool_backward", x.device, x, grad_out, b, h, w, c, gx)
        return gx


class _EmoFinalFunction(torch.autograd.Function):
    """a [B,64], w98 [98] -> value [B,4,2], jacobian [B,4,2,2]."""

    @staticmethod
    def forward(ctx, a, w98):
        b = a.shape[0]
        dev = a.device
        value = torch.empty(b, 4, 2, dtype=torch.float32, device=dev)
        jac = torch.empty(b, 4, 2, 2, dtype=torch.float32, device=dev)
        _op.call("emo_final", dev, a, w98, b, value, jac)
        ctx.save_for_backward(a, w98)
        ctx.set_materialize_grads(False)      # an output the loss never reads has no gradient: its term is skipped
        return value, jac

    @staticmethod
    def backward(ctx, g_value, g_jac):
        a, w98 = ctx.saved_tensors
        if g_value is None and g_jac is None:
            return None, None
        b = a.shape[0]
        dev = a.device
        g_value = None if g_value is None else _op.dense(g_value)
        g_jac = None if g_jac is None else _op.dense(g_jac)
        ga, gw = torch.empty_like(a), torch.empty_like(w98)
        work = _op.workspace("emo_final", dev, b)
        _op.call("emo_final_backward", dev, a, w98, g_value, g_jac, b, ga, gw, work=work)
        return (ga if ctx.needs_input_grad[0] else None), (gw if ctx.needs_input_grad[1] else None)


def conv2d_s2_nhwc(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``F.conv2d(x, weight, stride=2, padding=k // 2)`` on the kernels' own layout: x NHWC [B,Hin,Win,Cin] -> NHWC
    [B,Hin/2,Win/2,Cout]; weight OIHW [Cout,Cin,k,k], k 1 or 3, no bias; Hin and Win even, Cin and Cout multiples of 32.
    Differentiable in x and weight."""
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"conv2d_s2_nhwc: NHWC input [B,H,W,Cin] and OIHW weight [Cout,Cin,k,k]; got {tuple(x.shape)} / {tuple(weight.shape)}")
    b, h, w, c = x.shape
    cout, cin, kh, kw = weight.shape
    if kh != kw or kh not in (1, 3):
        raise ValueError(f"conv2d_s2_nhwc: 1x1 or 3x3 filters only, got {kh}x{kw}")
    if b < 1 or h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"conv2d_s2_nhwc: even map sides only (odd sizes are out of scope), got {h} x {w}")
    if c != cin or cin % CHANNEL_GRANULE or cout % CHANNEL_GRANULE:
        raise ValueError(f"conv2d_s2_nhwc: weight {tuple(weight.shape)} / input {tuple(x.shape)} unsupported (channels multiples of {CHANNEL_GRANULE})")
    _op.operands("emo_ops", "conv2d_s2_nhwc", x, weight)
    if _lib.lib().eamm_op_conv_s2_workspace_floats(b, h, w, cin, cout, kh) == 0:
        raise ValueError(f"conv2d_s2_nhwc: unsupported convolution {tuple(x.shape)} x {tuple(weight.shape)}")
    return _ConvS2Function.apply(_op.dense(x), weight)


def maxpool3s2_nhwc(x: torch.Tensor) -> torch.Tensor:
    """``F.max_pool2d(x, 3, 2, 1)`` on NHWC [B,H,W,C] (H, W even) -> [B,H/2,W/2,C], differentiable."""
    if x.dim() != 4:
        raise ValueError(f"maxpool3s2_nhwc: NHWC input [B,H,W,C], got {tuple(x.shape)}")
    b, h, w, c = x.shape
    if b < 1 or c < 1 or h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"maxpool3s2_nhwc: even map sides only, got {h} x {w}")
    if x.numel() >= 2 ** 31:
        raise ValueError("maxpool3s2_nhwc: fewer than 2^31 elements")
    _op.need_gpu(x, "emo_ops", "maxpool3s2_nhwc")
    return _MaxPoolFunction.apply(_op.dense(x))


def final_weights(final: Sequence[torch.nn.Module]) -> torch.Tensor:
    """The six parameter tensors of ``Emotion_k.final`` (Conv1d at positions 0, 3, 5) flattened in state_dict order: the [98] vector
    ``emo_final`` takes.  A torch concatenation: autograd splits the vector's gradient back onto the modules."""
    return torch.cat([p.reshape(-1) for i in (0, 3, 5) for p in (final[i].weight, final[i].bias)])


def emo_final(a: torch.Tensor, w98: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """util.py:1520-1523 after ``fc_all``: a [B,64] through Conv1d(1,2,4,2,1) - MaxPool1d(2,2) - ReLU - Conv1d(2,4,4,2,1) - ReLU -
    Conv1d(4,4,3) -> (value [B,4,2], jacobian [B,4,2,2]); differentiable in a and in the 98 weights (``final_weights``)."""
    if a.dim() != 2 or a.shape[1] != 64 or a.shape[0] < 1:
        raise ValueError(f"emo_final: input [B,64], got {tuple(a.shape)}")
    if w98.dim() != 1 or w98.numel() != 98:
        raise ValueError(f"emo_final: 98 weights (final_weights), got {tuple(w98.shape)}")
    _op.operands("emo_ops", "emo_final", a, w98)
    return _EmoFinalFunction.apply(_op.dense(a), _op.dense(w98))
