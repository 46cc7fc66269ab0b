"""The operators that make AT_net2 (``AudioFeatureNet``) and its ``decon`` tail (``DeconvTail``) differentiable --
``torch.autograd.Function`` wrappers whose forward AND backward are libeamm_hip.so kernels (csrc/audio.hip, lstm_backward.hip,
audio_backward.hip):

* ``lstm_layer(xproj, w_hh)``  =  one layer of ``nn.LSTM(., 256, batch_first=True)`` from a zero state (reference modules/util.py:551,
  :596-598) on its input projection ``xproj = x W_ih^T + b_ih + b_hh`` [N,T,1024] (gate order i, f, g, o): the inference engine's
  persistent recurrence kernel forward, a persistent backward recurrence of the same partition (16 workgroups, each with its slice
  of W_hh in LDS, exchanging one step's values through tagged words); C ABI ``eamm_op_lstm_forward`` / ``_scan`` / ``_backward``.  The
  forward saves only ``y``: the backward recomputes the gate pre-activations (one product of the shifted ``y`` with W_hh^T, plus
  ``xproj``) and scans ``c_t`` before the recurrence; ``dW_hh`` is one torch matmul of the gate gradients with the shifted ``y``.
* ``conv_transpose4s2_nhwc(x, weight, bias)``  =  ``F.conv_transpose2d(x, weight, bias, stride=2, padding=1)`` with a 4x4 filter in the
  reference's layout [Cin,Cout,4,4] on NHWC (util.py:562-574, ``decon``'s layers 1 .. 4); ``eamm_op_deconv4s2`` / ``_dgrad`` / ``_wgrad``.
* ``maxpool3_nhwc(x, sy, sx)``  =  ``F.max_pool2d(x, 3, (sy, sx))`` on NHWC (util.py:541, :546), the first maximum of a window taking
  the gradient as in ATen; ``eamm_op_audio_maxpool`` / ``_backward``.

``AudioFeatureNet`` and ``DeconvTail`` compose them (with the stride-1 convolutions and BatchNorm of ``autograd_ops`` /
``train_graph``) into the trainable network of the reference's first training stage (train.py ``train_part1``, model.py:187-221).
OP-LEVEL like ``autograd_ops``: every call packs its filter again on the device.  GPU only: no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib, _op
from ._op import CHANNEL_GRANULE, round_up

HIDDEN = 256     # the LSTM kernels' hidden size
MAX_CLIPS = 8    # ... and their largest batch


def lstm_check(device) -> None:
    """Waits for the current stream of ``device`` and raises ``EammError`` if an LSTM operator's recurrence timed out on it (a
    workgroup waited longer than the limit for another; the outputs then hold NaN from the step it stopped at)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    _op.call("lstm_check", device)


class _LstmLayerFunction(torch.autograd.Function):
    """xproj [N,T,1024], w_hh [1024,256] -> y [N,T,256]; only y is kept besides the inputs."""

    @staticmethod
    def forward(ctx, xproj, w_hh):
        n, t, _ = xproj.shape
        dev = xproj.device
        y = torch.empty(n, t, HIDDEN, dtype=torch.float32, device=dev)
        work = _op.workspace("lstm", dev, n, t)     # the call's own W_hh image, state and hand-off words
        w = _op.dense(w_hh.detach())
        _op.call("lstm_forward", dev, xproj, w, n, t, y, work=work)
        ctx.save_for_backward(xproj, w_hh, y)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        xproj, w_hh, y = ctx.saved_tensors
        n, t, _ = xproj.shape
        dev = xproj.device
        w = _op.dense(w_hh.detach())
        grad_y = _op.dense(grad_y)
        h_prev = torch.cat([y.new_zeros(n, 1, HIDDEN), y[:, :-1]], dim=1).reshape(n * t, HIDDEN)          # h_{t-1}, zero state first
        gates = torch.addmm(xproj.detach().reshape(n * t, 4 * HIDDEN), h_prev, w.t()).view(n, t, 4 * HIDDEN).contiguous()
        c = torch.empty(n, t, HIDDEN, dtype=torch.float32, device=dev)
        gx = torch.empty(n, t, 4 * HIDDEN, dtype=torch.float32, device=dev)
        work = _op.workspace("lstm_backward", dev, n, t)
        _op.call("lstm_scan", dev, gates, n, t, c)
        _op.call("lstm_backward", dev, gates, c, w, grad_y, n, t, gx, work=work)
        gw = torch.matmul(gx.reshape(n * t, 4 * HIDDEN).t(), h_prev) if ctx.needs_input_grad[1] else None
        return (gx if ctx.needs_input_grad[0] else None), gw


class _Deconv4s2Function(torch.autograd.Function):
    """NHWC x [B,H,W,Cin], weight [Cin,Cout,4,4], bias [Cout] or None -> NHWC [B,2H,2W,Cout]."""

    @staticmethod
    def forward(ctx, x, weight, bias, bias_grad_is_zero):
        b, h, w, cin = x.shape
        cout = weight.shape[1]
        dev = x.device
        out = torch.empty(b, 2 * h, 2 * w, cout, dtype=torch.float32, device=dev)
        work = _op.workspace("deconv4s2", dev, b, h, w, cin, cout)
        wt = _op.dense(weight.detach())
        bs = _op.dense(bias.detach()) if bias is not None else None
        _op.call("deconv4s2", dev, x, b, h, w, cin, wt, bs, cout, out, work=work)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.bias_grad_is_zero = bool(bias_grad_is_zero)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        b, h, w, cin = x.shape
        cout = weight.shape[1]
        dev = x.device
        grad_out = _op.dense(grad_out)
        gx = gw = gb = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            work = _op.workspace("deconv4s2_dgrad", dev, b, h, w, cin, cout)
            wt = _op.dense(weight.detach())
            _op.call("deconv4s2_dgrad", dev, grad_out, b, h, w, cin, wt, cout, gx, work=work)
        if ctx.needs_input_grad[1] or want_b:
            gw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            if want_b:   # in front of a batch-statistics BatchNorm the bias gradient is exactly zero: no reduction
                gb = torch.zeros(cout, dtype=torch.float32, device=dev) if ctx.bias_grad_is_zero else torch.empty(cout, dtype=torch.float32, device=dev)
            work = _op.workspace("deconv4s2_wgrad", dev, b, h, w, cin, cout)
            _op.call("deconv4s2_wgrad", dev, x, grad_out, b, h, w, cin, cout, gw, gb if (want_b and not ctx.bias_grad_is_zero) else None,
                     work=work)
            if not ctx.needs_input_grad[1]:
                gw = None
        return gx, gw, gb, None


class _MaxPool3Function(torch.autograd.Function):
    """NHWC [B,H,W,C] -> [B,(H-3)/sy+1,(W-3)/sx+1,C]; only x is kept: the backward recomputes each window's winner."""

    @staticmethod
    def forward(ctx, x, sy, sx):
        b, h, w, c = x.shape
        out = torch.empty(b, (h - 3) // sy + 1, (w - 3) // sx + 1, c, dtype=torch.float32, device=x.device)
        _op.call("audio_maxpool", x.device, x, b, h, w, c, sy, sx, out)
        ctx.save_for_backward(x)
        ctx.strides = (sy, sx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        b, h, w, c = x.shape
        sy, sx = ctx.strides
        grad_out = _op.dense(grad_out)
        gx = torch.empty_like(x)
        _op.call("audio_maxpool_backward", x.device, x, grad_out, b, h, w, c, sy, sx, gx)
        return gx, None, None


def lstm_layer(xproj: torch.Tensor, w_hh: torch.Tensor) -> torch.Tensor:
    """One ``nn.LSTM`` layer (hidden 256, ``batch_first``) from a zero initial state: ``xproj`` [N,T,1024] is the input projection
    with both biases added (gate order i, f, g, o), ``w_hh`` [1024,256]; returns ``y`` [N,T,256].  1 <= N <= 8, T >= 1.
    Differentiable in both.  The call does not wait for the device: ``lstm_check`` reports a recurrence that timed out."""
    if not torch.is_tensor(xproj) or xproj.dim() != 3 or xproj.shape[2] != 4 * HIDDEN:
        raise ValueError(f"lstm_layer: xproj must be [N,T,{4 * HIDDEN}] (gates i, f, g, o of {HIDDEN} units), got "
                         f"{tuple(getattr(xproj, 'shape', ()))}")
    n, t, _ = xproj.shape
    if not 1 <= n <= MAX_CLIPS:
        raise ValueError(f"lstm_layer: 1 to {MAX_CLIPS} clips per call, got N = {n}")
    if t < 1:
        raise ValueError("lstm_layer: xproj has no time steps (T = 0)")
    if not torch.is_tensor(w_hh) or tuple(w_hh.shape) != (4 * HIDDEN, HIDDEN):
        raise ValueError(f"lstm_layer: w_hh must be [{4 * HIDDEN},{HIDDEN}], got {tuple(getattr(w_hh, 'shape', ()))}")
    if n * t * 4 * HIDDEN >= 2 ** 31:
        raise ValueError("lstm_layer: fewer than 2^31 gate values")
    _op.operands("audio_ops", "lstm_layer", xproj, w_hh)
    return _LstmLayerFunction.apply(_op.dense(xproj), w_hh)


def conv_transpose4s2_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                           bias_grad_is_zero: bool = False) -> torch.Tensor:
    """``F.conv_transpose2d(x, weight, bias, stride=2, padding=1)`` for 4x4 filters on the kernels' own layout: x NHWC [B,H,W,Cin] ->
    NHWC [B,2H,2W,Cout]; weight [Cin,Cout,4,4] (``nn.ConvTranspose2d``'s layout).  Channels are zero-padded to the kernels' granule
    of 32 here (the padded filter rows / columns are zeros and the slices drop their gradient).  ``bias_grad_is_zero``: the output
    feeds a batch-statistics BatchNorm, so the bias gradient is exactly zero and its reduction is skipped.  Differentiable in x,
    weight and bias."""
    if not torch.is_tensor(x) or not torch.is_tensor(weight) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"conv_transpose4s2_nhwc: NHWC input [B,H,W,Cin] and weight [Cin,Cout,4,4]; got "
                         f"{tuple(getattr(x, 'shape', ()))} / {tuple(getattr(weight, 'shape', ()))}")
    b, h, w, c = x.shape
    cin, cout, kh, kw = weight.shape
    if (kh, kw) != (4, 4):
        raise ValueError(f"conv_transpose4s2_nhwc: 4x4 filters only (stride 2, padding 1), got {kh}x{kw}")
    if c != cin or cin < 1 or cout < 1:
        raise ValueError(f"conv_transpose4s2_nhwc: weight {tuple(weight.shape)} does not fit input {tuple(x.shape)}")
    if b < 1 or h < 1 or w < 1:
        raise ValueError(f"conv_transpose4s2_nhwc: empty input {tuple(x.shape)}")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"conv_transpose4s2_nhwc: bias must be [{cout}], got {tuple(bias.shape)}")
    cin_p, cout_p = round_up(cin, CHANNEL_GRANULE), round_up(cout, CHANNEL_GRANULE)
    if max(b * h * w * cin_p, 4 * b * h * w * cout_p) * 4 >= 2 ** 32 - 16:
        raise ValueError(f"conv_transpose4s2_nhwc: input {tuple(x.shape)} / output beyond the kernels' 32-bit byte offsets")
    _op.operands("audio_ops", "conv_transpose4s2_nhwc", x, weight, bias)
    if cin_p != cin:
        x = F.pad(x, (0, cin_p - cin))
        weight = F.pad(weight, (0, 0, 0, 0, 0, 0, 0, cin_p - cin))
    if cout_p != cout:
        weight = F.pad(weight, (0, 0, 0, 0, 0, cout_p - cout))
        bias = F.pad(bias, (0, cout_p - cout)) if bias is not None else None
    if _lib.lib().eamm_op_deconv4s2_workspace_floats(b, h, w, cin_p, cout_p) == 0:
        raise ValueError(f"conv_transpose4s2_nhwc: unsupported shape {tuple(x.shape)} x {tuple(weight.shape)}")
    y = _Deconv4s2Function.apply(_op.dense(x), weight, bias, bias_grad_is_zero)
    return y[..., :cout] if cout_p != cout else y


def maxpool3_nhwc(x: torch.Tensor, sy: int, sx: int) -> torch.Tensor:
    """``F.max_pool2d(x, 3, stride=(sy, sx))`` (no padding) on NHWC [B,H,W,C] -> [B,(H-3)//sy+1,(W-3)//sx+1,C], differentiable; strides
    1 or 2, C a multiple of 4."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"maxpool3_nhwc: NHWC input [B,H,W,C], got {tuple(getattr(x, 'shape', ()))}")
    b, h, w, c = x.shape
    if sy not in (1, 2) or sx not in (1, 2):
        raise ValueError(f"maxpool3_nhwc: strides 1 or 2, got ({sy}, {sx})")
    if b < 1 or h < 3 or w < 3:
        raise ValueError(f"maxpool3_nhwc: map sides of at least 3 (a 3x3 window without padding), got {h} x {w}")
    if c < 4 or c % 4:
        raise ValueError(f"maxpool3_nhwc: channels a multiple of 4, got C = {c}")
    if x.numel() >= 2 ** 31:
        raise ValueError("maxpool3_nhwc: fewer than 2^31 elements")
    _op.need_gpu(x, "audio_ops", "maxpool3_nhwc")
    return _MaxPool3Function.apply(_op.dense(x), int(sy), int(sx))
