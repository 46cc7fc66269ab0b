"""The key-point heads' reduction as a differentiable operator -- a ``torch.autograd.Function`` whose forward AND backward are
libeamm_hip.so kernels (csrc/kp_head.hip: ``kp_head_launch``, ``kp_head_backward_launch``; C ABI ``eamm_op_kp_head`` /
``eamm_op_kp_head_backward``).

It carries reference modules/keypoint_detector.py:77-105 (``KPDetector``) and :180-205 (``KPDetector_a``) after the two 7x7
convolutions: the temperature softmax over the map, the soft-argmax and the heat-map-weighted sum of the jacobian maps.  The
differentiable detectors (``keypoint_detector``) call it on ONE "same"-padded convolution with the ``kp`` and ``jacobian`` filters
stacked.  GPU only: no CPU fallback.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _op


class _KpHeadFunction(torch.autograd.Function):
    """logits NHWC [B,h,w,Cs] -> value [B,K,2], jacobian [B,K,2,2] (njm > 0), heatmap [B,K,h-6+2pad,w-6+2pad] (want_heatmap)."""

    @staticmethod
    def forward(ctx, logits, k, njm, pad, temperature, want_heatmap):
        b, h, w, cs = logits.shape
        dev = logits.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        value = new(b, k, 2)
        jac = new(b, k, 2, 2) if njm > 0 else None
        heat = new(b, k, h - 6 + 2 * pad, w - 6 + 2 * pad) if want_heatmap else None
        stats = new(b, k, 2)
        ws = _op.workspace("kp_head", dev, b, k)
        _op.call("kp_head", dev, logits, b, k, njm, h, w, cs, pad, float(temperature), value, jac, heat, stats, work=ws)
        ctx.save_for_backward(logits, stats, value, jac)
        ctx.cfg = (k, njm, pad, float(temperature))
        ctx.set_materialize_grads(False)      # an output the loss never reads has no gradient: its term is skipped, not a zero tensor
        return value, jac, heat

    @staticmethod
    def backward(ctx, g_value, g_jac, g_heat):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        logits, stats, value, jac = ctx.saved_tensors
        k, njm, pad, temperature = ctx.cfg
        b, h, w, cs = logits.shape
        dev = logits.device
        cont = lambda t: None if t is None else _op.dense(t)
        g_value, g_jac, g_heat = cont(g_value), cont(g_jac), cont(g_heat)
        grad = torch.empty_like(logits)
        ws = _op.workspace("kp_head", dev, b, k)
        _op.call("kp_head_backward", dev, logits, stats, value, jac, g_value, g_jac, g_heat, b, k, njm, h, w, cs, pad, temperature, grad,
                 work=ws)
        return grad, None, None, None, None, None


def kp_head(logits_nhwc: torch.Tensor, K: int, njm: int, pad: int, temperature: float, want_heatmap: bool = True) -> Dict[str, torch.Tensor]:
    """keypoint_detector.py:86-103 on the NHWC output [B,h,w,Cs] of the "same"-padded 7x7 convolution with the ``kp`` and
    ``jacobian`` filters stacked: channel k is key point k's logit, channel ``K + 4 m + c`` entry c of jacobian map m (``njm`` =
    0, 1 or K maps), further channels are ignored (their gradient is zero).  The reference convolves with padding ``pad``: only the
    window that starts at 3 - pad exists; no cropped copy is made.  Returns the reference's dict: ``value`` [B,K,2], ``heatmap``
    [B,K,h-6+2pad,w-6+2pad] (unless ``want_heatmap`` is False), ``jacobian`` [B,K,2,2] (``njm`` > 0)."""
    K, njm, pad = int(K), int(njm), int(pad)
    if logits_nhwc.dim() != 4 or K < 1 or njm not in (0, 1, K):
        raise ValueError(f"kp_head: NHWC logits [B,h,w,Cs] with K >= 1 key points and 0, 1 or K jacobian maps; got {tuple(logits_nhwc.shape)}, "
                         f"K = {K}, njm = {njm}")
    b, h, w, cs = logits_nhwc.shape
    if cs < K + 4 * njm or cs % 4:
        raise ValueError(f"kp_head: {cs} channels do not hold {K} key-point logits + {njm} jacobian maps (Cs >= K + 4 njm, a multiple of 4)")
    if not 0 <= pad <= 3 or h - 6 + 2 * pad < 1 or w - 6 + 2 * pad < 1:
        raise ValueError(f"kp_head: a {h} x {w} map with padding {pad} (0..3) leaves no window of at least 1 x 1")
    if not temperature > 0:
        raise ValueError(f"kp_head: temperature must be positive, got {temperature}")
    _op.need_gpu(logits_nhwc, "autograd_ops", "kp_head")   # (the module name this message has always carried)
    value, jac, heat = _KpHeadFunction.apply(_op.dense(logits_nhwc), K, njm, pad, float(temperature), bool(want_heatmap))
    out = {"value": value}
    if heat is not None:
        out["heatmap"] = heat
    if jac is not None:
        out["jacobian"] = jac
    return out
