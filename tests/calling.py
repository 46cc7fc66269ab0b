"""How the differentiable operators are CALLED: what tests/test_calling_host.py and tests/test_gpu_calling_ops.py share.  Plain helper
module like tests/guarded.py: no pytest hooks, no fixtures.

``checked()``: while active, every tensor the binding turns into an address (``eamm_amd._handle.ptr``, the one conversion point of
``_op.call`` and of the BatchNorm calls) is looked at BEFORE the library is called -- on the call's device, contiguous, starting on a
16-byte boundary, float32 unless include/eamm_hip.h documents another type for that operand (``DOCUMENTED``).  A violation raises
``AssertionError`` naming the entry and the operand, and nothing is forwarded: a test that varies or spoils an operand inside
``checked()`` never launches on a bad pointer, whatever the binding does.

``OPERATORS``: one ``Row`` per public differentiable operator -- the smallest inputs on which its kernels still take their general
path, which of them are differentiable, and a float64 reference in plain torch (the expression of the operator's own test module:
test_gpu_backward._warp_reference, test_gpu_motion_ops, test_gpu_kp_backward.head_expression, the loops of test_gpu_audio_backward /
test_gpu_emotion_backward, equivariance_common, perceptual_common, test_gpu_disc_ops._norm_oracle, F.batch_norm).  A reference takes
the operands in one dtype on the CPU and returns the operator's outputs in the operator's own layout, differentiable by autograd:
float64 gives ``want``, float32 the ``want32`` of tests/closeness.py."""
import contextlib
import dataclasses
import sys
import types
from typing import Callable, Optional, Tuple

import torch
import torch.nn.functional as F

import equivariance_common as ec
from closeness import OP_FLOOR
from perceptual_common import _MEAN, _STD, ref_level
from test_gpu_kp_backward import head_expression
from test_gpu_motion_ops import _reference_front

DEV = "cuda:0"
ALIGN = 16

# (entry, C argument index) -> (dtype, alignment in bytes): the operands include/eamm_hip.h documents as something other than float32
DOCUMENTED = {
    ("eamm_disc_norm_act_pool", 10): (torch.float64, 16),             # double* stats
    ("eamm_disc_norm_act_pool_backward", 2): (torch.float64, 16),     # const double* stats
    ("eamm_op_kp_records", 8): (torch.int32, 4),                      # int* singular_flag
    ("eamm_op_resize_aa", 1): (torch.uint8, 1),                       # const uint8_t* in  (frames are HWC uint8)
    ("eamm_op_resize_aa", 10): (torch.uint8, 1),                      # uint8_t* out
    ("eamm_op_similarity_warp", 1): (torch.uint8, 1),                 # const uint8_t* in
    ("eamm_op_to_u8", 5): (torch.uint8, 1),                           # uint8_t* out
}


class Seen:
    """What ``checked()`` saw: ``converted`` = [(entry, operand)] of every tensor that passed on its way to the library."""

    def __init__(self):
        self.converted = []

    @property
    def reached(self):
        return len(self.converted)


@contextlib.contextmanager
def checked(device=DEV):
    import eamm_amd._handle as handle
    original = handle.ptr
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", 0)
    seen = Seen()

    def ptr(t, entry=None, operand=None):
        if t is None:
            return None
        what = f"{entry or 'an entry'}, operand {operand if operand is not None else '?'}"
        dtype, align = DOCUMENTED.get((entry, operand), (torch.float32, ALIGN))
        assert t.device == device, f"{what}: on {t.device}, the call is on {device}"
        assert t.is_contiguous(), f"{what}: not contiguous (shape {tuple(t.shape)}, strides {t.stride()})"
        assert t.data_ptr() % align == 0, f"{what}: starts {t.data_ptr() % align} bytes past a {align}-byte boundary"
        assert t.dtype == dtype, f"{what}: {t.dtype}, the header documents {dtype}"
        seen.converted.append((entry, operand))
        return original(t)

    patched = []
    for name, mod in list(sys.modules.items()):
        if name == "eamm_amd" or name.startswith("eamm_amd."):
            for attr, value in list(vars(mod).items()):
                if value is original:
                    setattr(mod, attr, ptr)
                    patched.append((mod, attr))
    try:
        yield seen
    finally:
        for mod, attr in patched:
            setattr(mod, attr, original)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Row:
    name: str
    op: str                              # the public operator's name: a refusal carries it
    functions: Tuple[str, ...]           # the torch.autograd.Function classes the row's call reaches
    make: Callable[[], dict]             # () -> {operand name: fp32 CPU tensor}, in the operator's argument order
    call: Callable[[dict], tuple]        # {operand name: tensor on the GPU} -> the outputs (None: an absent one)
    ref: Callable[[dict], tuple]         # {operand name: CPU tensor of one dtype} -> the same outputs, by autograd-differentiable torch
    diff: Tuple[str, ...]                # the differentiable operands
    outputs: Tuple[str, ...] = ("out",)
    unstable: Tuple[str, ...] = ()       # operands whose gradient tests/guarded.py lists as unstable (float atomics): held to the bar, not to bits
    inplace: Tuple[str, ...] = ()        # operands the operator writes over: never a leaf, handed over as a copy
    contiguous_only: Optional[str] = None  # the text of the ValueError a non-contiguous operand gets, where the operator documents it
    grad_floor: float = OP_FLOOR         # the floor of the operator's own test for its gradients
    after: Optional[Callable[[], None]] = None   # run once the device has finished (the LSTM's time-out check)
    prepare: Optional[Callable[[], object]] = None   # a module the call needs, built before the operands exist; handed over as "module"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _pad_last(t, to):
    return F.pad(t, (0, to - t.shape[-1]))


# ---- autograd_ops -----------------------------------------------------------------------------------------------------------------------
def _warp_make(n, ns, h, w, c, layout, seed):
    import test_gpu_backward as tb
    feat, defo, om, _ = tb._warp_inputs(n, ns, h, w, c, True, seed)
    if layout == "nhwc":
        return {"features": _nhwc(feat).contiguous(), "deformation": defo.contiguous(), "occlusion": om[:, 0].contiguous()}
    return {"features": feat, "deformation": defo.contiguous(), "occlusion": om}


def _warp_ref(layout):
    def ref(t):      # test_gpu_backward._warp_reference's expression
        f, d, o = t["features"], t["deformation"], t["occlusion"]
        if layout == "nhwc":
            f, o = _nchw(f), o[:, None]
        src = f if f.shape[0] == d.shape[0] else f.expand(d.shape[0], -1, -1, -1)
        y = F.grid_sample(src, d, mode="bilinear", padding_mode="zeros", align_corners=False) * o
        return (_nhwc(y) if layout == "nhwc" else y,)
    return ref


def _conv_make(B, H, W, cin, cout, k, layout, seed):
    g = _gen(seed)
    x = _randn(g, B, cin, H, W)
    wt = _randn(g, cout, cin, k, k, scale=(2.0 / (cin * k * k)) ** 0.5)
    return {"x": _nhwc(x).contiguous() if layout == "nhwc" else x, "weight": wt, "bias": _randn(g, cout, scale=0.1)}


def _conv_ref(layout):
    def ref(t):
        x = _nchw(t["x"]) if layout == "nhwc" else t["x"]
        y = F.conv2d(x, t["weight"], t["bias"], padding=t["weight"].shape[2] // 2)
        return (_nhwc(y) if layout == "nhwc" else y,)
    return ref


def _first7_make():
    g = _gen(31)
    x3 = _randn(g, 1, 9, 13, 3)
    return {"x4": _pad_last(x3, 4), "weight": _randn(g, 32, 3, 7, 7, scale=(2.0 / 147) ** 0.5), "bias": _randn(g, 32, scale=0.1)}


def _first7_ref(t):
    return (_nhwc(F.conv2d(_nchw(t["x4"][..., :3]), t["weight"], t["bias"], padding=3)),)


def _final7_make():
    g = _gen(32)
    return {"x": _randn(g, 1, 9, 13, 32), "weight": _randn(g, 3, 32, 7, 7, scale=(2.0 / (49 * 32)) ** 0.5), "bias": _randn(g, 3, scale=0.1)}


def _final7_ref(t):
    return (torch.sigmoid(F.conv2d(_nchw(t["x"]), t["weight"], t["bias"], padding=3)),)


def _autograd_rows():
    from eamm_amd import autograd_ops as A
    warp = lambda fn: lambda t: (fn(t["features"], t["deformation"], t["occlusion"]),)
    conv = lambda fn: lambda t: (fn(t["x"], t["weight"], t["bias"]),)
    return [
        Row("warp", "warp", ("_WarpFunction",), lambda: _warp_make(2, 2, 12, 20, 32, "nchw", 1), warp(A.warp), _warp_ref("nchw"),
            ("features", "deformation", "occlusion"), unstable=("features",)),
        Row("warp_nhwc", "warp_nhwc", ("_WarpFunction",), lambda: _warp_make(2, 1, 12, 20, 32, "nhwc", 2), warp(A.warp_nhwc), _warp_ref("nhwc"),
            ("features", "deformation", "occlusion"), unstable=("features",)),
        Row("conv2d_same", "conv2d_same", ("_Conv2dSameFunction",), lambda: _conv_make(1, 8, 12, 32, 32, 3, "nchw", 3), conv(A.conv2d_same),
            _conv_ref("nchw"), ("x", "weight", "bias")),
        Row("conv2d_same_nhwc", "conv2d_same_nhwc", ("_Conv2dSameFunction",), lambda: _conv_make(1, 8, 12, 32, 32, 7, "nhwc", 4),
            conv(A.conv2d_same_nhwc), _conv_ref("nhwc"), ("x", "weight", "bias")),
        # the backward that starts from the forward's saved workspace (conv_wgrad_saved): the smallest shape for which
        # eamm_op_conv_saved_transform_offset names an offset -- 2048 4x4 tiles, Cin a multiple of 64 (tests/test_calling_host.py)
        Row("conv2d_same_nhwc_saved", "conv2d_same_nhwc", ("_Conv2dSameFunction",), lambda: _conv_make(*SAVED_SHAPE, 3, "nhwc", 5),
            conv(A.conv2d_same_nhwc), _conv_ref("nhwc"), ("x", "weight", "bias")),
        Row("first_conv7", "first_conv7", ("_FirstConv7Function",), _first7_make, lambda t: (A.first_conv7(t["x4"], t["weight"], t["bias"]),),
            _first7_ref, ("x4", "weight", "bias")),
        Row("final_conv7_sigmoid", "final_conv7_sigmoid", ("_FinalConvSigmoidFunction",), _final7_make,
            lambda t: (A.final_conv7_sigmoid(t["x"], t["weight"], t["bias"]),), _final7_ref, ("x", "weight", "bias")),
    ]


SAVED_SHAPE = (2, 128, 128, 64, 32)      # B, H, W, Cin, Cout


# ---- motion_ops -------------------------------------------------------------------------------------------------------------------------
def _aa_make():
    from eamm_amd.weights import antialias_kernel
    return {"source": torch.rand(2, 3, 16, 24, generator=_gen(41)), "weight": antialias_kernel(3)}


def _aa_ref(t):     # modules/util.py:1044-1052, as test_gpu_motion_ops.test_antialias_down_forward_and_backward
    y = F.conv2d(F.pad(t["source"], (6, 6, 6, 6)), t["weight"], groups=3)[:, :, ::4, ::4]
    return (_pad_last(_nhwc(y), 4),)


def _kp_make(n, K, jac):
    from eamm_amd.weights import synthetic_keypoints
    kd, ks = synthetic_keypoints(n, K, seed=2, jacobian=jac), synthetic_keypoints(n, K, seed=0, jacobian=jac)
    out = {"kd_value": kd["value"], "ks_value": ks["value"]}
    if jac:
        out = {"kd_value": kd["value"], "kd_jacobian": kd["jacobian"], "ks_value": ks["value"], "ks_jacobian": ks["jacobian"]}
    return out


def _kp_dicts(t):
    kd, ks = {"value": t["kd_value"]}, {"value": t["ks_value"]}
    if "kd_jacobian" in t:
        kd["jacobian"], ks["jacobian"] = t["kd_jacobian"], t["ks_jacobian"]
    return kd, ks


def _records_ref(t):     # dense_motion.py:47-67: kd.xy, ks.xy, J = Js inverse(Jd) (the identity without jacobians)
    kd, ks = _kp_dicts(t)
    n, K = kd["value"].shape[:2]
    if "jacobian" in kd:
        J = torch.matmul(ks["jacobian"], torch.inverse(kd["jacobian"])).reshape(n, K, 4)
    else:
        J = torch.eye(2, dtype=kd["value"].dtype).reshape(1, 1, 4).expand(n, K, 4)
    return (torch.cat([kd["value"], ks["value"], J], dim=2),)


def _records(n, K, seed_d=4, seed_s=6):
    from eamm_amd.weights import synthetic_keypoints
    kd, ks = synthetic_keypoints(n, K, seed=seed_d), synthetic_keypoints(n, K, seed=seed_s)
    return _records_ref({"kd_value": kd["value"], "kd_jacobian": kd["jacobian"], "ks_value": ks["value"], "ks_jacobian": ks["jacobian"]})[0].contiguous()


def _from_records(rec):
    """The key-point dicts test_gpu_motion_ops._reference_front takes, from records: J inverse(identity) = J."""
    n, K = rec.shape[:2]
    eye = torch.eye(2, dtype=rec.dtype).expand(n, K, 2, 2)
    return {"value": rec[..., 0:2], "jacobian": eye}, {"value": rec[..., 2:4], "jacobian": rec[..., 4:8].reshape(n, K, 2, 2)}


FRONT = dict(n=2, K=3, h=16, w=16, variance=0.01, cpad=32)


def _front_make():
    small = torch.rand(FRONT["n"], FRONT["h"], FRONT["w"], 3, generator=_gen(5))
    return {"records": _records(FRONT["n"], FRONT["K"]), "small": _pad_last(small, 4)}


def _front_ref(t):
    kd, ks = _from_records(t["records"])
    hg, warped, _ = _reference_front(kd, ks, _nchw(t["small"][..., :3]), FRONT["variance"], True)
    n, k1 = hg.shape[:2]
    hg = hg.permute(0, 3, 4, 1, 2).reshape(n, FRONT["h"], FRONT["w"], 4 * k1)     # channel 4k = heat-map k, 4k+1..3 = RGB warped by motion k
    return _pad_last(hg, FRONT["cpad"]), warped


def _head_make(occ, stacked):
    g = _gen(9)
    n, K, h, w = 2, 3, 16, 16
    out = {"mask_logits": _randn(g, n, h, w, 32)}
    if occ and not stacked:
        out["occlusion_logits"] = _randn(g, n, h, w, 32)
    out["records"] = _records(n, K)
    return out


def _head_ref(occ, stacked):
    def ref(t):     # dense_motion.py:98-111, as test_gpu_motion_ops.test_motion_head_against_torch_double
        lm, rec = t["mask_logits"], t["records"]
        n, h, w, _ = lm.shape
        K = rec.shape[1]
        kd, ks = _from_records(rec)
        _, _, motions = _reference_front(kd, ks, torch.zeros(n, 3, h, w, dtype=lm.dtype), 0.01, True)
        mask = F.softmax(_nchw(lm[..., :K + 1]), dim=1)
        defo = (motions.permute(0, 1, 4, 2, 3) * mask[:, :, None]).sum(dim=1).permute(0, 2, 3, 1)
        o = None
        if occ:
            o = torch.sigmoid(lm[..., K + 1] if stacked else t["occlusion_logits"][..., 0])
        return mask, defo, o
    return ref


def _motion_rows():
    from eamm_amd import motion_ops as M
    head = lambda stacked: lambda t: tuple(M.motion_head(t["mask_logits"], t.get("occlusion_logits"), t["records"], stacked=stacked))
    return [
        Row("antialias_down", "antialias_down", ("_AntiAliasDownFunction",), _aa_make, lambda t: (M.antialias_down(t["source"], t["weight"], 0.25),),
            _aa_ref, ("source",)),
        Row("kp_records_jacobians", "kp_records", ("_KpRecordsFunction",), lambda: _kp_make(2, 3, True), lambda t: (M.kp_records(*_kp_dicts(t)),),
            _records_ref, ("kd_value", "kd_jacobian", "ks_value", "ks_jacobian")),
        Row("kp_records_values", "kp_records", ("_KpRecordsFunction",), lambda: _kp_make(2, 3, False), lambda t: (M.kp_records(*_kp_dicts(t)),),
            _records_ref, ("kd_value", "ks_value")),
        Row("motion_front", "motion_front", ("_MotionFrontFunction",), _front_make,
            lambda t: tuple(M.motion_front(t["records"], t["small"], FRONT["variance"], FRONT["cpad"])), _front_ref, ("records", "small"),
            outputs=("hourglass_input", "sparse_deformed"), unstable=("small",)),
        Row("motion_head", "motion_head", ("_MotionHeadFunction",), lambda: _head_make(True, False), head(False), _head_ref(True, False),
            ("mask_logits", "occlusion_logits", "records"), outputs=("mask", "deformation", "occlusion")),
        Row("motion_head_stacked", "motion_head", ("_MotionHeadFunction",), lambda: _head_make(True, True), head(True), _head_ref(True, True),
            ("mask_logits", "records"), outputs=("mask", "deformation", "occlusion")),
        Row("motion_head_no_occlusion", "motion_head", ("_MotionHeadFunction",), lambda: _head_make(False, False), head(False),
            _head_ref(False, False), ("mask_logits", "records"), outputs=("mask", "deformation", "occlusion")),
    ]


# ---- kp_ops -----------------------------------------------------------------------------------------------------------------------------
KP_T = 0.1


def _kp_head_row(njm):
    from eamm_amd import kp_ops
    import test_gpu_kp_backward as kpb
    K, h, w, pad, B = 3, 9, 14, 0, 2

    def call(t):
        out = kp_ops.kp_head(t["logits"], K, njm, pad, KP_T)
        return out["value"], out.get("jacobian"), out["heatmap"]

    def ref(t):
        out = head_expression(t["logits"], K, njm, pad, KP_T)
        return out["value"], out.get("jacobian"), out["heatmap"]

    return Row(f"kp_head_njm{njm}", "kp_head", ("_KpHeadFunction",), lambda: {"logits": kpb.head_logits(h, w, K, njm, B)}, call, ref, ("logits",),
               outputs=("value", "jacobian", "heatmap"))


# ---- emo_ops ----------------------------------------------------------------------------------------------------------------------------
def _emo_final_ref(t):     # util.py:1287-1295, as test_gpu_emotion_backward.test_emo_final_forward_and_gradients
    al, wl = t["a"], t["w98"]
    B = al.shape[0]
    c1w, c1b, c2w, c2b, c3w, c3b = wl[0:8].view(2, 1, 4), wl[8:10], wl[10:42].view(4, 2, 4), wl[42:46], wl[46:94].view(4, 4, 3), wl[94:98]
    y = torch.relu(F.max_pool1d(F.conv1d(al[:, None], c1w, c1b, 2, 1), 2, 2))
    r = F.conv1d(torch.relu(F.conv1d(y, c2w, c2b, 2, 1)), c3w, c3b)
    return r[:, :, :2], r[:, :, 2:].reshape(B, 4, 2, 2)


def _emo_rows():
    from eamm_amd import emo_ops as E

    def s2_make():
        g = _gen(103)
        return {"x": _randn(g, 2, 6, 10, 32), "weight": _randn(g, 32, 32, 3, 3, scale=1.0 / (32 * 9) ** 0.5)}

    def final_make():
        g = _gen(23)
        return {"a": _randn(g, 2, 64).abs(), "w98": _randn(g, 98, scale=0.5)}

    return [
        Row("conv2d_s2_nhwc", "conv2d_s2_nhwc", ("_ConvS2Function",), s2_make, lambda t: (E.conv2d_s2_nhwc(t["x"], t["weight"]),),
            lambda t: (_nhwc(F.conv2d(_nchw(t["x"]), t["weight"], stride=2, padding=1)),), ("x", "weight")),
        Row("maxpool3s2_nhwc", "maxpool3s2_nhwc", ("_MaxPoolFunction",), lambda: {"x": _randn(_gen(7), 2, 6, 10, 64)},
            lambda t: (E.maxpool3s2_nhwc(t["x"]),), lambda t: (_nhwc(F.max_pool2d(_nchw(t["x"]), 3, 2, 1)),), ("x",)),
        Row("emo_final", "emo_final", ("_EmoFinalFunction",), final_make, lambda t: tuple(E.emo_final(t["a"], t["w98"])), _emo_final_ref,
            ("a", "w98"), outputs=("value", "jacobian")),
    ]


# ---- audio_ops --------------------------------------------------------------------------------------------------------------------------
def _lstm_make():
    import test_gpu_audio_backward as tab
    xproj, whh, _, _ = tab.lstm_reference((2, 3))
    return {"xproj": xproj.clone(), "w_hh": whh.clone()}


def _lstm_ref(t):     # the recurrence as nn.LSTM computes it, written out: test_gpu_audio_backward.lstm_reference
    xp, w = t["xproj"], t["w_hh"]
    n, steps, _ = xp.shape
    h = torch.zeros(n, 256, dtype=xp.dtype)
    c = torch.zeros(n, 256, dtype=xp.dtype)
    ys = []
    for s in range(steps):
        i, f, gg, o = (xp[:, s] + h @ w.t()).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        ys.append(h)
    return (torch.stack(ys, dim=1),)


def _audio_rows():
    from eamm_amd import audio_ops as U

    def deconv_make():     # 24 -> 35 channels: both are padded to the kernels' granule
        g = _gen(73)
        return {"x": _randn(g, 2, 3, 4, 24), "weight": _randn(g, 24, 35, 4, 4, scale=1.0 / (24 * 4) ** 0.5), "bias": _randn(g, 35, scale=0.1)}

    def pool_make():
        x = torch.randperm(2 * 7 * 6 * 8, generator=_gen(29)).float().reshape(2, 7, 6, 8) / 64.0     # no two values equal: no ties
        return {"x": x}

    return [
        Row("lstm_layer", "lstm_layer", ("_LstmLayerFunction",), _lstm_make, lambda t: (U.lstm_layer(t["xproj"], t["w_hh"]),), _lstm_ref,
            ("xproj", "w_hh"), after=lambda: U.lstm_check(DEV)),
        Row("conv_transpose4s2_nhwc", "conv_transpose4s2_nhwc", ("_Deconv4s2Function",), deconv_make,
            lambda t: (U.conv_transpose4s2_nhwc(t["x"], t["weight"], t["bias"]),),
            lambda t: (_nhwc(F.conv_transpose2d(_nchw(t["x"]), t["weight"], t["bias"], stride=2, padding=1)),), ("x", "weight", "bias")),
        Row("maxpool3_nhwc", "maxpool3_nhwc", ("_MaxPool3Function",), pool_make, lambda t: (U.maxpool3_nhwc(t["x"], 1, 2),),
            lambda t: (_nhwc(F.max_pool2d(_nchw(t["x"]), 3, stride=(1, 2))),), ("x",)),
    ]


# ---- perceptual_ops ---------------------------------------------------------------------------------------------------------------------
INVS = (1, 2)


def _image_make(seed, extra=None):
    from eamm_amd.weights import antialias_kernel
    out = {"image": torch.rand(2, 3, 16, 24, generator=_gen(seed)), "weight": antialias_kernel(3)}
    if extra != "levels":
        out.update(mean=torch.tensor(_MEAN), std=torch.tensor(_STD))
    if extra == "stem":
        g = _gen(seed + 1)
        out.update(conv_weight=F.pad(_randn(g, 32, 3, 3, 3, scale=(2.0 / 27) ** 0.5), (0, 0, 0, 0, 0, 29)), conv_bias=_randn(g, 32, scale=0.05))
    return out


def _normalised(t, inv):
    return (ref_level(t["image"], inv) - t["mean"].reshape(1, 3, 1, 1)) / t["std"].reshape(1, 3, 1, 1)


def _perceptual_rows():
    from eamm_amd import perceptual_ops as P

    def relu_make():
        return {"x": _randn(_gen(6), 2, 6, 10, 32)}

    def relu_ref(t):
        y = F.relu(t["x"])
        return y, _nhwc(F.max_pool2d(_nchw(y), 2, 2))

    def l1_make():
        g = _gen(12)
        a, b = _randn(g, 3, 5, 7, 11), _randn(g, 3, 5, 7, 11)
        a.reshape(-1)[::7] = b.reshape(-1)[::7]                       # planted a == b: sign(0) = 0
        return {"a": a, "b": b}

    def frozen_make():
        g = _gen(14)
        return {"x": _randn(g, 1, 8, 12, 32), "weight": _randn(g, 32, 32, 3, 3, scale=(2.0 / (9 * 32)) ** 0.5), "bias": _randn(g, 32, scale=0.05)}

    return [
        Row("vgg_input", "vgg_input", ("_PyramidFunction",), lambda: _image_make(3),
            lambda t: tuple(P.vgg_input(t["image"], t["weight"], t["mean"], t["std"], INVS)),
            lambda t: tuple(_pad_last(_nhwc(_normalised(t, inv)), 32) for inv in INVS), ("image",), outputs=("level_1", "level_2")),
        Row("pyramid_levels", "pyramid_levels", ("_PyramidFunction",), lambda: _image_make(5, "levels"),
            lambda t: tuple(P.pyramid_levels(t["image"], t["weight"], INVS)), lambda t: tuple(ref_level(t["image"], inv) for inv in INVS), ("image",),
            outputs=("level_1", "level_2")),
        Row("relu_pool", "relu_pool", ("_ReluPoolFunction",), relu_make, lambda t: tuple(P.relu_pool(t["x"], True)), relu_ref, ("x",),
            outputs=("y", "pooled"), inplace=("x",), contiguous_only="relu_pool: a contiguous NHWC tensor"),
        Row("l1_pair", "l1_pair", ("_L1PairFunction",), l1_make, lambda t: (P.l1_pair(t["a"], t["b"], 10.0),),
            lambda t: (10.0 * (t["a"] - t["b"]).abs().mean(),), ("a", "b")),
        Row("frozen_conv3x3", "frozen_conv3x3", ("_FrozenConvFunction",), frozen_make, lambda t: (P.frozen_conv3x3(t["x"], t["weight"], t["bias"]),),
            _conv_ref("nhwc"), ("x",)),
        Row("vgg_stem", "vgg_stem", ("_VggStemFunction",), lambda: _image_make(18, "stem"),
            lambda t: tuple(P.vgg_stem(t["image"], t["weight"], t["mean"], t["std"], t["conv_weight"], t["conv_bias"], INVS)),
            lambda t: tuple(_nhwc(F.conv2d(_normalised(t, inv), t["conv_weight"][:, :3], t["conv_bias"], padding=1)) for inv in INVS), ("image",),
            outputs=("level_1", "level_2")),
    ]


# ---- disc_ops ---------------------------------------------------------------------------------------------------------------------------
def _disc_rows():
    from eamm_amd import disc_ops as D
    import test_gpu_disc_ops as tdo

    def conv_make(shape, cout, real, seed):
        x, wt, bias = tdo._conv_inputs(shape, cout, real, seed)
        return {"x": x, "weight": wt, "bias": bias}

    def conv_ref(t):
        real = t["weight"].shape[1]
        return (_nhwc(F.conv2d(_nchw(t["x"][..., :real]), t["weight"], t["bias"])),)

    def norm_make(shape, norm, seed=4):
        g = _gen(seed)
        out = {"x": _randn(g, *shape, scale=1.5) + 0.3}
        if norm:
            out.update(gamma=0.5 + torch.rand(shape[3], generator=g), beta=_randn(g, shape[3], scale=0.2))
        return out

    def norm_ref(pool):
        def ref(t):     # test_gpu_disc_ops._norm_oracle's expression
            y = _nchw(t["x"])
            if "gamma" in t:
                y = F.instance_norm(y, weight=t["gamma"], bias=t["beta"], eps=1e-5)
            y = F.leaky_relu(y, 0.2)
            return (_nhwc(F.avg_pool2d(y, 2) if pool else y),)
        return ref

    conv = lambda t: (D.conv4_valid(t["x"], t["weight"], t["bias"]),)
    norm = lambda pool: lambda t: (D.norm_act_pool(t["x"], t.get("gamma"), t.get("beta"), pool),)
    return [
        Row("conv4_valid_thin", "conv4_valid", ("_Conv4Function",), lambda: conv_make((2, 9, 12, 4), 64, 3, 1), conv, conv_ref, ("x", "weight", "bias")),
        Row("conv4_valid_wide", "conv4_valid", ("_Conv4Function",), lambda: conv_make((1, 8, 16, 32), 32, 32, 1), conv, conv_ref, ("x", "weight", "bias")),
        Row("norm_act_pool", "norm_act_pool", ("_NormActPoolFunction",), lambda: norm_make((2, 5, 7, 64), True), norm(True), norm_ref(True),
            ("x", "gamma", "beta")),
        Row("norm_act_pool_plain", "norm_act_pool", ("_NormActPoolFunction",), lambda: norm_make((1, 5, 5, 64), False), norm(False), norm_ref(False),
            ("x",)),
    ]


# ---- equivariance_ops -------------------------------------------------------------------------------------------------------------------
POINTS = 5


def _equi_rows():
    from eamm_amd import equivariance_ops as Q

    def frame_make():
        theta, params = ec.draw_params(2, POINTS, ec.WIDE, seed=1)
        return {"frame": torch.rand(2, 3, 16, 24, generator=_gen(1)), "theta": theta, "control_params": params}

    def points_make():
        theta, params = ec.draw_params(3, POINTS, ec.WIDE, seed=2)
        return {"coords": ec.planted_coords(POINTS, 37)[None].contiguous(), "theta": theta, "control_params": params}     # one set for every image

    def points_ref(want_jac):
        def ref(t):     # equivariance_common.warp_with_jacobian on the row's own leaf
            each = t["coords"].expand(t["theta"].shape[0], -1, -1)
            out = ec.warp(each, t["theta"], t["control_params"], POINTS)
            if not want_jac:
                return out, None
            gx, = torch.autograd.grad(out[..., 0].sum(), each, create_graph=True)
            gy, = torch.autograd.grad(out[..., 1].sum(), each, create_graph=True)
            return out, torch.stack([gx, gy], dim=-2)
        return ref

    pts = lambda want_jac: lambda t: tuple(Q.tps_warp_points(t["coords"], t["theta"], t["control_params"], POINTS, want_jac))
    return [
        Row("tps_warp_frame", "tps_warp_frame", (), frame_make, lambda t: (Q.tps_warp_frame(t["frame"], t["theta"], t["control_params"], POINTS),),
            lambda t: (ec.transform_frame(t["frame"], t["theta"], t["control_params"], POINTS),), ()),
        Row("tps_warp_points_jacobian", "tps_warp_points", ("_TpsWarpPointsFunction",), points_make, pts(True), points_ref(True), ("coords",),
            outputs=("out", "jacobian")),
        Row("tps_warp_points", "tps_warp_points", ("_TpsWarpPointsFunction",), points_make, pts(False), points_ref(False), ("coords",),
            outputs=("out", "jacobian")),
    ]


# ---- sync_batchnorm ---------------------------------------------------------------------------------------------------------------------
def _bn_rows():
    def nchw_make():
        g = _gen(51)
        return {"x": _randn(g, 3, 5, 7, 9, scale=2.0) + 0.5, "weight": torch.rand(5, generator=g) + 0.5, "bias": _randn(g, 5, scale=0.3)}

    def nhwc_make():
        g = _gen(5)
        return {"x": _randn(g, 3, 6, 10, 12, scale=2.0) + 0.5, "weight": torch.rand(12, generator=g) + 0.5, "bias": _randn(g, 12, scale=0.3)}

    def lend(mod, t):     # the row's tensors as the module's parameters (as train_graph lends a holder's to its adapter)
        mod._parameters["weight"], mod._parameters["bias"] = t["weight"], t["bias"]
        return mod

    def nchw_call(t):
        return (lend(t["module"], t)(t["x"]),)

    def nhwc_call(t):     # the fused NHWC Function through its public caller, train_graph's norm_relu (BatchNorm + ReLU + 2x2 average pool)
        from eamm_amd.train_graph import _Graph
        graph = _Graph(types.SimpleNamespace(training=True, process_group=None, sync_batchnorm=None))
        return (graph.norm_relu(t["x"], lend(t["module"], t), pool=True),)

    def sbn():
        from eamm_amd import SynchronizedBatchNorm2d
        return SynchronizedBatchNorm2d(5).to(DEV).train()

    def ref(t, nhwc):
        x = _nchw(t["x"]) if nhwc else t["x"]
        y = F.batch_norm(x, None, None, t["weight"], t["bias"], True, 0.1, 1e-5)
        return (_nhwc(F.avg_pool2d(F.relu(y), 2)) if nhwc else y,)

    return [
        Row("sync_batchnorm_train", "SynchronizedBatchNorm2d", ("_BatchNormFunction",), nchw_make, nchw_call, lambda t: ref(t, False),
            ("x", "weight", "bias"), prepare=sbn),
        Row("batchnorm_nhwc_fused", "SynchronizedBatchNorm2d", ("_BatchNormNHWCFunction",), nhwc_make, nhwc_call, lambda t: ref(t, True),
            ("x", "weight", "bias"), prepare=lambda: torch.nn.BatchNorm2d(12).to(DEV).train()),
    ]


def _rows():
    rows = (_autograd_rows() + _motion_rows() + [_kp_head_row(njm) for njm in (0, 1, 3)] + _emo_rows() + _audio_rows() + _perceptual_rows()
            + _disc_rows() + _equi_rows() + _bn_rows())
    assert len({r.name for r in rows}) == len(rows)
    return {r.name: r for r in rows}


OPERATORS = _rows()

# torch.autograd.Function classes of eamm_amd that no row reaches, with the reason (at most 2)
EXEMPT_FUNCTIONS = {}
