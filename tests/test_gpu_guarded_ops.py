"""Every operator entry between poisoned guard bands (tests/guarded.py), at the alignment include/eamm_hip.h documents.

Each case runs three times: on plain torch tensors, in an arena whose views start on a 256-byte boundary, and in one whose views
start 16 bytes past it.  A case is a function of ``place`` that runs the existing comparison with the existing reference at the
existing bar (most are the other test files' own helpers, called with their ``place=`` argument).  After the two guarded runs
``Arena.check()`` must pass -- no guard word changed, no input written to, no NaN in an output -- and every output must be
bit-equal to the plain run's: the library documents fixed-order sums and no float atomics outside the listed exceptions.

The registry and the driver ``run_three`` live in tests/guarded.py.  This file registers the eamm_op_* and eamm_bn_* cases; the modules
imported at its end register theirs, and ``test_guarded`` runs them all.  tests/test_guarded_host.py checks that none is missing.

On a machine with a GPU run the file one family at a time (``-k conv-``, ``-k warp-``, ``-k infer-``, ``-k train-``, ``-k emo-``,
``-k audio-``, ``-k kp-``, ``-k motion-``, ``-k perc-``, ``-k bn-``, ``-k modes-``, ``-k clip-``, ``-k disc-``, ``-k equi-``, ``-k "four_floats or boundary or refused"``):
a stray store is the failure this file exists to find, and a family that has one should not be followed by another."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eamm_amd import _lib, _op
from closeness import close
from guarded import CASES, EXEMPT, GUARDED, Arena, Plain, case, run_three  # noqa: F401  (tests/test_guarded_host.py reads the registry here)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

def _call(name, *args, work=None):
    _op.call(name[len("eamm_op_"):], torch.device(DEV), *args, work=work)


def _rel(got, want):
    return float((got.detach().cpu().double() - want).abs().max()) / max(1.0, float(want.abs().max()))


# ---- eamm_op_conv: the case tables of test_gpu_ops.py and of the split-bf16 files ----------------------------------------------
import test_gpu_final_split
import test_gpu_ops
import test_gpu_ppoly_split
import test_gpu_wino4_split

CONV = ["3x3_mtail_ntail", "3x3_odd_linear", "3x3_up_odd_2x3", "3x3_up_odd_split", "3x3_splitk3_pool", "3x3_up_concat",
        "dma_odd_linear", "dma256_tails_res", "dma256_splitk3", "dma512x64", "skinny32_mtail", "skinny64_splitk5",
        "col7_ragged", "col7s_ragged", "col7_one_chunk",
        "patch_up_ragged", "ppoly_up_ragged", "ppoly_up_odd", "ppoly_split2_rag",
        "wino_tails_resid", "wino_ring5", "wino4_tails_resid", "wino4_split3_res", "wino4_pool_ragged", "wino4_ring4",
        "7x1_rowsplit", "7x7_head", "7x7_sigmoid", "7x7_first"]


def _conv_case(name, place):
    kw = test_gpu_ops.CASES[name]
    err, scale = test_gpu_ops.run_case(**kw, seed=hash(name) % 1000, place=place)
    assert err <= (6e-5 if kw.get("tile_n", 0) >= 2000 else 2e-5) * scale, (name, err, scale)     # test_conv_mfma_matches_torch's bars


for _n in CONV:
    case("conv-" + _n, ["eamm_op_conv"], functools.partial(_conv_case, _n))

_FUSED_FINAL = {"ragged": (3, 20, 24, 64), "narrow": (2, 40, 12, 64)}
for _n, _s in _FUSED_FINAL.items():
    case("conv-fused_final_" + _n, ["eamm_op_conv"],
         functools.partial(lambda n, s, place: test_gpu_ops.test_fused_final_layer_matches_torch(n, *s, place=place), _n, _s))


def _wino4_split_case(name, place):
    rel, err, top, _ = test_gpu_wino4_split.measure(name, place=place)
    assert rel <= 2.0 * test_gpu_wino4_split.PARENT[name] and err <= 6e-5 * max(1.0, top), (name, rel, err)


def _ppoly_split_case(name, place):
    rel, err, top, _ = test_gpu_ppoly_split.measure(name, place=place)
    assert rel <= 2.0 * test_gpu_ppoly_split.PARENT[name] and err <= 6e-5 * max(1.0, top), (name, rel, err)


def _final_split_case(name, place):
    err, _ = test_gpu_final_split.measure(name, place=place)
    assert err <= 2.0 * test_gpu_final_split.PARENT[name] and err <= 2e-6, (name, err)


case("conv-wino4_split_tails_resid", ["eamm_op_conv"], functools.partial(_wino4_split_case, "tails_resid"))
case("conv-ppoly_split_ragged", ["eamm_op_conv"], functools.partial(_ppoly_split_case, "ragged"))
case("conv-ppoly_split_concat", ["eamm_op_conv"], functools.partial(_ppoly_split_case, "concat"))
case("conv-final_split_ragged", ["eamm_op_conv"], functools.partial(_final_split_case, "ragged"))
case("conv-final_split_one_tile", ["eamm_op_conv"], functools.partial(_final_split_case, "one_tile"))


# ---- eamm_op_warp / _backward / _image ---------------------------------------------------------------------------------------------
import test_gpu_backward
import test_gpu_inference_ops as infer

_WARP = {"per_frame_source": dict(n=2, ns=2, hf=12, wf=20, C=32, h=12, w=20, seed=1),
         "resized_flow": dict(n=2, ns=1, hf=32, wf=32, C=64, h=16, w=16, seed=3)}


def _warp_case(name, place):
    got, want = test_gpu_ops._warp_case(**_WARP[name], place=place)
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max())), name


for _n in _WARP:
    case("warp-" + _n, ["eamm_op_warp"], functools.partial(_warp_case, _n))


@case("warp-backward_per_frame_source", ["eamm_op_warp_backward"], unstable=("d_features",))
def _warp_backward_case(place):
    """test_gpu_backward.test_warp_backward_matches_autograd's inputs, reference and bars, on the C entry.

    FINDING: d_features is not bit-stable between two plain calls -- warp_features_backward_kernel scatters it with float atomicAdd
    (warp.hip, one per corner and channel), as ATen's grid_sample backward does, so only the reference comparison holds for it.
    d_deformation and d_occlusion take one atomic per pixel onto zero at this channel count (8 lanes reduce first) and are bit-equal."""
    n, ns, h, w, c = 2, 2, 12, 20, 32
    feat, defo, om, gout = test_gpu_backward._warp_inputs(n, ns, h, w, c, True, 1)
    _, want_f, want_d, want_o = test_gpu_backward._warp_reference(feat, defo, om, gout)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    f, d, o = place(nhwc(feat), "in", name="features"), place(defo.contiguous(), "in", name="deformation"), place(om[:, 0].contiguous(), "in", name="occlusion")
    g = place(nhwc(gout), "in", name="grad_out")
    gf, gd, go = place((ns, h, w, c), "out", name="d_features"), place((n, h, w, 2), "out", name="d_deformation"), place((n, h, w), "out", name="d_occlusion")
    _call("eamm_op_warp_backward", f, d, o, g, n, ns, h, w, c, gf, gd, go)
    torch.cuda.synchronize()
    errs = {"d_feat": _rel(gf.permute(0, 3, 1, 2), want_f), "d_flow": _rel(gd, want_d), "d_occ": _rel(go, want_o[:, 0])}
    assert errs["d_feat"] <= 5e-6 and errs["d_flow"] <= 2e-5 and errs["d_occ"] <= 1e-5, errs


case("warp-image_per_frame_source", ["eamm_op_warp_image"], lambda place: infer._warp_image_case(2, 2, 12, 20, 12, 20, 3, 3, seed=1, place=place))
case("warp-image_resized_flow", ["eamm_op_warp_image"], lambda place: infer._warp_image_case(2, 2, 24, 40, 6, 10, 3, 3, seed=30, place=place))
case("warp-image_four_of_six_planes", ["eamm_op_warp_image"], lambda place: infer._warp_image_case(2, 1, 16, 16, 4, 4, 6, 4, seed=20, place=place))


# ---- the frozen inference path's small kernels: test_gpu_inference_ops.py at its tail-block parametrisations --------------------------
for _a in [(64, 3, 20, 36), (96, 1, 8, 8)]:
    case("infer-first7_%d_%d_%d_%d" % _a, ["eamm_op_first7"], functools.partial(lambda a, place: infer.test_first7_matches_conv2d(*a, place=place), _a))
for _a in [(30, 1, 17, 19), (10, 3, 12, 20)]:      # 323 pixels: a 67-thread tail block, K = 30; 240 pixels: less than a block
    case("infer-motion_head_K%d_%d_%d_%d" % _a, ["eamm_op_motion_head_infer"],
         functools.partial(lambda a, place: infer.test_motion_head_inference_kernel(*a, place=place), _a), nan_ok=("occlusion", "occ_out"))
for _a in [(10, 1, 70), (5, 1, 131), (16, 1, 5), (10, 0, 20)]:
    case("infer-motion_head_rowsplit_K%d_occ%d_w%d" % _a, ["eamm_op_motion_head_rowsplit", "eamm_op_motion_head_infer"],
         functools.partial(lambda a, place: infer.test_motion_head_rowsplit_kernel(*a, place=place), _a), nan_ok=("occlusion", "occ_out"))
for _w in (5, 131):
    case(f"infer-final_shift_sum_w{_w}", ["eamm_op_final_shift_sum"], functools.partial(lambda w, place: infer.test_final_shift_sum(w, place=place), _w))
case("infer-to_u8", ["eamm_op_to_u8"], lambda place: infer.test_to_u8_is_bit_exact_at_every_rounding_edge(place=place))
for _a in [(3, 20, 12, 2), (1, 8, 8, 1), (2, 32, 48, 4)]:
    case("infer-source_prepare_%d_%d_%d_inv%d" % _a, ["eamm_op_source_prepare", "eamm_op_antialias_down"],
         functools.partial(lambda a, place: infer._source_prepare_case(*a, seed=a[1], place=place), _a))
for _a in [(1, True), (3, False)]:
    case("infer-broadcast_features_ns%d_out2_%s" % _a, ["eamm_op_broadcast_features"],
         functools.partial(lambda a, place: infer.test_broadcast_features(*a, place=place), _a))
for _a in [(35, 35, 64), (32, 35, 32)]:
    case("infer-nchw_to_nhwc_pad_%d_%d_%d" % _a, ["eamm_op_nchw_to_nhwc_pad"],
         functools.partial(lambda a, place: infer._pad_case(2, a[0], a[1], 5, 7, a[2], seed=a[0], place=place), _a))
case("infer-nchw_to_nhwc_pad_grid_stride_remainder", ["eamm_op_nchw_to_nhwc_pad"], lambda place: infer._pad_case(33, 29, 29, 63, 65, 32, seed=2, place=place))
for _a in [(3, 49, 96), (1, 1, 64)]:
    case("infer-emo_avgpool_%d_%d_%d" % _a, ["eamm_op_emo_avgpool"], functools.partial(lambda a, place: infer.test_emo_avgpool(*a, place=place), _a))
for _b in (1, 9):
    case(f"infer-emo_embed_B{_b}", ["eamm_op_emo_embed"], functools.partial(lambda b, place: infer.test_emo_embed(b, place=place), _b))
for _a in [(9, 1260, 512, 300, 1), (8, 33, 7, 257, 1), (1, 64, 0, 64, 0)]:
    case("infer-emo_linear_%d_%d_%d_%d_%d" % _a, ["eamm_op_emo_linear"], functools.partial(lambda a, place: infer.test_emo_linear(*a, place=place), _a))
for _a in [(5, 28, 12), (2, 3, 5)]:
    case("infer-audio_conv1_%d_%d_%d" % _a, ["eamm_op_audio_conv1"], functools.partial(lambda a, place: infer.test_audio_conv1(*a, place=place), _a))
for _n in (1, 255, 257):
    case(f"infer-audio_scale_n{_n}", ["eamm_op_audio_scale"], functools.partial(lambda n, place: infer.test_audio_scale_is_bit_exact(n, place=place), _n))


# ---- the training convolutions with caller workspaces (eamm_op_train_conv.hip): workspaces at exactly the queried size ---------------
def _work(place, query, *dims, name="workspace"):
    n = getattr(_lib.lib(), query)(*dims)
    assert 0 < n < 2 ** 40, (query, dims, n)
    return place(int(n), "work", name=name)


def _train_conv_case(name, place):
    """test_gpu_backward.test_conv_backward_matches_autograd's inputs, float64 autograd reference and 2e-5 bar, with the three C
    entries autograd_ops.conv2d_same makes (forward, data gradient = the forward entry on the transposed filter, weight gradient)
    on placed operands.  Where the forward takes its F(4x4,3x3) form, eamm_op_conv_wgrad_saved starts from the transform the
    forward left in its workspace and must equal eamm_op_conv_wgrad bit for bit."""
    kw = test_gpu_backward.CONV_CASES[name]
    g = torch.Generator().manual_seed(100 + list(test_gpu_backward.CONV_CASES).index(name))
    B, H, W, cin, cout, k = kw["B"], kw["H"], kw["W"], kw["cin"], kw["cout"], kw["k"]
    x = torch.randn(B, cin, H, W, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g) if kw["bias"] else None
    gout = torch.randn(B, cout, H, W, generator=g)
    xr, wr = x.double().requires_grad_(), wt.double().requires_grad_()
    br = b.double().requires_grad_() if b is not None else None
    yr = F.conv2d(xr, wr, br, padding=k // 2)
    yr.backward(gout.double())

    L = _lib.lib()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xd, wd, gd = place(nhwc(x), "in", name="x"), place(wt, "in", name="weight"), place(nhwc(gout), "in", name="grad_out")
    bd = place(b, "in", name="bias") if b is not None else None
    y, dx = place((B, H, W, cout), "out", name="y"), place((B, H, W, cin), "out", name="dx")
    dw, db = place((cout, cin, k, k), "out", name="dw"), place((cout,), "out", name="db") if b is not None else None
    fwork = _work(place, "eamm_op_conv_dev_workspace_floats", B, H, W, cin, cout, k, k, name="forward workspace")
    _call("eamm_op_conv_dev", xd, B, H, W, cin, wd, bd, cout, k, k, 0, y, work=fwork)
    bwork = _work(place, "eamm_op_conv_dev_workspace_floats", B, H, W, cout, cin, k, k, name="dgrad workspace")
    _call("eamm_op_conv_dev", gd, B, H, W, cout, wd, None, cin, k, k, 1, dx, work=bwork)
    wwork = _work(place, "eamm_op_conv_wgrad_workspace_floats", B, H, W, cin, cout, k, k, name="wgrad workspace")
    _call("eamm_op_conv_wgrad", xd, gd, B, H, W, cin, cout, k, k, dw, db, work=wwork)
    torch.cuda.synchronize()
    errs = {"out": _rel(y.permute(0, 3, 1, 2), yr.detach()), "dx": _rel(dx.permute(0, 3, 1, 2), xr.grad), "dw": _rel(dw, wr.grad)}
    if b is not None:
        errs["db"] = _rel(db, br.grad)
    assert all(v <= 2e-5 for v in errs.values()), (name, errs)
    off = L.eamm_op_conv_saved_transform_offset(B, H, W, cin, cout, k, k)
    if off != 2 ** 64 - 1:
        dw1, db1 = place((cout, cin, k, k), "out", name="dw from saved"), place((cout,), "out", name="db from saved") if b is not None else None
        swork = _work(place, "eamm_op_conv_wgrad_workspace_floats", B, H, W, cin, cout, k, k, name="wgrad_saved workspace")
        _call("eamm_op_conv_wgrad_saved", C.c_void_p(fwork.data_ptr() + 4 * off), gd, B, H, W, cin, cout, dw1, db1, work=swork)
        torch.cuda.synchronize()
        assert torch.equal(dw, dw1) and (b is None or torch.equal(db, db1))
    return off


for _n in ("3x3_96_32", "3x3_pixels_not_multiple_of_32"):
    case("train-" + _n, ["eamm_op_conv_dev", "eamm_op_conv_wgrad"], functools.partial(_train_conv_case, _n))


@case("train-wino4_64_64_saved_transform", ["eamm_op_conv_dev", "eamm_op_conv_wgrad", "eamm_op_conv_wgrad_saved"])
def _train_conv_saved(place):
    """The smallest case of the table whose forward saves its transform (2048 tiles): the only ones eamm_op_conv_wgrad_saved accepts."""
    assert _train_conv_case("wino4_64_64", place) != 2 ** 64 - 1


@case("train-thin_1_21_37_32", ["eamm_op_conv7_thin", "eamm_op_conv7_thin_wgrad", "eamm_op_final_conv_sigmoid"])
def _thin_case(place, B=1, H=21, W=37, N=32):
    """test_gpu_backward.test_thin_7x7_layers_match_autograd at its ragged shape: the same inputs, autograd reference and 2e-5 bar;
    every launch gets a workspace of its own at the queried size (7 N 32 floats for eamm_op_final_conv_sigmoid, as the header says)."""
    g = torch.Generator().manual_seed(31 + H)
    q = "eamm_op_conv7_thin_workspace_floats"
    thin4 = lambda t: F.pad(t.permute(0, 2, 3, 1), (0, 1)).contiguous()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    x3 = torch.randn(B, 3, H, W, generator=g)
    w1 = torch.randn(N, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    b1 = 0.1 * torch.randn(N, generator=g)
    gy = torch.randn(B, N, H, W, generator=g)
    wr = w1.double().requires_grad_()
    yr = F.conv2d(x3.double(), wr, b1.double(), padding=3)
    yr.backward(gy.double())
    x4, w1_d, b1_d = place(thin4(x3), "in", name="x4"), place(w1, "in", name="w first"), place(b1, "in", name="b first")
    y = place((B, H, W, N), "out", name="y first")
    _call("eamm_op_conv7_thin", x4, w1_d, b1_d, B, H, W, N, 0, y, work=_work(place, q, B, H, W, N, name="workspace first fwd"))
    dw = place((N, 3, 7, 7), "out", name="dw first")
    gy_d = place(nhwc(gy), "in", name="grad y")
    _call("eamm_op_conv7_thin_wgrad", x4, gy_d, B, H, W, N, 1, dw, work=_work(place, q, B, H, W, N, name="workspace first wgrad"))
    torch.cuda.synchronize()
    errs = {"first_fwd": _rel(y.permute(0, 3, 1, 2), yr.detach()), "first_dw": _rel(dw, wr.grad)}

    x = torch.randn(B, N, H, W, generator=g)
    w2 = torch.randn(3, N, 7, 7, generator=g) * (2.0 / (49 * N)) ** 0.5
    g3 = torch.randn(B, 3, H, W, generator=g)
    xr, wr2 = x.double().requires_grad_(), w2.double().requires_grad_()
    F.conv2d(xr, wr2, None, padding=3).backward(g3.double())
    g4, w2_d, x_d = place(thin4(g3), "in", name="g4"), place(w2, "in", name="w final"), place(nhwc(x), "in", name="x final")
    dx = place((B, H, W, N), "out", name="dx final")
    _call("eamm_op_conv7_thin", g4, w2_d, None, B, H, W, N, 1, dx, work=_work(place, q, B, H, W, N, name="workspace final dgrad"))
    dw2 = place((3, N, 7, 7), "out", name="dw final")
    _call("eamm_op_conv7_thin_wgrad", g4, x_d, B, H, W, N, 0, dw2, work=_work(place, q, B, H, W, N, name="workspace final wgrad"))
    torch.cuda.synchronize()
    errs.update({"final_dx": _rel(dx.permute(0, 3, 1, 2), xr.grad), "final_dw": _rel(dw2, wr2.grad)})
    b2 = 0.1 * torch.randn(3, generator=g)
    y3 = place((B, 3, H, W), "out", name="y final")
    _call("eamm_op_final_conv_sigmoid", x_d, w2_d, place(b2, "in", name="b final"), B, H, W, N, y3, work=place(7 * N * 32, "work", name="packed filter"))
    torch.cuda.synchronize()
    errs["final_fwd"] = _rel(y3, torch.sigmoid(F.conv2d(x.double(), w2.double(), b2.double(), padding=3)))
    assert all(v <= 2e-5 for v in errs.values()), errs


# ---- Emotion_k's trunk operators: test_gpu_emotion_backward.py's references and bar -----------------------------------------------------
import test_gpu_emotion_backward as emo


def _conv_s2_case(k, shape, place):
    b, h, w, cin, cout = shape
    x, wt, gy, ref = emo.conv_reference(k, shape)
    (y64, dx64, dw64), (y32, dx32, dw32) = ref[torch.float64], ref[torch.float32]
    xd, wd, gd = place(emo.nhwc(x), "in", name="x"), place(wt, "in", name="weight"), place(emo.nhwc(gy), "in", name="grad_out")
    y, dx, dw = place((b, h // 2, w // 2, cout), "out", name="y"), place((b, h, w, cin), "out", name="dx"), place((cout, cin, k, k), "out", name="dw")
    _call("eamm_op_conv_s2", xd, b, h, w, cin, wd, cout, k, y, work=_work(place, "eamm_op_conv_s2_workspace_floats", b, h, w, cin, cout, k, name="forward workspace"))
    _call("eamm_op_conv_s2_dgrad", gd, b, h, w, cin, wd, cout, k, dx,
          work=_work(place, "eamm_op_conv_s2_dgrad_workspace_floats", b, h, w, cin, cout, k, name="dgrad workspace"))
    _call("eamm_op_conv_s2_wgrad", xd, gd, b, h, w, cin, cout, k, dw,
          work=_work(place, "eamm_op_conv_s2_wgrad_workspace_floats", b, h, w, cin, cout, k, name="wgrad workspace"))
    torch.cuda.synchronize()
    close(y, emo.nhwc(y64), emo.nhwc(y32), f"k{k} {shape} forward")
    close(dx, emo.nhwc(dx64), emo.nhwc(dx32), f"k{k} {shape} data gradient")
    close(dw, dw64, dw32, f"k{k} {shape} weight gradient")


for _k in (1, 3):
    for _s in [(1, 2, 2, 32, 32), (9, 10, 6, 32, 32), (1, 4, 4, 256, 512)]:
        case("emo-conv_s2_k%d_%s" % (_k, "x".join(map(str, _s))), ["eamm_op_conv_s2", "eamm_op_conv_s2_dgrad", "eamm_op_conv_s2_wgrad"],
             functools.partial(_conv_s2_case, _k, _s))


@case("emo-maxpool_1_2_2_64", ["eamm_op_emo_maxpool", "eamm_op_emo_maxpool_backward"])
def _emo_maxpool_case(place, shape=(1, 2, 2, 64)):
    b, h, w, c = shape
    x, gy, ref = emo.pool_case(shape, False)
    xd, gd = place(emo.nhwc(x), "in", name="x"), place(emo.nhwc(gy), "in", name="grad_out")
    y, dx = place((b, h // 2, w // 2, c), "out", name="y"), place((b, h, w, c), "out", name="dx")
    _call("eamm_op_emo_maxpool", xd, b, h, w, c, y)
    _call("eamm_op_emo_maxpool_backward", xd, gd, b, h, w, c, dx)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), emo.nhwc(ref[torch.float32][0]))
    want = emo.nhwc(ref[torch.float64][1])
    assert bool(((dx.cpu() != 0) == (want != 0)).all())
    close(dx, want, emo.nhwc(ref[torch.float32][1]), f"maxpool {shape}")


case("emo-maxpool_2_6_10_64", ["eamm_op_emo_maxpool", "eamm_op_emo_maxpool_backward"], functools.partial(_emo_maxpool_case, shape=(2, 6, 10, 64)))


def _emo_final_case(B, place):
    """test_gpu_emotion_backward.test_emo_final_forward_and_gradients' inputs and float64 / float32 ATen references."""
    g = torch.Generator().manual_seed(21 + B)
    a = torch.randn(B, 64, generator=g).abs()
    w98 = 0.5 * torch.randn(98, generator=g)
    gv, gj = torch.randn(B, 4, 2, generator=g), torch.randn(B, 4, 2, 2, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        al, wl = a.to(dtype).clone().requires_grad_(), w98.to(dtype).clone().requires_grad_()
        c1w, c1b, c2w, c2b, c3w, c3b = wl[0:8].view(2, 1, 4), wl[8:10], wl[10:42].view(4, 2, 4), wl[42:46], wl[46:94].view(4, 4, 3), wl[94:98]
        y = torch.relu(F.max_pool1d(F.conv1d(al[:, None], c1w, c1b, 2, 1), 2, 2))
        r = F.conv1d(torch.relu(F.conv1d(y, c2w, c2b, 2, 1)), c3w, c3b)
        value, jac = r[:, :, :2], r[:, :, 2:].reshape(B, 4, 2, 2)
        ((value * gv.to(dtype)).sum() + (jac * gj.to(dtype)).sum()).backward()
        ref[dtype] = (value.detach(), jac.detach(), al.grad, wl.grad)
    ad, wd, gvd, gjd = place(a, "in", name="a"), place(w98, "in", name="w98"), place(gv, "in", name="g_value"), place(gj, "in", name="g_jacobian")
    value, jac = place((B, 4, 2), "out", name="value"), place((B, 4, 2, 2), "out", name="jacobian")
    ga, gw = place((B, 64), "out", name="grad a"), place((98,), "out", name="grad w98")
    _call("eamm_op_emo_final", ad, wd, B, value, jac)
    _call("eamm_op_emo_final_backward", ad, wd, gvd, gjd, B, ga, gw, work=_work(place, "eamm_op_emo_final_workspace_floats", B))
    torch.cuda.synchronize()
    for name, got, i in (("value", value, 0), ("jacobian", jac, 1), ("grad input", ga, 2), ("grad weights", gw, 3)):
        close(got, ref[torch.float64][i], ref[torch.float32][i], f"emo_final B={B} {name}")


for _b in (1, 9):
    case(f"emo-final_B{_b}", ["eamm_op_emo_final", "eamm_op_emo_final_backward"], functools.partial(_emo_final_case, _b))


# ---- AT_net2's operators: test_gpu_audio_backward.py's references and bar ---------------------------------------------------------------
import test_gpu_audio_backward as aud


def _lstm_case(shape, place):
    """The three entries as audio_ops._LstmLayerFunction calls them; the torch steps between them (h_{t-1}, the gate pre-activations, dW_hh
    from dxproj) stay torch, on the placed tensors."""
    n, t = shape
    xproj, whh, gy, ref = aud.lstm_reference(shape)
    (y64, dx64, dw64), (y32, dx32, dw32) = ref[torch.float64], ref[torch.float32]
    xd, wd, gd = place(xproj, "in", name="xproj"), place(whh, "in", name="w_hh"), place(gy, "in", name="grad_y")
    y = place((n, t, 256), "out", name="y")
    _call("eamm_op_lstm_forward", xd, wd, n, t, y, work=_work(place, "eamm_op_lstm_workspace_floats", n, t, name="forward workspace"))
    h_prev = torch.cat([y.new_zeros(n, 1, 256), y[:, :-1]], dim=1).reshape(n * t, 256)
    gates = place(torch.addmm(xd.reshape(n * t, 1024), h_prev, wd.t()).view(n, t, 1024), "inout", name="gates")
    c, gx = place((n, t, 256), "out", name="c"), place((n, t, 1024), "out", name="grad xproj")
    _call("eamm_op_lstm_scan", gates, n, t, c)
    _call("eamm_op_lstm_backward", gates, c, wd, gd, n, t, gx, work=_work(place, "eamm_op_lstm_backward_workspace_floats", n, t, name="backward workspace"))
    _call("eamm_op_lstm_check")
    gw = torch.matmul(gx.reshape(n * t, 1024).t(), h_prev)
    close(y, y64, y32, f"lstm {shape} y")
    close(gx, dx64, dx32, f"lstm {shape} dxproj")
    close(gw, dw64, dw32, f"lstm {shape} dW_hh")


for _s in [(1, 1), (3, 5), (8, 5)]:
    case("audio-lstm_N%d_T%d" % _s, ["eamm_op_lstm_forward", "eamm_op_lstm_scan", "eamm_op_lstm_backward"], functools.partial(_lstm_case, _s))


def _deconv_case(shape, place):
    """audio_ops.conv_transpose4s2_nhwc's three entries; channels zero-padded to the granule of 32 as that wrapper pads them."""
    b, h, w, cin, cout = shape
    x, wt, bias, gy, ref = aud.deconv_reference(shape)
    (y64, dx64, dw64, db64), (y32, dx32, dw32, db32) = ref[torch.float64], ref[torch.float32]
    cp = _op.round_up(cout, 32)
    assert cin % 32 == 0
    xd = place(aud.nhwc(x), "in", name="x")
    wd = place(F.pad(wt, (0, 0, 0, 0, 0, cp - cout)), "in", name="weight")
    bd = place(F.pad(bias, (0, cp - cout)), "in", name="bias")
    gd = place(F.pad(aud.nhwc(gy), (0, cp - cout)), "in", name="grad_out")
    y, dx = place((b, 2 * h, 2 * w, cp), "out", name="y"), place((b, h, w, cin), "out", name="dx")
    dw, db = place((cin, cp, 4, 4), "out", name="dw"), place((cp,), "out", name="db")
    _call("eamm_op_deconv4s2", xd, b, h, w, cin, wd, bd, cp, y, work=_work(place, "eamm_op_deconv4s2_workspace_floats", b, h, w, cin, cp, name="forward workspace"))
    _call("eamm_op_deconv4s2_dgrad", gd, b, h, w, cin, wd, cp, dx,
          work=_work(place, "eamm_op_deconv4s2_dgrad_workspace_floats", b, h, w, cin, cp, name="dgrad workspace"))
    _call("eamm_op_deconv4s2_wgrad", xd, gd, b, h, w, cin, cp, dw, db,
          work=_work(place, "eamm_op_deconv4s2_wgrad_workspace_floats", b, h, w, cin, cp, name="wgrad workspace"))
    torch.cuda.synchronize()
    close(y[..., :cout], aud.nhwc(y64), aud.nhwc(y32), f"deconv {shape} forward")
    close(dx, aud.nhwc(dx64), aud.nhwc(dx32), f"deconv {shape} data gradient")
    close(dw[:, :cout], dw64, dw32, f"deconv {shape} weight gradient")
    close(db[:cout], db64, db32, f"deconv {shape} bias gradient")


for _s in [(1, 1, 1, 32, 32), (3, 4, 4, 64, 35), (2, 5, 3, 256, 128)]:
    case("audio-deconv4s2_" + "x".join(map(str, _s)), ["eamm_op_deconv4s2", "eamm_op_deconv4s2_dgrad", "eamm_op_deconv4s2_wgrad"],
         functools.partial(_deconv_case, _s))


@case("audio-maxpool_3_3_3_4_1_1", ["eamm_op_audio_maxpool", "eamm_op_audio_maxpool_backward"])
def _audio_maxpool_case(place, shape=(3, 3, 3, 4, 1, 1)):
    """test_maxpool3_forward_is_bit_equal_and_backward_equal_without_ties' inputs: bit-equal to ATen both ways."""
    b, h, w, c, sy, sx = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randperm(b * h * w * c, generator=g).float().reshape(b, c, h, w) / 64.0
    xr = x.clone().requires_grad_()
    yr = F.max_pool2d(xr, 3, stride=(sy, sx))
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd, gd = place(aud.nhwc(x), "in", name="x"), place(aud.nhwc(gy), "in", name="grad_out")
    y, dx = place(tuple(aud.nhwc(yr).shape), "out", name="y"), place((b, h, w, c), "out", name="dx")
    _call("eamm_op_audio_maxpool", xd, b, h, w, c, sy, sx, y)
    _call("eamm_op_audio_maxpool_backward", xd, gd, b, h, w, c, sy, sx, dx)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), aud.nhwc(yr.detach())) and torch.equal(dx.cpu(), aud.nhwc(xr.grad))


case("audio-maxpool_2_26_5_512_2_2", ["eamm_op_audio_maxpool", "eamm_op_audio_maxpool_backward"],
     functools.partial(_audio_maxpool_case, shape=(2, 26, 5, 512, 2, 2)))


# ---- the key-point heads' reduction: test_gpu_kp_backward.py's expression, inputs and bar ---------------------------------------------------
import test_gpu_kp_backward as kpb


def _kp_head_case(h, w, pad, B, place, K=10, njm=10):
    logits = kpb.head_logits(h, w, K, njm, B)
    cs = logits.shape[3]
    oh, ow = h - 6 + 2 * pad, w - 6 + 2 * pad
    ref = {}
    for dtype in (torch.float64, torch.float32):
        leaf = logits.clone().to(dtype).requires_grad_()
        ref[dtype] = (leaf, kpb.head_expression(leaf, K, njm, pad, kpb.T))
    out64 = ref[torch.float64][1]
    g = torch.Generator().manual_seed(5)
    weights = {k: torch.randn(v.shape, generator=g) for k, v in out64.items()}
    x = place(logits, "in", name="logits")
    value, jac, heat, stats = (place(s, "out", name=n) for n, s in (("value", (B, K, 2)), ("jacobian", (B, K, 2, 2)), ("heatmap", (B, K, oh, ow)),
                                                                   ("stats", (B, K, 2))))
    _call("eamm_op_kp_head", x, B, K, njm, h, w, cs, pad, kpb.T, value, jac, heat, stats, work=_work(place, "eamm_op_kp_head_workspace_floats", B, K, name="forward workspace"))
    torch.cuda.synchronize()
    for k, got in (("value", value), ("jacobian", jac), ("heatmap", heat)):
        kpb.close(got, out64[k], ref[torch.float32][1][k], f"forward {k}", kpb.TIGHT_MIN_REL)
    want = {}
    for dtype, (leaf, o) in ref.items():
        kpb.weighted(o, weights, ("value", "jacobian", "heatmap")).backward()
        want[dtype] = leaf.grad
    gv, gj, gh = (place(weights[k], "in", name="g_" + k) for k in ("value", "jacobian", "heatmap"))
    grad = place((B, h, w, cs), "out", name="grad logits")
    _call("eamm_op_kp_head_backward", x, stats, value, jac, gv, gj, gh, B, K, njm, h, w, cs, pad, kpb.T, grad,
          work=_work(place, "eamm_op_kp_head_workspace_floats", B, K, name="backward workspace"))
    torch.cuda.synchronize()
    kpb.close(grad, want[torch.float64], want[torch.float32], "grad_logits", kpb.TIGHT_MIN_REL)


for _b in (1, 9):
    # (7, 7, 0): a window of one pixel, whose soft-argmax is the reference's 0 / 0 -- the value and what its gradient reaches are NaN
    # there, exactly where the reference's are (kpb.close demands it)
    case(f"kp-head_7x7_pad0_B{_b}", ["eamm_op_kp_head", "eamm_op_kp_head_backward"], functools.partial(_kp_head_case, 7, 7, 0, _b),
         nan_ok=("value", "grad logits"))
    case(f"kp-head_10x13_pad1_B{_b}", ["eamm_op_kp_head", "eamm_op_kp_head_backward"], functools.partial(_kp_head_case, 10, 13, 1, _b))


# ---- the dense-motion operators: test_gpu_motion_ops_shapes.py's cases, references and bars --------------------------------------------
import test_gpu_motion_ops_shapes as ms


def _records_on_device(inp):
    """The records and the leaves they came from, through the autograd wrapper on plain tensors: the key-point gradients are taken
    by sending the guarded entry's record gradient back through it, as the null-pointer tests of that file do."""
    from eamm_amd import motion_ops
    kdd, ksd = ms._to_dev(inp["kd"]), ms._to_dev(inp["ks"])
    return kdd, ksd, motion_ops.kp_records(kdd, ksd)


def _motion_front_case(name, cpad, place):
    inp = ms._case_inputs(name)
    n, k, h, w = inp["n"], inp["k"], inp["h"], inp["w"]
    want, floor = ms._front_reference(name)
    kdd, ksd, rec_leaf = _records_on_device(inp)
    small_dev = ms._small_nhwc(inp)      # (sent to the device in front of the first placement: a side-stream run must not wait for it after)
    rec, small = place(rec_leaf.detach(), "in", name="records"), place(small_dev, "in", name="small")
    hg, sdef = place((n, h, w, cpad), "out", name="hourglass input"), place((n, k + 1, 3, h, w), "out", name="sparse_deformed")
    _call("eamm_op_motion_front", rec, small, n, k, h, w, ms.VAR, cpad, hg, sdef)
    g_hg, g_sd = place(ms._hg_line(inp["g_hg"], cpad, 1), "in", name="grad hourglass input"), place(inp["g_sd"], "in", name="grad sparse_deformed")
    g_small, g_rec = place((n, h, w, 4), "out", name="d small"), place((n, k, 8), "out", name="d records")
    _call("eamm_op_motion_front_backward", rec, small, n, k, h, w, ms.VAR, cpad, g_hg, g_sd, g_small, g_rec,
          work=_work(place, "eamm_op_motion_workspace_floats", n, k, h, w))
    torch.cuda.synchronize()
    assert float(g_small[..., 3].abs().max()) == 0.0 and (cpad == 4 * (k + 1) or float(hg[..., 4 * (k + 1):].abs().max()) == 0.0)
    rec_leaf.backward(g_rec.clone())
    got = {"hourglass input": ms._hg_planes(hg, k), "sparse_deformed": sdef, "d small": g_small[..., :3].permute(0, 3, 1, 2)}
    ms._compare(f"guarded front {name}", ms._kp_grads_dev(got, kdd, ksd), want, floor)


def _motion_head_case(name, place):
    inp = ms._case_inputs(name)
    n, k, h, w = inp["n"], inp["k"], inp["h"], inp["w"]
    hd, want, floor = ms._head_case(name)
    ld, ldo = ms.CASES[name]["head"]
    assert isinstance(ldo, int) and not hd["stacked"]
    kdd, ksd, rec_leaf = _records_on_device(inp)
    rec, lm, lo = place(rec_leaf.detach(), "in", name="records"), place(hd["lm"], "in", name="mask logits"), place(hd["lo"], "in", name="occlusion logits")
    mask, defo, occ = place((n, k + 1, h, w), "out", name="mask"), place((n, h, w, 2), "out", name="deformation"), place((n, h, w), "out", name="occlusion")
    _call("eamm_op_motion_head", lm, ld, lo, ldo, rec, n, k, h, w, mask, defo, occ)
    g_m, g_d, g_o = place(hd["g_m"], "in", name="grad mask"), place(hd["g_d"], "in", name="grad deformation"), place(hd["g_o"], "in", name="grad occlusion")
    g_lm, g_lo, g_rec = place((n, h, w, ld), "out", name="d mask logits"), place((n, h, w, ldo), "out", name="d occlusion logits"), place((n, k, 8), "out", name="d records")
    _call("eamm_op_motion_head_backward", mask, occ, rec, n, k, h, w, g_m, g_d, g_o, g_lm, ld, g_lo, ldo, g_rec,
          work=_work(place, "eamm_op_motion_workspace_floats", n, k, h, w))
    torch.cuda.synchronize()
    if ld > k + 1:
        assert float(g_lm[..., k + 1:].abs().max()) == 0.0
    if ldo > 1:
        assert float(g_lo[..., 1:].abs().max()) == 0.0
    rec_leaf.backward(g_rec.clone())
    got = {"mask": mask, "deformation": defo, "occlusion": occ, "d mask logits": g_lm[..., :k + 1], "d occlusion logits": g_lo[..., 0]}
    ms._compare(f"guarded head {name}", ms._kp_grads_dev(got, kdd, ksd), want, floor)


# A: 17 x 15 = 255 pixels, the smallest map that is not square (one dead lane; logit rows of 11 floats); D: 13 x 20 = 260, K = 15
for _n in ("A", "D"):
    # FINDING (documented in motion_backward.hip's header, test_record_gradients_are_deterministic): the small image's gradient is
    # accumulated with float atomics and is not bit-stable between two plain calls; only its reference comparison holds
    case(f"motion-front_{_n}", ["eamm_op_motion_front", "eamm_op_motion_front_backward"], functools.partial(_motion_front_case, _n, 64), unstable=("d small",))
    case(f"motion-head_{_n}", ["eamm_op_motion_head", "eamm_op_motion_head_backward"], functools.partial(_motion_head_case, _n))


@case("motion-kp_records_150", ["eamm_op_kp_records", "eamm_op_kp_records_backward"])
def _kp_records_case(place):
    """test_kp_records_blocks_conditioning_and_partial_gradients' "150_records": two 128-thread blocks in the backward."""
    from eamm_amd.weights import synthetic_keypoints
    n, k = 5, 30
    kd, ks = synthetic_keypoints(n, k, seed=13), synthetic_keypoints(n, k, seed=11)
    g_rec = torch.randn(n, k, 8, generator=torch.Generator().manual_seed(3))
    want, floor = ms._want_and_floor(lambda dt: ms._records_eval(kd, ks, g_rec, dt, True), unit_scale=False)
    kdv, kdj, ksv, ksj = (place(t, "in", name=nm) for nm, t in (("kd value", kd["value"]), ("kd jacobian", kd["jacobian"]), ("ks value", ks["value"]),
                                                                ("ks jacobian", ks["jacobian"])))
    rec, flag = place((n, k, 8), "out", name="records"), place(torch.zeros(1, dtype=torch.int32), "inout", name="singular flag")
    _call("eamm_op_kp_records", kdv, kdj, ksv, ksj, n, k, rec, flag)
    gr = place(g_rec, "in", name="grad records")
    outs = {nm: place(sh, "out", name=nm) for nm, sh in (("d kp_driving.value", (n, k, 2)), ("d kp_source.value", (n, k, 2)),
                                                        ("d kp_driving.jacobian", (n, k, 2, 2)), ("d kp_source.jacobian", (n, k, 2, 2)))}
    _call("eamm_op_kp_records_backward", kdj, ksj, gr, n, k, outs["d kp_driving.value"], outs["d kp_source.value"], outs["d kp_driving.jacobian"],
          outs["d kp_source.jacobian"])
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ms._compare("guarded kp_records", dict(outs, records=rec), want, floor, unit_scale=False)


def _antialias_case(b, hh, ww, inv, place):
    """test_antialias_down_shapes' reference and 2e-6 bar, forward and backward entries."""
    from eamm_amd.weights import antialias_kernel
    gen = torch.Generator().manual_seed(b * 1000 + hh)
    src = torch.rand(b, 3, hh, ww, generator=gen)
    wgt = antialias_kernel(3)
    xr = src.double().requires_grad_()
    ref = xr if inv == 1 else F.conv2d(F.pad(xr, (6, 6, 6, 6)), wgt.double(), groups=3)[:, :, ::4, ::4]
    g = torch.randn(ref.shape, generator=gen)
    (ref * g.double()).sum().backward()
    xd, wd = place(src, "in", name="source"), place(wgt, "in", name="aa kernel") if inv != 1 else None
    small = place((b, hh // inv, ww // inv, 4), "out", name="small")
    _call("eamm_op_antialias_down", xd, wd, b, hh, ww, inv, small)
    gs = place(F.pad(g.permute(0, 2, 3, 1), (0, 1)).contiguous(), "in", name="grad small")
    grad = place((b, 3, hh, ww), "out", name="grad source")
    _call("eamm_op_antialias_down_backward", gs, wd, b, hh, ww, inv, grad)
    torch.cuda.synchronize()
    assert float(small[..., 3].abs().max()) == 0.0
    assert ms._rel(small[..., :3].permute(0, 3, 1, 2), ref) <= 2e-6 and ms._rel(grad, xr.grad) <= 2e-6


for _a in [(1, 20, 12, 4), (1, 8, 8, 4), (2, 12, 20, 1)]:
    case("motion-antialias_%d_%d_%d_inv%d" % _a, ["eamm_op_antialias_down", "eamm_op_antialias_down_backward"], functools.partial(_antialias_case, *_a))


# ---- the perceptual loss's small kernels: test_gpu_perceptual_ops.py's references, closeness.close ----------------------------------------
import test_gpu_perceptual_ops as perc
from perceptual_common import _MEAN, _STD, ref_level


def _vgg_input_case(inv, place, shape=(2, 3, 40, 24)):
    from eamm_amd.weights import antialias_kernel
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(3))
    b, _, hh, ww = shape
    r = perc.rnd(b, hh // inv, ww // inv, 32, seed=4)
    mean, std, k = torch.tensor(_MEAN), torch.tensor(_STD), antialias_kernel(3)
    want = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()
        norm = ((ref_level(xr, inv) - mean.to(dt).reshape(1, 3, 1, 1)) / std.to(dt).reshape(1, 3, 1, 1)).permute(0, 2, 3, 1)
        (norm * r[..., :3].to(dt)).sum().backward()
        want[dt] = (norm.detach(), xr.grad)
    xd, kd, md, sd = place(x, "in", name="image"), place(k, "in", name="aa kernel"), place(mean, "in", name="mean"), place(std, "in", name="std")
    out, level = place((b, hh // inv, ww // inv, 32), "out", name="normalised"), place((b, 3, hh // inv, ww // inv), "out", name="level")
    _call("eamm_op_vgg_input", xd, kd, md, sd, b, hh, ww, inv, out, None)
    _call("eamm_op_vgg_input", xd, kd, None, None, b, hh, ww, inv, None, level)
    gd, grad = place(r, "in", name="grad normalised"), place((b, 3, hh, ww), "out", name="grad image")
    _call("eamm_op_vgg_input_backward", gd, 32, None, kd, sd, b, hh, ww, inv, grad)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out[..., 3:])) == 0
    close(out[..., :3], want[torch.float64][0], want[torch.float32][0], f"vgg_input {shape} 1/{inv}")
    close(grad, want[torch.float64][1], want[torch.float32][1], f"vgg_input backward {shape} 1/{inv}")
    close(level, ref_level(x.double(), inv), ref_level(x, inv), f"level {shape} 1/{inv}")


for _i in (1, 8):
    case(f"perc-vgg_input_inv{_i}", ["eamm_op_vgg_input", "eamm_op_vgg_input_backward"], functools.partial(_vgg_input_case, _i))


@case("perc-relu_pool_1_7_5_32", ["eamm_op_relu_pool", "eamm_op_relu_pool_backward"])
def _relu_pool_case(place, shape=(1, 7, 5, 32)):
    """test_relu_pool's planted input and references, mode "both"; x is written in place."""
    x = perc.planted(shape, seed=6)
    b, h, w, c = shape
    ry, rp = perc.rnd(*shape, seed=7), perc.rnd(b, h // 2, w // 2, c, seed=8)
    want = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()
        y = F.relu(xr)
        p = F.max_pool2d(y.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        ((y * ry.to(dt)).sum() + (p * rp.to(dt)).sum()).backward()
        want[dt] = (y.detach(), p.detach(), xr.grad)
    xd, pooled = place(x, "inout", name="x"), place((b, h // 2, w // 2, c), "out", name="pooled")
    _call("eamm_op_relu_pool", xd, b, h, w, c, pooled)
    dy, dp, dx = place(ry, "in", name="dy"), place(rp, "in", name="dp"), place(shape, "out", name="dx")
    _call("eamm_op_relu_pool_backward", xd, dy, dp, b, h, w, c, dx)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), want[torch.float32][0]) and torch.equal(pooled.cpu(), want[torch.float32][1])
    close(dx, want[torch.float64][2], want[torch.float32][2], f"relu_pool backward {shape}")


@case("perc-l1_pair_1155", ["eamm_op_l1_pair", "eamm_op_l1_pair_backward"])
def _l1_pair_case(place, shape=(3, 5, 7, 11)):
    """test_l1_pair at 1155 elements: two workgroups and a tail of three behind the last float4."""
    a, b = perc.rnd(*shape, seed=12), perc.rnd(*shape, seed=13)
    a.reshape(-1)[::7] = b.reshape(-1)[::7]
    w, n = 10.0, a.numel()
    want64, want32 = w * (a.double() - b.double()).abs().mean(), w * (a - b).abs().mean()
    g64 = (w / n) * torch.sign(a.double() - b.double())
    ad, bd = place(a, "in", name="a"), place(b, "in", name="b")
    value, g = place(1, "out", name="value"), place(shape, "out", name="gradient")
    _call("eamm_op_l1_pair", ad, bd, n, w, value, g, work=_work(place, "eamm_op_l1_pair_workspace_floats", n))
    gv, ga = place(torch.tensor([3.0]), "in", name="grad value"), place(shape, "out", name="grad a")
    _call("eamm_op_l1_pair_backward", g, n, gv, ga)
    torch.cuda.synchronize()
    err, bar = abs(float(value) - float(want64)), max(4 * abs(float(want32) - float(want64)), 2e-5 * abs(float(want64)))
    assert err <= bar, (err, bar)
    close(ga, 3.0 * g64, (3.0 * g64).float(), f"l1_pair gradient {shape}")
    assert int(torch.count_nonzero(ga.reshape(-1)[::7])) == 0


# ---- training-mode BatchNorm (eamm_bn_*: no device index, the stream last, errors through eamm_bn_last_error) -------------------------------
def _bn(name, *args):
    argv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(_lib.lib(), name)(*argv, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc, _lib.lib().eamm_bn_last_error())


def _packed_sums_are_written(sums, c):
    """The packed [6C+2] layout: 2C+2 floats, then the same 2C totals as doubles.  A double's low word read as a float may look like
    a NaN, so the arena's own NaN test does not apply to these operands; this one reads each part as what it is."""
    assert bool(torch.isfinite(sums[:2 * c + 2]).all()) and bool(torch.isfinite(sums[2 * c + 2:].cpu().view(torch.float64)).all())


def _bn_nchw_case(shape, place):
    """tests/test_batchnorm.py's awkward shapes, inputs, float64 references and bars (test_gpu_gradients_against_float64_autograd,
    test_gpu_statistics_against_float64), on the six layout-free / NCHW entries in the order SynchronizedBatchNorm2d calls them
    (mode EAMM_BN_SINGLE).  The workspace promises 8-byte alignment only; a 16-byte skew satisfies it."""
    rs = np.random.RandomState(sum(shape) + 1)
    N, c, H, W = shape
    hw, n = H * W, N * H * W
    x = torch.from_numpy((rs.standard_normal(shape) * rs.uniform(0.5, 2, (1, c, 1, 1)) + rs.standard_normal((1, c, 1, 1))).astype(np.float32))
    dy = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    w = torch.from_numpy(rs.uniform(0.5, 1.5, c).astype(np.float32))
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), torch.zeros(c, dtype=torch.float64, requires_grad=True)
    yr = F.batch_norm(xr, None, None, wr, br, True, 0.1, 1e-5)
    yr.backward(dy.double())
    mean64, var64 = x.double().mean(dim=(0, 2, 3)), x.double().var(dim=(0, 2, 3), unbiased=False)

    xd, dyd, wd, bd = place(x, "in", name="x"), place(dy, "in", name="dy"), place(w, "in", name="weight"), place(torch.zeros(c), "in", name="bias")
    rm, rv = place(torch.zeros(c), "inout", name="running_mean"), place(torch.ones(c), "inout", name="running_var")
    sums, bsums = place(6 * c + 2, "out", name="sums"), place(6 * c + 2, "out", name="backward sums")
    mean, scale, inv = place(c, "out", name="mean"), place(c, "out", name="scale"), place(c, "out", name="inv_std")
    y, dx, dw, db, coef = place(shape, "out", name="y"), place(shape, "out", name="dx"), place(c, "out", name="dweight"), place(c, "out", name="dbias"), place(3 * c, "out", name="coef")
    q = int(_lib.lib().eamm_bn_workspace_floats(N, c, hw))
    _bn("eamm_bn_local_sums", xd, N, c, hw, sums, place(q, "work", name="forward workspace"))
    _bn("eamm_bn_finalize", sums, c, 1e-5, 0.1, 1, wd, rm, rv, mean, scale, inv)
    _bn("eamm_bn_apply", xd, mean, scale, bd, N, c, hw, y)
    _bn("eamm_bn_backward_sums", xd, dyd, mean, N, c, hw, bsums, place(q, "work", name="backward workspace"))
    _bn("eamm_bn_backward_finalize", bsums, bsums, c, inv, wd, 1e-5, 1, dw, db, coef)
    _bn("eamm_bn_backward_apply", xd, dyd, mean, coef, N, c, hw, dx)
    torch.cuda.synchronize()
    assert float((y.cpu().double() - yr.detach()).abs().max()) <= 5e-5 * 1.5          # weight <= 1.5 times the unit-weight output's 5e-5
    assert float((rm.cpu().double() - 0.1 * mean64).abs().max()) <= 1e-6
    assert float((rv.cpu().double() - (0.9 + 0.1 * var64 * n / (n - 1))).abs().max()) <= 1e-5
    _packed_sums_are_written(sums, c)
    _packed_sums_are_written(bsums, c)
    got = sums.cpu().double()
    assert float(got[2 * c] + 4096 * got[2 * c + 1]) == n
    assert float((dx.cpu().double() - xr.grad).abs().max()) <= 2e-5 * max(1.0, float(xr.grad.abs().max()))
    assert float((dw.cpu().double() - wr.grad).abs().max()) <= 2e-6 * n ** 0.5 + 1e-5
    assert float((db.cpu().double() - br.grad).abs().max()) <= 2e-6 * n ** 0.5 + 1e-5


_BN_NCHW = ["eamm_bn_local_sums", "eamm_bn_finalize", "eamm_bn_apply", "eamm_bn_backward_sums", "eamm_bn_backward_finalize", "eamm_bn_backward_apply"]
for _s in [(3, 5, 7, 9), (4, 33, 1, 1)]:
    case("bn-nchw_" + "x".join(map(str, _s)), _BN_NCHW, functools.partial(_bn_nchw_case, _s), nan_ok=("sums", "backward sums"))


def _bn_nhwc_case(shape, relu, pool, fused, place):
    """test_gpu_backward.test_fused_nhwc_batchnorm_matches_autograd's construction, float64 autograd reference and 5e-6 bar (mode
    EAMM_BN_SINGLE) on the NHWC entries: ``fused`` takes eamm_bn_nhwc_local_stats / _backward_local, otherwise the separate sums and
    finalize entries.  C must be a multiple of 4, so the NCHW cases' shapes do not apply: (3, 6, 10, 12) has a ragged last block in
    every kernel and pools; (4, 1, 1, 36) is four pixels."""
    B, H, W, Cc = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, Cc, H, W, generator=g) * 2 + 0.5
    wt, bs = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    gout = torch.randn(B, Cc, H // 2 if pool else H, W // 2 if pool else W, generator=g)
    xr, wr, br = x.double().requires_grad_(), wt.double().requires_grad_(), bs.double().requires_grad_()
    rm64, rv64 = torch.zeros(Cc, dtype=torch.float64), torch.ones(Cc, dtype=torch.float64)
    yr = F.batch_norm(xr, rm64, rv64, wr, br, True, 0.1, 1e-5)
    yr = F.relu(yr) if relu else yr
    yr = F.avg_pool2d(yr, 2) if pool else yr
    yr.backward(gout.double())

    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    M = B * H * W
    xd, gd, wd, bd = place(nhwc(x), "in", name="x"), place(nhwc(gout), "in", name="grad_out"), place(wt, "in", name="weight"), place(bs, "in", name="bias")
    rm, rv = place(torch.zeros(Cc), "inout", name="running_mean"), place(torch.ones(Cc), "inout", name="running_var")
    sums, bsums = place(6 * Cc + 2, "out", name="sums"), place(6 * Cc + 2, "out", name="backward sums")
    mean, scale, inv = place(Cc, "out", name="mean"), place(Cc, "out", name="scale"), place(Cc, "out", name="inv_std")
    y, dx = place(tuple(nhwc(gout).shape), "out", name="y"), place((B, H, W, Cc), "out", name="dx")
    dw, db, coef = place(Cc, "out", name="dweight"), place(Cc, "out", name="dbias"), place(3 * Cc, "out", name="coef")
    q = int(_lib.lib().eamm_bn_nhwc_workspace_floats(M, Cc))
    fw, bw = place(q, "work", name="forward workspace"), place(q, "work", name="backward workspace")
    if fused:
        _bn("eamm_bn_nhwc_local_stats", xd, M, Cc, 1e-5, 0.1, 1, wd, rm, rv, sums, mean, scale, inv, fw)
    else:
        _bn("eamm_bn_nhwc_local_sums", xd, M, Cc, sums, fw)
        _bn("eamm_bn_finalize", sums, Cc, 1e-5, 0.1, 1, wd, rm, rv, mean, scale, inv)
    _bn("eamm_bn_nhwc_apply", xd, mean, scale, bd, B, H, W, Cc, int(relu), int(pool), y)
    if fused:
        _bn("eamm_bn_nhwc_backward_local", xd, gd, mean, scale, bd, B, H, W, Cc, int(relu), int(pool), inv, wd, 1e-5, 1, bsums, dw, db, coef, bw)
    else:
        _bn("eamm_bn_nhwc_backward_sums", xd, gd, mean, scale, bd, B, H, W, Cc, int(relu), int(pool), bsums, bw)
        _bn("eamm_bn_backward_finalize", bsums, bsums, Cc, inv, wd, 1e-5, 1, dw, db, coef)
    _bn("eamm_bn_nhwc_backward_apply", xd, gd, mean, scale, bd, coef, B, H, W, Cc, int(relu), int(pool), dx)
    torch.cuda.synchronize()
    _packed_sums_are_written(sums, Cc)
    _packed_sums_are_written(bsums, Cc)
    errs = {"y": _rel(y.permute(0, 3, 1, 2), yr.detach()), "dx": _rel(dx.permute(0, 3, 1, 2), xr.grad), "dw": _rel(dw, wr.grad), "db": _rel(db, br.grad),
            "rm": _rel(rm, rm64), "rv": _rel(rv, rv64)}
    assert all(v <= 5e-6 for v in errs.values()), errs


for _s, _r, _p in [((3, 6, 10, 12), True, True), ((4, 1, 1, 36), False, False)]:
    _id = "x".join(map(str, _s))
    case(f"bn-nhwc_{_id}_fused", ["eamm_bn_nhwc_local_stats", "eamm_bn_nhwc_apply", "eamm_bn_nhwc_backward_local", "eamm_bn_nhwc_backward_apply"],
         functools.partial(_bn_nhwc_case, _s, _r, _p, True), nan_ok=("sums", "backward sums"))
    case(f"bn-nhwc_{_id}_separate", ["eamm_bn_nhwc_local_sums", "eamm_bn_finalize", "eamm_bn_nhwc_apply", "eamm_bn_nhwc_backward_sums",
                                     "eamm_bn_backward_finalize", "eamm_bn_nhwc_backward_apply"], functools.partial(_bn_nhwc_case, _s, _r, _p, False),
         nan_ok=("sums", "backward sums"))


# ---- the engine-only operand modes: test_gpu_conv_modes.py's problems, float64 references and bounds ---------------------------------------
import test_gpu_conv_modes as modes


def _transform_case(tile, B, H, W, Cc, pre, place):
    x, s_, t_ = modes.transform_problem(tile, B, H, W, Cc)
    got = modes.run_transform(x, s_ if pre else None, t_ if pre else None, tile, place=place)
    a64 = torch.relu(x.double() * s_.double() + t_.double()) if pre else x.double()
    modes.check_transform(f"guarded F({tile}x{tile}) {(B, H, W, Cc)}", got, a64, tile)


for _a in [(4, 2, 8, 12, 36, True), (4, 1, 4, 4, 4, False), (2, 2, 6, 10, 64, True), (2, 1, 2, 2, 4, False)]:
    case("modes-wino_transform_F%d_%d_%d_%d_%d_pre%d" % _a, ["eamm_op_wino_transform"], functools.partial(_transform_case, *_a))


def _conv_ex_pre_case(name, place):
    c = dict(modes.PRE_CASES[name])
    tile, act, pool = c.pop("tile"), c.pop("act", 0), c.pop("pool", 0)
    x0, _, w, b, res = modes.conv_problem(100 + list(modes.PRE_CASES).index(name), **c)
    pre = modes.affine(c["C0"], torch.Generator().manual_seed(tile))
    out, _ = modes.run_conv(x0, None, w, b, res, act=act, pool=pool, tile=tile, pre=pre, place=place)
    modes.check_conv(name, out, modes.conv_ref(x0, None, w, b, res, act=act, pool=pool, pre=pre), 6e-5)


def _conv_ex_out2_case(name, place):
    c = dict(modes.OUT2_CASES[name])
    tile, splitk, up = c.pop("tile"), c.pop("splitk", 0), c.get("up", 0)
    x0, x1, w, b, res = modes.conv_problem(200 + list(modes.OUT2_CASES).index(name), **c)
    s2, t2 = modes.affine(c["Cout"], torch.Generator().manual_seed(300 + tile))
    out, out2 = modes.run_conv(x0, x1, w, b, res, up=up, splitk=splitk, tile=tile, second=(s2, t2), place=place)
    modes.check_conv(name, out, modes.conv_ref(x0, x1, w, b, res, up=up), 2e-5)
    assert torch.isfinite(out2).all()
    ok, ratio = modes.second_bound_ok(out2, out, s2, t2)
    assert ok, (name, ratio)


def _conv_ex_nchw_case(name, place):
    c = dict(modes.NCHW_CASES[name])
    tile, splitk, act, up = c.pop("tile"), c.pop("splitk", 0), c.pop("act", 0), c.get("up", 0)
    x0, x1, w, b, res = modes.conv_problem(400 + list(modes.NCHW_CASES).index(name), **c)
    planes, _ = modes.run_conv(x0, x1, w, b, res, up=up, act=act, splitk=splitk, tile=tile, want_nchw=1, place=place)
    modes.check_conv(name, modes.nhwc(planes), modes.conv_ref(x0, x1, w, b, res, up=up, act=act), 2e-5)


def _conv_ex_split_case(tile, Cout, place):
    """The floats of a thin pixel past Cout - 32 keep their sentinel (test_split_hand_over): out2 may hold NaN there, and only there."""
    x0, x1, w, b, res = modes.conv_problem(500 + Cout + tile, B=2, H=4, W=6, C0=64, Cout=Cout, up=1)
    wide, thin = modes.run_conv(x0, x1, w, b, res, up=1, tile=tile, split_n=32, place=place)
    want = modes.conv_ref(x0, x1, w, b, res, up=1)
    modes.check_conv("wide", wide, want[:, :32], 2e-5)
    modes.check_conv("thin", thin[..., :Cout - 32], want[:, 32:], 2e-5)
    assert bool(torch.isnan(thin[..., Cout - 32:]).all())


def _conv_ex_dense_case(name, place):
    c = dict(modes.DENSE_CASES[name])
    act, splitk = c.pop("act", 0), c.pop("splitk", 0)
    x0, x1, w, b, res = modes.conv_problem(600 + list(modes.DENSE_CASES).index(name), ks=1, **c)
    out, _ = modes.run_conv(x0, x1, w, b, res, act=act, splitk=splitk, tile=0, place=place)
    modes.check_conv(name, out, modes.conv_ref(x0, x1, w, b, res, act=act), 2e-5)


for _n in ("2153_resid", "2156_pool", "2000_tails_resid"):
    case("modes-conv_ex_pre_" + _n, ["eamm_op_conv_ex"], functools.partial(_conv_ex_pre_case, _n))
for _n in ("tile0_odd_ntail", "tile0_splitk3", "tile0_up", "1001_tails_resid", "1004_skinny", "1002_scalar"):
    case("modes-conv_ex_out2_" + _n, ["eamm_op_conv_ex"], functools.partial(_conv_ex_out2_case, _n))
for _n in ("7x7_sigmoid", "3x3_up", "splitk2"):
    case("modes-conv_ex_nchw_" + _n, ["eamm_op_conv_ex"], functools.partial(_conv_ex_nchw_case, _n))
for _t, _c in [(0, 35), (0, 36), (1003, 36)]:
    case(f"modes-conv_ex_split_tile{_t}_Cout{_c}", ["eamm_op_conv_ex"], functools.partial(_conv_ex_split_case, _t, _c), nan_ok=("out2",))
for _n in ("one_row", "xp0_two_in", "pointwise"):
    case("modes-conv_ex_1x1_" + _n, ["eamm_op_conv_ex"], functools.partial(_conv_ex_dense_case, _n))


def _warp_ex_case(name, place):
    k = dict(modes.WARP_CASES[name])
    n, ns, hf, wf, Cc, h, w = (k[q] for q in ("n", "ns", "hf", "wf", "C", "h", "w"))
    g = torch.Generator().manual_seed(k.get("seed", 0))
    feat = torch.randn(ns, Cc, hf, wf, generator=g)
    ident = torch.stack(torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")[::-1], -1)
    defo = ident[None] + 0.3 * torch.randn(n, h, w, 2, generator=g)
    om = torch.rand(n, 1, h, w, generator=g)
    d, o = defo, om
    if (h, w) != (hf, wf):
        d = F.interpolate(defo.permute(0, 3, 1, 2), size=(hf, wf), mode="bilinear").permute(0, 2, 3, 1)
        o = F.interpolate(om, size=(hf, wf), mode="bilinear")
    want = F.grid_sample(feat if ns == n else feat.expand(n, -1, -1, -1), d, mode="bilinear", padding_mode="zeros", align_corners=False) * o
    s2, t2 = modes.affine(Cc, g)
    out, out2 = modes.run_warp(feat, defo, om, n, ns, hf, wf, Cc, h, w, second=(s2, t2), place=place)
    assert torch.isfinite(out).all() and torch.isfinite(out2).all()
    assert float((modes.nchw(out) - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
    ok, ratio = modes.second_bound_ok(out2, out, s2, t2)
    assert ok, (name, ratio)


for _n in ("C8", "C24", "resized_flow"):
    case("modes-warp_ex_" + _n, ["eamm_op_warp_ex"], functools.partial(_warp_ex_case, _n))


# ---- the clip-level kernels: key-point filter, MFCC, the emotion video's preprocessing -----------------------------------------------------
import os

from conftest import GOLDEN


def _one_euro_case(which, with_state, place):
    """tests/test_gpu_pipeline.py: the reference filter's own outputs (fixture one_euro.npz), bit for bit."""
    z = np.load(os.path.join(GOLDEN, "one_euro.npz"))
    kw = {"kp": (0.05, 8.0, 1.0, 100.0, 10.0), "emo": (1.0, 0.2, 1.0, 100.0, 100.0)}[which]
    for k in ("value", "jacobian"):
        x = torch.from_numpy(z[k])
        T_, E = x.shape[0], x[0].numel()
        xd, out = place(x.reshape(T_, E), "in", name="x " + k), place((T_, E), "out", name="out " + k)
        state = place(torch.zeros(3, E), "inout", name="state " + k) if with_state else None
        _call("eamm_op_one_euro", xd, T_, E, *kw, out, state, 0)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().reshape(x.shape), torch.from_numpy(z[f"{which}_{k}"])), (which, k)


case("clip-one_euro_kp", ["eamm_op_one_euro"], functools.partial(_one_euro_case, "kp", False))
case("clip-one_euro_emo_with_state", ["eamm_op_one_euro"], functools.partial(_one_euro_case, "emo", True))


def _mfcc_case(S, pad, n_clips, place):
    """tests/test_gpu_audio_input.py's signals, float64 oracle and 2e-4 bar.  A workgroup takes a block of frames; 721 samples give 3
    (pad 0) or 28 (pad 1920) frames, 5000 samples 30: last blocks that are partial."""
    import test_gpu_audio_input as ain
    from eamm_amd import mfcc_reference
    xs = np.stack([ain.sig(name, S, i) for i, name in zip(range(n_clips), ("voiced_with_gaps", "click", "lowpassed_noise"))])
    Fr = int(_lib.lib().eamm_op_mfcc_frames(S, pad))
    xd, out = place(torch.from_numpy(xs), "in", name="pcm"), place((n_clips, Fr, 13), "out", name="mfcc")
    _call("eamm_op_mfcc", xd, S, n_clips, S, pad, out)
    torch.cuda.synchronize()
    for i in range(n_clips):
        ref = mfcc_reference(xs[i], pad)
        assert ref.shape == (Fr, 13) and float(np.abs(out[i].cpu().numpy() - ref).max()) <= ain.TOL, (S, pad, i)


for _a in [(721, 0, 1), (721, 1920, 1), (5000, 1920, 3)]:
    case("clip-mfcc_S%d_pad%d_clips%d" % _a, ["eamm_op_mfcc"], functools.partial(_mfcc_case, *_a))


def _video_prep_case(shape, place):
    """tests/test_gpu_video_input.py's frames, landmarks, numpy oracle and bars: resize then alignment, through the two C entries."""
    import test_gpu_video_input as vid
    from eamm_amd import video_input as vi
    n = 2
    f = vid.smooth_frames(n, *shape, seed=shape[0])
    H, W, Ch = shape
    wy, wx = vi.gaussian_taps(H), vi.gaussian_taps(W)
    ty, tx = (C.c_double * len(wy))(*wy), (C.c_double * len(wx))(*wx)
    fd, r = place(torch.from_numpy(f), "in", name="frames"), place((n, 256, 256, 3), "out", dtype=torch.uint8, name="resized")
    _call("eamm_op_resize_aa", fd, n, H, W, Ch, ty, len(wy) // 2, tx, len(wx) // 2, r)
    lm = vid.face_landmarks(n)
    maps = place(torch.from_numpy(np.ascontiguousarray(vi.alignment_maps(lm, None).reshape(n, 6), dtype=np.float64)), "in", name="maps")
    aligned = place((n, 256, 256, 3), "out", name="aligned")
    _call("eamm_op_similarity_warp", r, n, 256, 256, 3, maps, 0, aligned)
    torch.cuda.synchronize()
    want = vi.resize_reference(f)
    vid.assert_levels(r.cpu().numpy() / 255.0, want / 255.0, ("resize", shape))
    np.testing.assert_array_max_ulp(aligned.cpu().numpy(), vi.align_reference(f, lm, None), maxulp=1)


case("clip-resize_and_align_180x320x3", ["eamm_op_resize_aa", "eamm_op_similarity_warp"], functools.partial(_video_prep_case, (180, 320, 3)))
case("clip-resize_and_align_300x200x4", ["eamm_op_resize_aa", "eamm_op_similarity_warp"], functools.partial(_video_prep_case, (300, 200, 4)))


def _augment_case(angle, flip, p, e, host_noise, place):
    """test_augmentation_against_the_oracle with two source frames and three output frames (the third wraps to source frame 0)."""
    import test_gpu_video_input as vid
    from eamm_amd import EmotionVideo, video_input as vi
    n, T_ = 2, 3
    f, lm = vid.smooth_frames(n, 256, 256, seed=3), vid.face_landmarks(n, seed=4)
    noise = np.random.RandomState(5).rand(n, 60, 100, 3).astype(np.float32) if host_noise else None
    ev = EmotionVideo(f, lm, draw=vid._draw(n, angle, flip, p, e, noise))       # draws and aligns on plain tensors; the launch below is the guarded one
    aligned, hinv = place(ev.aligned, "in", name="aligned"), place(ev._hinv, "in", name="inverse homographies")
    nz = place(ev._noise, "in", name="noise") if host_noise else None
    out = place((T_, 3, 256, 256), "out", name="frames")
    x0, y0, w, h = ev.params["mouth"]
    _call("eamm_op_emotion_augment", aligned, n, 0, T_, int(ev.draw["flip"]), ev._rot, hinv, nz, ev.draw.get("noise_seed", 0), x0, y0, w, h, out)
    torch.cuda.synchronize()
    vid.assert_levels(out.cpu().numpy(), vi.emotion_video_reference(f, lm, draw=ev.draw, T=T_), (angle, flip))


case("clip-emotion_augment_identity", ["eamm_op_emotion_augment"], functools.partial(_augment_case, 0.0, False, [20], [20], False))
case("clip-emotion_augment_rotated_host_noise", ["eamm_op_emotion_augment"], functools.partial(_augment_case, 30.0, True, [-29], [39], True))


# ---- proof that the harness sees the GPU: both accesses land in guard memory the arena owns --------------------------------------------
def test_a_store_four_floats_past_an_output_is_reported():
    """eamm_op_l1_pair_backward (out[i] = g[i] * grad_value for i < n, element-wise) told n elements on an `out` view placed for n - 4:
    the last float4 store's fourth lane and the three tail elements land on the first four guard words behind the view.  check() must
    name the operand, the trailing side and offsets 0..3, and nothing else.  (eamm_op_audio_scale would not do: it scales in place,
    and a scaled guard NaN keeps its bits.)"""
    n = 1155
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    for skew in (0, 16):
        arena = Arena(DEV, skew=skew)
        gd, gv = arena.place(g, "in", name="g"), arena.place(torch.tensor([3.0]), "in", name="grad_value")
        out = arena.place(n - 4, "out", name="out")
        _call("eamm_op_l1_pair_backward", gd, n, gv, out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), g[:n - 4] * 3.0)
        damage = arena.damage()
        assert [(d["name"], d["side"], d["first"], d["last"], d["count"]) for d in damage] == [("out", "after", 0, 3, 4)], damage
        with pytest.raises(AssertionError, match=r"guard after operand 'out' damaged: 4 words, offsets 0\.\.3"):
            arena.check()


def test_a_load_four_floats_past_an_input_poisons_the_result():
    """eamm_op_l1_pair (mean |a - b| of n elements) on an `a` placed four floats short: the last four differences read guard NaNs."""
    n = 1155
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    for skew in (0, 16):
        for short in (0, 4):
            arena = Arena(DEV, skew=skew)
            ad, bd = arena.place(a[:n - short], "in", name="a"), arena.place(b, "in", name="b")
            loss, grad = arena.place(1, "out", name="loss"), arena.place(n, "out", name="gradient")
            ws = arena.place(int(_lib.lib().eamm_op_l1_pair_workspace_floats(n)), "work")
            _call("eamm_op_l1_pair", ad, bd, n, 1.0, loss, grad, work=ws)
            torch.cuda.synchronize()
            assert not arena.damage() and not arena.changed_inputs()
            assert bool(torch.isnan(loss).any()) == (short == 4), (skew, short, loss)
            assert ("loss" in arena.nan_outputs()) == (short == 4)


def test_an_address_four_bytes_off_is_refused_before_any_launch():
    """eamm_op_l1_pair and its backward document 16-byte alignment and check it (op_aligned16) in front of all device work
    (eamm_op_perceptual.hip: the refusals precede the launch): an address 4 bytes into an arena view comes back as EAMM_ERR_ARG and
    nothing was written -- the outputs are still guard words."""
    n = 1155
    arena = Arena(DEV, skew=16)
    a, b = arena.place(torch.zeros(n + 1), "in", name="a"), arena.place(torch.zeros(n + 1), "in", name="b")
    value, grad, out = arena.place(1, "out", name="value"), arena.place(n + 1, "out", name="gradient"), arena.place(n + 1, "out", name="out")
    ws = arena.place(int(_lib.lib().eamm_op_l1_pair_workspace_floats(n)), "work")
    off = lambda t: C.c_void_p(t.data_ptr() + 4)
    for args in ((off(a), b, n, 1.0, value, grad), (a, off(b), n, 1.0, value, grad), (a, b, n, 1.0, value, off(grad))):
        with pytest.raises(_lib.EammError) as exc:
            _call("eamm_op_l1_pair", *args, work=ws)
        assert exc.value.code == _lib.ERR_ARG
    for args in ((off(a), n, value, out), (a, n, value, off(out))):
        with pytest.raises(_lib.EammError) as exc:
            _call("eamm_op_l1_pair_backward", *args)
        assert exc.value.code == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert not arena.damage() and not arena.changed_inputs()
    assert all(bool((t.view(torch.int32) == 0x7FC5A5A5).all()) for t in (value, grad, out, ws))


# ---- the handle families, boundary tensors only ---------------------------------------------------------------------------------------------
# A handle's internal buffers are its own allocations and out of an arena's reach: these tests put the tensors that cross the C boundary
# -- the inputs, and the outputs where the call takes the caller's pointers -- in views 16 bytes off a 256-byte boundary, and ask for
# the bits of the same call on plain tensors and for an intact arena.
from eamm_amd._handle import ptr as _p, stream_ptr as _stream


def _boundary(run):
    """``run(place)`` -> dict of outputs; plain, then at skew 16: equal bits, check() passes."""
    want = run(Plain(DEV))
    torch.cuda.synchronize()
    arena = Arena(DEV, skew=16)
    got = run(arena)
    torch.cuda.synchronize()
    arena.check()
    assert sorted(got) == sorted(want)
    for k in want:
        assert bool(torch.isfinite(want[k].float()).all()) and torch.equal(got[k], want[k]), k


def test_engine_encode_source_and_forward_frames_on_skewed_boundary_tensors():
    """Engine at tiny_config() 64 x 64, three frames: eamm_encode_source's image and eamm_forward_frames' key points in "in" views, its
    six float outputs and the uint8 frames in "out" views (the call as Engine.forward_frames makes it)."""
    from eamm_amd import tiny_config
    from eamm_amd.engine import Engine
    from eamm_amd.weights import synthetic_keypoints, synthetic_source, synthetic_state_dict
    cfg = tiny_config()
    eng = Engine(cfg, 64, 64, 4, 1, torch.device(DEV))
    eng.load_state_dict(synthetic_state_dict(cfg, seed=3))
    n, K, ch, h, w = 3, eng.num_kp, eng.num_channels, eng.h, eng.w
    src = synthetic_source(64, seed=1)
    kd, ks = synthetic_keypoints(n, K, seed=4), synthetic_keypoints(1, K, seed=6)
    shapes = {"prediction": (n, ch, 64, 64), "mask": (n, K + 1, h, w), "sparse_deformed": (n, K + 1, ch, h, w), "occlusion_map": (n, 1, h, w),
              "deformed": (n, ch, 64, 64), "deformation": (n, h, w, 2)}

    def run(place):
        eng.encode_source(place(src, "in", name="source"))
        t = {a + "." + b: place(v, "in", name=a + "." + b) for a, d in (("kd", kd), ("ks", ks)) for b, v in d.items()}
        res = {k: place(sh, "out", name=k) for k, sh in shapes.items()}
        res["frames_u8"] = place((n, 64, 64, 3), "out", dtype=torch.uint8, name="frames_u8")
        o = _lib.EammOutputs(**{k: v.data_ptr() for k, v in res.items()})
        _lib.check(eng._L.eamm_forward_frames(eng._ctx, n, _p(t["kd.value"]), _p(t["kd.jacobian"]), _p(t["ks.value"]), _p(t["ks.jacobian"]),
                                              C.byref(o), _stream(eng.device)), eng._ctx)
        eng.check_numeric()
        return res

    _boundary(run)
    plain = eng.forward_frames({a: b.to(DEV) for a, b in kd.items()}, {a: b.to(DEV) for a, b in ks.items()}, outputs=tuple(shapes))
    again = run(Plain(DEV))
    assert all(torch.equal(plain[k], again[k]) for k in plain)            # the call above IS Engine.forward_frames' call


def test_kp_detect_on_skewed_boundary_tensors():
    from eamm_amd import KPDetector, tiny_kp_config
    from eamm_amd.weights import kp_state_dict_spec, synthetic_source, synthetic_state_dict
    cfg = tiny_kp_config()
    det = KPDetector(**cfg)
    det.load_state_dict(synthetic_state_dict(cfg, seed=7, spec=kp_state_dict_spec(cfg)))
    det = det.to(DEV).eval()
    x = synthetic_source(64, seed=2, batch=3)
    first = det(x.to(DEV))                                                    # builds the handle; the shapes of the outputs

    def run(place):
        xd = place(x, "in", name="image")
        out = {k: place(tuple(v.shape), "out", name=k) for k, v in first.items()}
        o = _lib.EammKpOutputs(**{k: v.data_ptr() for k, v in out.items()})
        det._handle.call("detect", _p(xd), 3, C.byref(o), _stream(xd.device))
        return out

    _boundary(run)
    assert all(torch.equal(first[k], v) for k, v in run(Plain(DEV)).items())


def test_emo_detect_on_skewed_boundary_tensors():
    import test_emotion_detector as ted
    from eamm_amd.weights import synthetic_keypoints, synthetic_source
    fx, cfg = ted.load("emotion_tiny128")[:2]
    m = ted.make(cfg, int(fx["weight_seed"])).to(DEV).eval()
    n, size = 2, int(fx["size"])
    x, kp = synthetic_source(size, seed=5, batch=n), synthetic_keypoints(n, 10, seed=8)
    first = m.detect(x.to(DEV), kp["value"].to(DEV), kp["jacobian"].to(DEV))

    def run(place):
        xd, v, j = place(x, "in", name="image"), place(kp["value"], "in", name="value"), place(kp["jacobian"], "in", name="jacobian")
        out = {k: place(tuple(t.shape), "out", name="out " + k) for k, t in first.items()}
        o = _lib.EammEmoOutputs(**{k: t.data_ptr() for k, t in out.items()})
        m._handle.call("detect", _p(xd), _p(v), _p(j), n, C.byref(o), _stream(xd.device))
        return out

    _boundary(run)
    assert all(torch.equal(first[k], v) for k, v in run(Plain(DEV)).items())


def test_deconv_forward_on_skewed_boundary_tensors():
    from eamm_amd import DeconvTail
    tail = DeconvTail(max_batch=8)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for q in tail.parameters():
            q.copy_(torch.randn(q.shape, generator=g) * 0.05)
    tail = tail.to(DEV).eval()
    x = torch.randn(3, tail.channels[0], generator=g)
    first = tail(x.to(DEV))

    def run(place):
        xd, out = place(x, "in", name="x"), place(tuple(first.shape), "out", name="feature map")
        tail._handle.call("forward", _p(xd), 3, _p(out), _stream(xd.device))
        return {"feature map": out}

    _boundary(run)
    assert torch.equal(first, run(Plain(DEV))["feature map"])


def test_audio_lstm_features_on_skewed_boundary_tensors():
    """One clip, five steps: image, audio windows and pose in "in" views, lstm_out in an "out" view."""
    import test_gpu_audio_feature as taf
    from eamm_amd.weights import synthetic_audio_inputs
    m = taf.net()
    image, audio, pose = synthetic_audio_inputs(1, 5, seed=21)
    first = m.lstm_features(image.to(DEV), audio.to(DEV), pose.to(DEV))
    m.check()

    def run(place):
        img, aud, pos = place(image, "in", name="image"), place(audio, "in", name="audio"), place(pose, "in", name="pose")
        out = place(tuple(first.shape), "out", name="lstm_out")
        m._handle.call("lstm_features", _p(img), _p(aud), _p(pos), 1, 5, 1.6, None, None, None, None, None, _p(out), _stream(img.device))
        m.check()
        return {"lstm_out": out}

    _boundary(run)
    assert torch.equal(first, run(Plain(DEV))["lstm_out"])


# ---- every guarded case, of this file and of the other modules that register some ------------------------------------------------------------
import test_gpu_conv_dev_1x1, test_gpu_disc_ops, test_gpu_equivariance_ops  # noqa: E401,F401  (the modules that register cases: this list)


@pytest.mark.parametrize("cid", list(CASES))
def test_guarded(cid):
    run_three(cid, DEV)
