"""The frozen inference path's small kernels one by one, through their operator entries (eamm_op_first7 ... eamm_op_audio_scale,
include/eamm_hip.h), against float64 references on the CPU -- at the shapes where each kernel takes a path the whole-model fixtures
never take.  Every case names the guard, loader branch, template instance or loop remainder it reaches.  Inputs are seeded on the
CPU; every output buffer starts as NaN (0xFF bytes for uint8) and is compared WHOLE, so an element nobody wrote fails the finite
check, and the channels a kernel must not read hold NaN, so a stray read poisons an output.  The tolerances are the ones the
neighbouring kernels' tests use (tests/test_gpu_ops.py, tests/test_gpu_motion_ops.py) or follow from the fp32 operation count."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eamm_amd import _op
from guarded import Plain
from eamm_amd.weights import antialias_kernel, synthetic_keypoints
from test_gpu_motion_ops import _close, _reference_front

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _run(name, *args):
    """One entry on device 0 and the current stream, then a wait.  Tensors are passed as such (never as a bare data_ptr() of a
    temporary): they stay referenced until the launch has finished."""
    _op.call(name[len("eamm_op_"):], torch.device(DEV), *args)
    torch.cuda.synchronize()


def _whole(got, want, bound, what):
    """max |got - want| over the WHOLE buffer, after the finite check that an unwritten (NaN) element fails."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), (what, "unwritten / non-finite elements", int((~torch.isfinite(got)).sum()))
    err = float((got - want.double()).abs().max())
    print(f"{what}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)
    return err


# ---- conv_first7_kernel<NT> (conv_first.hip): NT = Cout / 32 in 1..4, 16 x 16 tiles with a 3-pixel halo ---------------------------
FIRST7 = [(c, 2, 16, 16) for c in (32, 64, 96, 128)]             # NT = 1, 2, 3, 4: every template instance, whole tiles, batch index
for _c in (64, 96):
    FIRST7 += [(_c, 1, 8, 8),       # one partial tile (the y < H && x < W store guard); the halo rows / columns 11..21 wholly outside
               (_c, 3, 20, 36),     # partial last tile in both directions; batch index
               (_c, 1, 16, 52)]     # four tiles in a row: interior halos read the neighbouring tiles' pixels


@pytest.mark.parametrize("cout,ns,H,W", FIRST7)
def test_first7_matches_conv2d(cout, ns, H, W, place=None):
    place = place or Plain(DEV)
    g = torch.Generator().manual_seed(cout + 7 * H + W)
    x = torch.rand(ns, 3, H, W, generator=g)
    w = (torch.randn(cout, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5).contiguous()
    b = (0.1 * torch.randn(cout, generator=g)).contiguous()
    want = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=3)).permute(0, 2, 3, 1)
    xd, out = place(x, "in"), place((ns, H, W, cout), "out")
    _run("eamm_op_first7", xd, ns, H, W, w, b, cout, out)
    # the bound of the direct fp32-MFMA forms in test_gpu_ops.py: K = 147, only the summation order differs
    _whole(out, want, 2e-5 * max(1.0, float(want.abs().max())), f"first7 Cout {cout} [{ns},{H},{W}]")


# ---- the flow head, inference kernels (motion.hip): motion_head_kernel and motion_head_rowsplit_kernel -----------------------------
def _head_reference(logits64, kd, ks, K, has_occ):
    """test_gpu_motion_ops.test_motion_head_against_torch_double's composition (dense_motion.py:98-111) in float64."""
    n, h, w, _ = logits64.shape
    kd64, ks64 = {a: b.double() for a, b in kd.items()}, {a: b.double() for a, b in ks.items()}
    _, _, motions = _reference_front(kd64, ks64, torch.zeros(n, 3, h, w, dtype=torch.float64), 0.01, True)
    mask = F.softmax(logits64[..., :K + 1].permute(0, 3, 1, 2), dim=1)
    defo = (motions.permute(0, 1, 4, 2, 3) * mask[:, :, None]).sum(dim=1).permute(0, 2, 3, 1)
    occ = torch.sigmoid(logits64[..., K + 1]) if has_occ else None
    return mask, defo, occ


def _records(kd, ks):
    from eamm_amd import motion_ops
    with torch.no_grad():
        return motion_ops.kp_records({a: b.to(DEV) for a, b in kd.items()}, {a: b.to(DEV) for a, b in ks.items()})


def _check_head(tag, bufs, want, has_occ, with_outs):
    """bufs = (deformation, occlusion, mask_out, occ_out), all NaN before the launch; 2e-6 as test_gpu_motion_ops.py."""
    defo, occ, mask_out, occ_out = bufs
    mask_ref, def_ref, occ_ref = want
    errs = {"deformation": _close(defo, def_ref, 2e-6, tag + " deformation")}
    assert torch.isfinite(defo).all()
    if has_occ:
        errs["occlusion"] = _close(occ, occ_ref, 2e-6, tag + " occlusion")
        assert torch.isfinite(occ).all()
    else:
        assert torch.isnan(occ).all(), tag + ": occlusion written without has_occ"
    if with_outs:
        errs["mask"] = _close(mask_out, mask_ref, 2e-6, tag + " mask_out")
        assert torch.isfinite(mask_out).all()
        if has_occ:
            _close(occ_out[:, 0], occ_ref, 2e-6, tag + " occ_out")
            assert torch.isfinite(occ_out).all() and torch.equal(occ_out[:, 0], occ)
        else:
            assert torch.isnan(occ_out).all()
    print(tag + ": " + ", ".join(f"{a} {e:.2e}" for a, e in errs.items()) + " of max(1, max|want|) (bound 2e-06)")


def _head_buffers(n, K, h, w, with_outs, place=None):
    place = place or Plain(DEV)
    return (place((n, h, w, 2), "out", name="deformation"), place((n, h, w), "out", name="occlusion"),
            place((n, K + 1, h, w), "out", name="mask_out") if with_outs else None, place((n, 1, h, w), "out", name="occ_out") if with_outs else None)


@pytest.mark.parametrize("n,h,w", [(3, 12, 20), (1, 17, 19), (2, 16, 16)])     # h * w = 240 < 256; 323: a 67-thread tail block; 256
@pytest.mark.parametrize("K", [1, 10, 30])                                     # K = 30: the occlusion logit is lane 31
def test_motion_head_inference_kernel(K, n, h, w, place=None):
    place = place or Plain(DEV)
    g = torch.Generator().manual_seed(100 * K + h)
    kd, ks = synthetic_keypoints(n, K, seed=4), synthetic_keypoints(n, K, seed=6)
    rec = place(_records(kd, ks), "in", name="records")
    for has_occ in (0, 1):
        logits = torch.randn(n, h, w, 32, generator=g)
        logits[..., K + 1 + has_occ:] = NAN                                    # the channels above the used ones must not reach an output
        want = _head_reference(logits.double(), kd, ks, K, has_occ)
        ld = place(logits, "in", name="logits")
        for with_outs in (False, True):                                        # mask_out / occ_out both NULL, both given
            bufs = _head_buffers(n, K, h, w, with_outs, place)
            _run("eamm_op_motion_head_infer", ld, rec, n, K, h, w, has_occ, *bufs)
            _check_head(f"head K {K} occ {has_occ} outs {with_outs} [{n},{h},{w}]", bufs, want, has_occ, with_outs)


# (K, has_occ): NC = 12 -> 7 NC = 84, the 16-byte loader; NC = 11 and NC = 7 -> the scalar loader; NC = 18 -> 7 NC = 126, the widest the
# engine uses (scalar loader, 126 % 4 = 2).  w: narrower than the halo; one partial tile; exactly one 64-pixel tile; a seam with a
# partial second tile; three tiles.
@pytest.mark.parametrize("w", [5, 20, 64, 70, 131])
@pytest.mark.parametrize("K,has_occ", [(10, 1), (10, 0), (5, 1), (16, 1)])
def test_motion_head_rowsplit_kernel(K, has_occ, w, place=None):
    place = place or Plain(DEV)
    n, h, PS = 2, 3, 128
    NC = K + 1 + has_occ
    g = torch.Generator().manual_seed(1000 * K + 10 * w + has_occ)
    kd, ks = synthetic_keypoints(n, K, seed=4), synthetic_keypoints(n, K, seed=6)
    rec = place(_records(kd, ks), "in", name="records")
    part = 0.5 * torch.randn(n, h, w, PS, generator=g)
    part[..., 7 * NC:] = NAN
    bias = torch.randn(NC, generator=g)
    # logit co = bias[co] + sum_dx part[y, x + dx - 3, dx * NC + co], zero outside the row
    taps = F.pad(part[..., :7 * NC].double().reshape(n, h, w, 7, NC), (0, 0, 0, 0, 3, 3))
    logits64 = bias.double() + sum(taps[:, :, dx:dx + w, dx] for dx in range(7))
    want = _head_reference(logits64, kd, ks, K, has_occ)
    bufs = _head_buffers(n, K, h, w, True, place)
    _run("eamm_op_motion_head_rowsplit", place(part, "in", name="part"), PS, NC, place(bias, "in", name="bias"), rec, n, K, h, w, has_occ, *bufs)
    _check_head(f"rowsplit NC {NC} w {w}", bufs, want, has_occ, True)
    # the plain form on the reference logits rounded to fp32 agrees with the row-split form within the same bound
    l32 = torch.full((n, h, w, 32), NAN)
    l32[..., :NC] = logits64.float()
    plain = _head_buffers(n, K, h, w, True, place)
    _run("eamm_op_motion_head_infer", place(l32, "in", name="logits"), rec, n, K, h, w, has_occ, *plain)
    _check_head(f"plain on rowsplit's logits NC {NC} w {w}", plain, want, has_occ, True)
    for a, b, what in zip(bufs, plain, ("deformation", "occlusion", "mask_out", "occ_out")):
        if has_occ or what in ("deformation", "mask_out"):
            _close(a, b.cpu(), 2e-6, f"rowsplit vs plain {what} NC {NC} w {w}")


# ---- final_shift_sum_kernel: 128-pixel row tile, 3-pixel halo each side ------------------------------------------------------------
# W: narrower than the halo; one partial tile; exactly one tile; a seam with a 3-pixel second tile; two seams and a partial last tile
@pytest.mark.parametrize("W", [5, 20, 128, 131, 300])
def test_final_shift_sum(W, place=None):
    place = place or Plain(DEV)
    n, H = 2, 3
    g = torch.Generator().manual_seed(W)
    part = torch.randn(n, H, W, 32, generator=g)
    part[..., 21:] = NAN
    bias = torch.randn(3, generator=g)
    taps = F.pad(part[..., :21].double().reshape(n, H, W, 7, 3), (0, 0, 0, 0, 3, 3))
    want = torch.sigmoid(bias.double() + sum(taps[:, :, dx:dx + W, dx] for dx in range(7))).permute(0, 3, 1, 2)
    out = place((n, 3, H, W), "out")
    _run("eamm_op_final_shift_sum", place(part, "in", name="part"), place(bias, "in", name="bias"), n, H, W, out)
    _whole(out, want, 2e-6, f"final_shift_sum W {W}")              # absolute, as test_fused_final_layer_matches_torch


# ---- to_u8_kernel: rintf(p * 255) clamped -- bit-exact ----------------------------------------------------------------------------
def _u8_reference(p):
    return np.clip(np.rint(p.astype(np.float32) * np.float32(255)), 0, 255).astype(np.uint8)


def _to_u8(pred, place=None):
    place = place or Plain(DEV)
    n, _, H, W = pred.shape
    out = place((n, H, W, 3), "out", dtype=torch.uint8)       # 0xFF bytes
    _run("eamm_op_to_u8", place(torch.from_numpy(pred), "in"), n, H, W, out)
    return out.cpu().numpy()


def test_to_u8_is_bit_exact_at_every_rounding_edge(place=None):
    """Every k / 255 with its two fp32 neighbours, every half-way value (k + 0.5) / 255 with its two neighbours, signed zero,
    values just and far outside [0, 1], both infinities.  The reference is the same IEEE operations the kernel performs (one fp32
    multiply, round-half-even, clamp), so no tolerance applies.  These 1543 values do not fit the 315 elements of a [3,3,5,7]
    tensor: the frame size stays 5 x 7 (an odd plane of 35 pixels) and the batch grows to 15 frames, 1575 elements; seeded uniform
    values fill the rest."""
    k = np.arange(256, dtype=np.float32)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    exact, half = k / np.float32(255), (k + np.float32(0.5)) / np.float32(255)
    special = np.array([-0.0, -1e-3, 1 + 1e-3, 7.0, -7.0, np.inf, -np.inf], dtype=np.float32)
    vals = np.concatenate([exact, np.nextafter(exact, up), np.nextafter(exact, down), half, np.nextafter(half, up),
                           np.nextafter(half, down), special]).astype(np.float32)
    n = 15
    assert vals.size == 1543 <= n * 3 * 5 * 7
    rs = np.random.RandomState(3)
    pred = np.concatenate([vals, rs.uniform(0, 1, n * 105 - vals.size).astype(np.float32)])
    pred = pred[rs.permutation(pred.size)].reshape(n, 3, 5, 7)
    with np.errstate(invalid="ignore"):
        want = _u8_reference(pred).transpose(0, 2, 3, 1)
    got = _to_u8(pred, place)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) == 256


def test_to_u8_sends_nan_to_zero():
    """Pins the kernel's own rule: fmaxf(rintf(NaN), 0) = 0.  numpy's cast of NaN to uint8 is undefined, so the NaN elements are
    asserted apart from the reference; the others still follow it."""
    rs = np.random.RandomState(4)
    pred = rs.uniform(0, 1, (2, 3, 3, 5)).astype(np.float32)
    hole = rs.uniform(0, 1, pred.shape) < 0.3
    pred[hole] = np.nan
    with np.errstate(invalid="ignore"):
        want = _u8_reference(np.where(hole, np.float32(0), pred)).transpose(0, 2, 3, 1)
    got = _to_u8(pred)
    assert hole.any() and (got[hole.transpose(0, 2, 3, 1)] == 0).all()
    assert np.array_equal(got, want)


# ---- warp_image_kernel: grid-stride, grid capped at 16384 blocks -----------------------------------------------------------------
def _warp_image_case(n, ns, H, W, h, w, src_planes, channels, seed, place=None):
    place = place or Plain(DEV)
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(ns, src_planes, H, W, generator=g)
    ident = torch.stack(torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")[::-1], -1)
    defo = (ident[None] + 0.3 * torch.randn(n, h, w, 2, generator=g)).contiguous()     # some samples fall outside the image
    d = defo.double()
    if (h, w) != (H, W):
        d = F.interpolate(d.permute(0, 3, 1, 2), size=(H, W), mode="bilinear").permute(0, 2, 3, 1)
    s64 = src[:, :channels].double()
    want = F.grid_sample(s64 if ns == n else s64.expand(n, -1, -1, -1), d, mode="bilinear", padding_mode="zeros", align_corners=False)
    out = place((n, channels, H, W), "out")
    _run("eamm_op_warp_image", place(src, "in", name="source"), place(defo, "in", name="deformation"), n, ns, H, W, h, w, src_planes, channels, out)
    # as test_warp_features_matches_grid_sample
    _whole(out, want, 2e-5 * max(1.0, float(want.abs().max())), f"warp_image [{n},{ns},{H},{W}] flow {h}x{w} planes {src_planes}/{channels}")


@pytest.mark.parametrize("n,ns,H,W,h,w,src_planes,channels", [
    (3, 1, 16, 16, 16, 16, 3, 3),        # the direct flow read, one cached source
    (2, 2, 24, 40, 6, 10, 3, 3),         # the flow resized 4 x, a source per frame
    (2, 1, 16, 16, 4, 4, 6, 4),          # the first four of six planes
])
def test_warp_image_matches_grid_sample(n, ns, H, W, h, w, src_planes, channels):
    _warp_image_case(n, ns, H, W, h, w, src_planes, channels, seed=H + w)


def test_warp_image_grid_stride_remainder():
    """15430 * 16 * 17 = 4196960 pixels: 16384 blocks of 256 threads cover 4194304 of them, the stride loop's second trip the last
    2656 -- neither a multiple of 256 nor of the grid.  A source per frame, 16.8 MB.

    The pixel count comes from the frame count, not from the map's side, because the bound is the small maps' 2e-5: what grows with
    the side is not the kernel's arithmetic but the fp32 sampling coordinate ((g + 1) W - 1) / 2, whose rounding of a few 2^-24 W
    pixels is multiplied by the image's slope -- and at the zero-padded border that slope is the pixel value itself.  Two first
    versions of this case showed that and nothing else: 2 frames of 2101 x 1001 noise were 5.8e-3 from the float64 reference, 66
    smooth frames of 254 x 254 were 5.3e-4 (at a sample 0.03 pixels inside the bottom border), and torch's own fp32 grid_sample
    is the same 5.8e-3 and 5.3e-4 from float64 on those inputs; on this one it is 1.1e-5."""
    _warp_image_case(15430, 15430, 16, 17, 8, 8, 1, 1, seed=11)


# ---- source_to_nhwc_kernel + the once-per-clip anti-alias launch (source_prepare_launch) -------------------------------------------
def _source_prepare_case(ns, H, W, inv, seed, place=None):
    place = place or Plain(DEV)
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(ns, 3, H, W, generator=g)
    aa = antialias_kernel(3)
    h, w = H // inv, W // inv
    sd, ad = place(src, "in", name="source"), place(aa, "in", name="aa_kernel")
    nhwc, small, small_op = place((ns, H, W, 32), "out", name="nhwc"), place((ns, h, w, 4), "out", name="small"), place((ns, h, w, 4), "out", name="small_op")
    _run("eamm_op_source_prepare", sd, ad, ns, H, W, inv, 32, nhwc, small)
    _run("eamm_op_antialias_down", sd, ad, ns, H, W, inv, small_op)
    assert torch.equal(nhwc.cpu(), F.pad(src.permute(0, 2, 3, 1), (0, 29))), "the NHWC copy is not pad(permute(source))"
    assert torch.isfinite(small).all() and torch.equal(small, small_op), "the small copy differs from eamm_op_antialias_down's"
    ref = src.double()
    if inv != 1:    # util.py:1044-1052, as test_antialias_down_forward_and_backward
        ref = F.conv2d(F.pad(ref, (6, 6, 6, 6)), aa.double(), groups=3)[:, :, ::inv, ::inv]
    assert float(small[..., 3].abs().max()) == 0.0
    err = _close(small[..., :3].permute(0, 3, 1, 2), ref, 2e-6, "source_prepare small copy")
    print(f"source_prepare [{ns},{H},{W}] / {inv}: small copy max error {err:.3e} (bound 2e-06)")


@pytest.mark.parametrize("ns,H,W,inv", [(2, 32, 48, 4), (1, 8, 8, 1), (3, 20, 12, 2)])
def test_source_prepare(ns, H, W, inv):
    _source_prepare_case(ns, H, W, inv, seed=H)


def test_source_prepare_grid_stride_remainder():
    """724 * 732 pixels of eight float4 each = 4239744 elements of the NHWC copy: 45440 past the 16384-block grid, neither a multiple of
    256 nor of the grid.  A 6.4 MB source, a 68 MB copy."""
    _source_prepare_case(1, 724, 732, 4, seed=5)


# ---- broadcast_features_kernel.  Its grid is capped at 65536 blocks of 256 float4: a remainder case would need 268 MB, left out. ----
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("with_out2", [True, False])
def test_broadcast_features(ns, with_out2, place=None):
    place = place or Plain(DEV)
    n, hf, wf, C = 3, 4, 6, 32
    g = torch.Generator().manual_seed(ns)
    feat = torch.randn(ns, hf, wf, C, generator=g)
    s, t = torch.randn(C, generator=g), torch.randn(C, generator=g)
    out, out2 = place((n, hf, wf, C), "out", name="out"), place((n, hf, wf, C), "out", name="out2") if with_out2 else None
    _run("eamm_op_broadcast_features", place(feat, "in", name="features"), n, ns, hf, wf, C, out, out2, place(s, "in", name="scale"), place(t, "in", name="shift"))
    want = feat if ns == n else feat.expand(n, -1, -1, -1)
    assert torch.equal(out.cpu(), want), "out is not the source frame"
    if with_out2:
        # one fused multiply-add rounds once: at most one fp32 ulp from the float64 value rounded once
        w32 = F.relu(want.double() * s.double() + t.double()).float().numpy()
        got = out2.cpu().numpy()
        assert np.isfinite(got).all()
        ulps = np.abs(got.astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.maximum(np.abs(w32), np.float32(1e-30)))
        print(f"broadcast_features out2: max {ulps.max():.2f} ulp (bound 1)")
        assert ulps.max() <= 1.0 and (got[w32 == 0] == 0).all()


# ---- nchw_to_nhwc_pad_kernel with its `planes` argument: bit-exact -------------------------------------------------------------------
def _pad_case(B, C, planes, H, W, Cpad, seed, place=None):
    place = place or Plain(DEV)
    src = torch.randn(B, planes, H, W, generator=torch.Generator().manual_seed(seed))
    dst = place((B, H, W, Cpad), "out")
    _run("eamm_op_nchw_to_nhwc_pad", place(src, "in"), B, C, planes, H, W, Cpad, dst)
    assert torch.equal(dst.cpu(), F.pad(src[:, :C].permute(0, 2, 3, 1), (0, Cpad - C)))


# every plane, zero-padded; the first 32 of 35 planes, no padding; RGB
@pytest.mark.parametrize("C,planes,Cpad", [(35, 35, 64), (32, 35, 32), (3, 3, 32)])
def test_nchw_to_nhwc_pad(C, planes, Cpad):
    _pad_case(2, C, planes, 5, 7, Cpad, seed=C)


def test_nchw_to_nhwc_pad_grid_stride_remainder():
    """33 * 63 * 65 * 32 = 4324320 elements: 130016 past the 16384-block grid, neither a multiple of 256 nor of the grid (64 x 64 maps
    would make it a multiple of 256).  A 15.7 MB source."""
    _pad_case(33, 29, 29, 63, 65, 32, seed=2)


# ---- the emotion detector's tail (emotion.hip) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,C", [(1, 1, 64), (9, 16, 512), (3, 49, 96)])      # 64 threads of one block; 18 whole blocks; 288 = a 32-thread tail
def test_emo_avgpool(B, P, C, place=None):
    place = place or Plain(DEV)
    x = torch.randn(B, P, C, generator=torch.Generator().manual_seed(P))
    out = place((B, C), "out")
    _run("eamm_op_emo_avgpool", place(x, "in"), B, P, C, out)
    # a serial fp32 sum of P terms
    _whole(out, x.double().mean(dim=1), P * 2.0 ** -24 * float(x.abs().max()), f"emo_avgpool [{B},{P},{C}]")


@pytest.mark.parametrize("B", [1, 9])      # 1260 and 11340 outputs: a 236- and a 76-thread tail block
def test_emo_embed(B, place=None):
    place = place or Plain(DEV)
    rs = np.random.RandomState(B)
    six = rs.uniform(-2, 2, (B, 10, 6)).astype(np.float32)
    six[0, 0, :3] = (0.0, 2.0, -2.0)
    six[-1, 9, 3:] = (-2.0, 0.0, 2.0)
    parts = [six.astype(np.float64)]
    for f in range(10):
        a = six * np.float32(2 ** f)                       # exact in fp32
        assert a.dtype == np.float32
        parts += [np.sin(a.astype(np.float64)), np.cos(a.astype(np.float64))]
    want = np.stack(parts, axis=2).reshape(B, 1260)        # [B,10,21,6]: d, then (sin, cos) per frequency, each over the six numbers
    value = torch.from_numpy(np.ascontiguousarray(six[..., :2]))
    jac = torch.from_numpy(np.ascontiguousarray(six[..., 2:]))
    out = place((B, 1260), "out")
    _run("eamm_op_emo_embed", place(value, "in", name="value"), place(jac, "in", name="jacobian"), B, out)
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    worst = np.unravel_index(err.argmax(), err.shape)
    print(f"emo_embed B {B}: max error {err.max():.3e} (bound {4 * 2.0 ** -24:.3e}) at output {worst}")
    # outputs are at most 2 in magnitude; the accurate sinf / cosf are good to a few ulp up to the largest argument, 1024 rad
    bad = np.argwhere(err > 4 * 2.0 ** -24)
    args = [(int(b), int(j), float(six[b, j // 126, j % 6] * 2.0 ** max(0, (j % 126 // 6 - 1) // 2))) for b, j in bad[:8]]
    assert not len(bad), ("(frame, output, argument) of the first misses", args)


# x1 NULL, one block, nb = 1; fcp0 / fa0-like widths with an nb = 1 tail workgroup and a 44-thread tail block; one whole workgroup,
# odd K and O = 257 = one thread in the second block; two whole workgroups and an nb = 1 tail
@pytest.mark.parametrize("B,K0,K1,O,relu", [(1, 64, 0, 64, 0), (9, 1260, 512, 300, 1), (8, 33, 7, 257, 1), (17, 128, 64, 256, 0)])
def test_emo_linear(B, K0, K1, O, relu, place=None):
    place = place or Plain(DEV)
    g = torch.Generator().manual_seed(K0 + O)
    x0 = torch.randn(B, K0, generator=g)
    x1 = torch.randn(B, K1, generator=g) if K1 else None
    wt = torch.randn(K0 + K1, O, generator=g) / (K0 + K1) ** 0.5
    bias = torch.randn(O, generator=g)
    x = x0.double() if x1 is None else torch.cat([x0, x1], dim=1).double()
    want = x @ wt.double() + bias.double()
    if relu:
        want = F.relu(want)
    out = place((B, O), "out")
    _run("eamm_op_emo_linear", place(x0, "in", name="x0"), K0, None if x1 is None else place(x1, "in", name="x1"), K1, place(wt, "in", name="wt"),
         place(bias, "in", name="bias"), O, B, relu, out)
    _whole(out, want, 2e-5 * max(1.0, float(want.abs().max())), f"emo_linear [{B},{K0}+{K1}] -> {O} relu {relu}")


# ---- the audio front end (audio.hip) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fr,H,W", [(1, 28, 12), (5, 28, 12), (2, 3, 5)])       # the network's window, one and five; a map where every pixel is border
def test_audio_conv1(Fr, H, W, place=None):
    place = place or Plain(DEV)
    g = torch.Generator().manual_seed(Fr + H)
    x = 2 * torch.rand(Fr, H, W, generator=g) - 1
    w = 0.5 * torch.randn(64, 1, 3, 3, generator=g) * (2.0 / 9) ** 0.5
    b = 0.1 * torch.randn(64, generator=g)
    # nine fused multiply-adds and the bias add: ten roundings of at most 2^-24 |partial sum| each, and with |x| <= 1 no partial sum
    # exceeds sum |w| + |b|; below 3.3 that is under the 2e-6 of the check whatever the order
    assert float((w.abs().sum(dim=(1, 2, 3)) + b.abs()).max()) < 3.3
    want = F.relu(F.conv2d(x[:, None].double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    wt = w.reshape(64, 9).t().contiguous()                                      # [9][64], tap-major: the engine's layout
    out = place((Fr, H, W, 64), "out")
    _run("eamm_op_audio_conv1", place(x, "in", name="x"), place(wt, "in", name="wt"), place(b, "in", name="bias"), Fr, H, W, out)
    _whole(out, want, 2e-6, f"audio_conv1 [{Fr},{H},{W}]")


@pytest.mark.parametrize("n", [1, 255, 257, 100003])                            # one thread; a 255-thread block; one thread past a block; 391 blocks
def test_audio_scale_is_bit_exact(n, place=None):
    place = place or Plain(DEV)
    s = 1.6
    x = torch.randn(n + 64, generator=torch.Generator().manual_seed(n))
    x[n:] = 1.0                                                                  # the guard i < n: the floats behind the vector stay
    xd = place(x, "inout")
    _run("eamm_op_audio_scale", xd, n, s)
    want = x.numpy().copy()
    want[:n] = want[:n] * np.float32(s)
    assert np.array_equal(xd.cpu().numpy(), want)
