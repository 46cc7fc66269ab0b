"""The emotion video's host side (eamm_amd.video_input): the numpy oracle of S0..S6 against scipy / hand computation, the
Umeyama fit, the homographies, the two draws, the cyclic frame mapping, the config checks and the C entries' argument checks."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from eamm_amd import (EmotionVideo, _lib, align_video, crop_source, crop_source_reference, draw_augmentation,
                      emotion_augmentation_config, perspective_params, similarity_transform)
from eamm_amd import video_input as vi


def _frames(n, h, w, c=3, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, c)).astype(np.uint8)


# ---- warps against scipy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 50), (256, 256), (300, 200)])
def test_bilinear_warp_is_map_coordinates_grid_constant(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(1)
    img = rs.rand(*shape, 3)
    mats = [vi.rotation_matrix(23.0), vi.rotation_matrix(-30.0),
            np.array([[0.9, 0.2, -12.3], [-0.15, 1.1, 7.7]]), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])]
    x, y = vi._grid()
    for m in mats:
        got = vi.warp_reference(img, m)
        c = m[0, 0] * x + m[0, 1] * y + m[0, 2]
        r = m[1, 0] * x + m[1, 1] * y + m[1, 2]
        for k in range(3):
            want = ndi.map_coordinates(img[..., k], [r, c], order=1, mode="grid-constant", cval=0.0)
            np.testing.assert_allclose(got[..., k], want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", [(512, 512), (300, 200), (128, 128), (180, 320)])
def test_resize_is_zoom_of_gaussian(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    f = _frames(1, *shape, seed=2)[0]
    x = f.astype(np.float64) / 255.0
    sig = [max(0.0, (s / 256 - 1) / 2) for s in shape] + [0.0]
    if any(s > 0 for s in sig):
        x = ndi.gaussian_filter(x, sig, mode="mirror", truncate=4.0)
    want = ndi.zoom(x, (256 / shape[0], 256 / shape[1], 1), order=1, mode="mirror", grid_mode=True)
    assert want.shape == (256, 256, 3)
    np.testing.assert_allclose(vi._resize_values(f), want, rtol=0, atol=1e-12)


def test_resize_identity_at_256_and_alpha_dropped():
    f = _frames(2, 256, 256, 4, seed=3)
    np.testing.assert_array_equal(vi.resize_reference(f), f[..., :3])
    # the oracle's arithmetic path gives the identity too: k / 255 * 255 truncates to k for every level
    np.testing.assert_array_equal(vi._trunc_u8(vi._resize_values(f[0])), f[0, ..., :3])


# ---- geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflect", [False, True])
def test_umeyama_recovers_a_similarity(reflect):
    rs = np.random.RandomState(4)
    src = rs.uniform(0, 256, (35, 2))
    s, th, t = 1.3, 0.4, np.array([12.5, -7.25])
    R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    if reflect:
        R = R @ np.diag([1.0, -1.0])
    dst = src @ (s * R).T + t
    got = similarity_transform(src, dst)
    assert got.shape == (2, 3)
    if reflect:
        # the reflection fix keeps det(R) = +1: the least-squares PROPER similarity, in complex form z' = a z + b
        zs, zd = src[:, 0] + 1j * src[:, 1], dst[:, 0] + 1j * dst[:, 1]
        cs, cd = zs - zs.mean(), zd - zd.mean()
        a = (np.conj(cs) * cd).sum() / (np.abs(cs) ** 2).sum()
        b = zd.mean() - a * zs.mean()
        R, s, t = np.array([[a.real, -a.imag], [a.imag, a.real]]), 1.0, np.array([b.real, b.imag])
        assert np.linalg.det(got[:, :2]) > 0
    np.testing.assert_allclose(got[:, :2], s * R, atol=1e-9)
    np.testing.assert_allclose(got[:, 2], t, atol=1e-9)
    both = similarity_transform(src, np.stack([dst, src]))              # vectorised over frames, one template
    np.testing.assert_allclose(both[0], got, atol=1e-12)
    np.testing.assert_allclose(both[1], [[1, 0, 0], [0, 1, 0]], atol=1e-9)


def test_umeyama_degenerate_input_names_the_frame():
    src = np.random.RandomState(5).uniform(0, 256, (35, 2))
    with pytest.raises(ValueError, match="frame 1"):
        similarity_transform(src, np.stack([src, np.full((35, 2), 3.0)]))
    with pytest.raises(ValueError, match="frame 0"):
        similarity_transform(np.full((35, 2), 1.0), src)
    bad = src.copy()
    bad[3, 0] = np.nan
    with pytest.raises(ValueError, match="frame 2.*finite"):
        similarity_transform(src, np.stack([src, src, bad]))


def test_homography_maps_src_onto_dst():
    for p, e in [(20, 20), (-29, 39), (25, -33), (-20, -20)]:
        M, Minv = perspective_params([p], [e])
        src = np.array([[-e, -e], [-e, 256 + e], [256 + e, -e], [256 + e, 256 + e]], float)
        dst = src.copy()
        dst[1, 0] += p
        dst[3, 0] -= p
        h = np.c_[src, np.ones(4)] @ M[0].T
        np.testing.assert_allclose(h[:, :2] / h[:, 2:], dst, atol=1e-9)
        np.testing.assert_allclose(M[0] @ Minv[0], np.eye(3), atol=1e-12)


def _opencv_sample(img, hinv, x, y):
    """One S5 pixel written out by hand: 1/32-pixel coordinates, floor division, replicate clamping, dyadic weights."""
    X0, Y0, W = (hinv[i, 0] * x + hinv[i, 1] * y + hinv[i, 2] for i in range(3))
    w = 32.0 / W
    X, Y = int(round(X0 * w)), int(round(Y0 * w))         # round half to even, as cvRound
    sx, fx = X // 32, X - 32 * (X // 32)
    sy, fy = Y // 32, Y - 32 * (Y // 32)
    cl = lambda v: min(max(v, 0), 255)
    v = (img[cl(sy), cl(sx)] * ((32 - fx) * (32 - fy) / 1024) + img[cl(sy), cl(sx + 1)] * (fx * (32 - fy) / 1024) +
         img[cl(sy + 1), cl(sx)] * ((32 - fx) * fy / 1024) + img[cl(sy + 1), cl(sx + 1)] * (fx * fy / 1024))
    return v


def test_perspective_sample_is_opencv_fixed_point_with_replicate_borders():
    img = np.random.RandomState(6).rand(256, 256, 3)
    shifts = [(-3.3, 4.7), (3.3, -4.7), (0.51, 0.49), (-300.0, 2.0)]
    for dx, dy in shifts:
        hinv = np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])
        got = vi.perspective_reference(img, hinv)
        for x, y in [(0, 0), (255, 0), (0, 255), (255, 255), (100, 37), (254, 1)]:
            np.testing.assert_allclose(got[y, x], _opencv_sample(img, hinv, x, y), rtol=0, atol=1e-15)
    _, Minv = perspective_params([-27], [31])
    got = vi.perspective_reference(img, Minv[0])
    for x, y in [(0, 0), (255, 255), (3, 250), (128, 128)]:
        np.testing.assert_allclose(got[y, x], _opencv_sample(img, Minv[0], x, y), rtol=0, atol=1e-15)


# ---- randomness ----------------------------------------------------------------------------------------------------------
def test_reference_order_draw_consumes_the_generators_in_order():
    n = 4
    pr, nr = random.Random(5), np.random.RandomState(7)
    d = draw_augmentation(n, py_random=pr, np_random=nr)
    pr2, nr2 = random.Random(5), np.random.RandomState(7)
    pr2.random()
    flip = pr2.random() < 0.5
    angle = pr2.uniform(-30, 30)
    noise = np.stack([nr2.rand(60, 100, 3) for _ in range(n)]).astype(np.float32)
    pers, enl = [], []
    for _ in range(n):
        pers.append(nr2.randint(20, 30) * (-1) ** nr2.randint(2))
        enl.append(nr2.randint(20, 40) * (-1) ** nr2.randint(2))
    assert d["flip"] == flip and d["angle"] == angle
    np.testing.assert_array_equal(d["noise"], noise)
    np.testing.assert_array_equal(d["pers"], pers)
    np.testing.assert_array_equal(d["enlarge"], enl)
    assert pr.random() == pr2.random() and nr.rand() == nr2.rand()       # nothing more was consumed
    assert all(20 <= abs(p) < 30 for p in d["pers"]) and all(20 <= abs(e) < 40 for e in d["enlarge"])
    # the default generators are the global modules, as in the demo
    random.seed(11)
    np.random.seed(12)
    g = draw_augmentation(2)
    random.seed(11)
    np.random.seed(12)
    h = draw_augmentation(2, py_random=random, np_random=np.random)
    assert g["angle"] == h["angle"] and np.array_equal(g["noise"], h["noise"])


def test_seeded_draw_and_mouth_noise():
    a, b = draw_augmentation(6, seed=123), draw_augmentation(6, seed=123)
    assert a["flip"] == b["flip"] and a["angle"] == b["angle"] and a["noise_seed"] == 123 and "noise" not in a
    np.testing.assert_array_equal(a["pers"], b["pers"])
    assert -30 <= a["angle"] <= 30 and all(20 <= abs(p) < 30 for p in a["pers"])
    with pytest.raises(ValueError):
        draw_augmentation(2, seed=1, py_random=random.Random(1))
    z = vi.mouth_noise(99, [0, 1, 7])
    assert z.shape == (3, 60, 100, 3) and z.dtype == np.float32 and 0.0 <= z.min() and z.max() < 1.0
    assert abs(float(z.mean()) - 0.5) < 0.01
    np.testing.assert_array_equal(z[2], vi.mouth_noise(99, [7])[0])
    assert not np.array_equal(z[0], vi.mouth_noise(100, [0])[0])
    # one value by plain integer arithmetic: frame 7, row 3, column 5, channel 2
    M64 = (1 << 64) - 1
    G = 0x9E3779B97F4A7C15

    def mix(v):
        v = ((v ^ (v >> 30)) * 0xBF58476D1CE4E5B9) & M64
        v = ((v ^ (v >> 27)) * 0x94D049BB133111EB) & M64
        return v ^ (v >> 31)
    ctr = (7 * 6000 + 3 * 100 + 5) * 3 + 2 + 1
    u = mix((mix((99 + G) & M64) + ctr * G) & M64) >> 40
    assert z[2, 3, 5, 2] == np.float32(u / 16777216.0)


def test_cyclic_mapping_is_np_resize():
    rs = np.random.RandomState(8)
    for n, T in [(3, 7), (5, 3), (4, 4)]:
        aligned = rs.rand(n, 256, 256, 3).astype(np.float32)
        d = draw_augmentation(n, seed=n)
        out = vi.augment_reference(aligned, d, t0=0, t1=T)
        src = np.resize(np.arange(n), T)
        for t in range(T):
            np.testing.assert_array_equal(out[t], vi.augment_reference(aligned, d, t0=int(src[t]), t1=int(src[t]) + 1)[0])
        assert out.shape == (T, 3, 256, 256) and out.dtype == np.float32
        k = out.astype(np.float64) * 255
        assert np.abs(k - np.rint(k)).max() < 1e-4               # every value is float32(k / 255)


def test_augmentation_stages_by_hand():
    """Angle 0, no flip, the identity-like perspective p = e = 20 kept apart: the mouth rectangle holds the noise."""
    aligned = np.random.RandomState(9).rand(1, 256, 256, 3).astype(np.float32)
    d = {"flip": False, "angle": 0.0, "pers": np.array([20]), "enlarge": np.array([20]), "noise_seed": 5}
    _, hinv = perspective_params([0], [20])                      # p = 0: M is the identity
    np.testing.assert_allclose(hinv[0], np.eye(3), atol=1e-12)
    noise = vi.mouth_noise(5, [0])[0]
    img = aligned[0].astype(np.float64)
    img[160:220, 85:185] = noise
    d0 = dict(d, pers=np.array([0]))
    got = vi.augment_reference(aligned, d0)[0].transpose(1, 2, 0)
    np.testing.assert_array_equal(got, (np.clip(np.rint(img * 255), 0, 255) / 255).astype(np.float32))
    flipped = vi.augment_reference(aligned, dict(d0, flip=True))[0].transpose(1, 2, 0)
    np.testing.assert_array_equal(flipped, got[:, ::-1])


# ---- config --------------------------------------------------------------------------------------------------------------
def test_config_is_the_yaml_and_unsupported_parameters_are_refused():
    cfg = emotion_augmentation_config()
    assert cfg == {"crop_mouth_param": {"center_x": 135, "center_y": 190, "mask_width": 100, "mask_height": 60},
                   "rotation_param": {"degrees": 30}, "perspective_param": {"pers_num": 30, "enlarge_num": 40},
                   "flip_param": {"horizontal_flip": True, "time_flip": False},
                   "jitter_param": {"brightness": 0, "contrast": 0, "saturation": 0, "hue": 0}}
    p = vi.check_augmentation_params(cfg)
    assert p["mouth"] == (85, 160, 100, 60) and p["degrees"] == (-30.0, 30.0) and p["horizontal_flip"]
    bad = [({"jitter_param": {"brightness": 0.1, "contrast": 0, "saturation": 0, "hue": 0}}, "brightness"),
           ({"jitter_param": {"brightness": 0, "contrast": 0, "saturation": 0, "hue": 0.2}}, "hue"),
           ({"flip_param": {"horizontal_flip": True, "time_flip": True}}, "time_flip"),
           ({"resize_param": {"ratio": [0.9, 1.1]}}, "resize_param"),
           ({"crop_param": {"size": [256, 256]}}, "crop_param"),
           ({"rotation_param": None}, "rotation_param"),
           ({"perspective_param": {"pers_num": 20, "enlarge_num": 40}}, "pers_num"),
           ({"crop_mouth_param": {"center_x": 250, "center_y": 190, "mask_width": 100, "mask_height": 60}}, "mouth")]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            vi.check_augmentation_params({**cfg, **change})
        with pytest.raises(ValueError, match=word):
            draw_augmentation(2, seed=0, params={**cfg, **change})


# ---- the CPU path and input checks ---------------------------------------------------------------------------------------
def _landmarks(n, seed=10):
    rs = np.random.RandomState(seed)
    base = rs.uniform(40, 216, (68, 2))
    out = []
    for i in range(n):
        th, s, t = rs.uniform(-0.1, 0.1), rs.uniform(0.95, 1.05), rs.uniform(-5, 5, 2)
        R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        out.append((base - 128) @ (s * R).T + 128 + t)
    return np.stack(out)


def test_cpu_path_is_the_oracle():
    f = _frames(3, 300, 200, 4, seed=11)
    lm = _landmarks(3)
    a = align_video(f, lm, device="cpu").numpy()
    np.testing.assert_array_equal(a, vi.align_reference(f, lm))
    assert a.shape == (3, 256, 256, 3) and a.dtype == np.float32
    # frame 0 is fitted onto its own points: the identity map, so the aligned frame is the resized frame / 255
    np.testing.assert_allclose(a[0], vi.resize_reference(f)[0] / 255.0, atol=1e-6)
    ev = EmotionVideo(f, lm, seed=3, device="cpu")
    np.testing.assert_array_equal(ev[1:5].numpy(), vi.emotion_video_reference(f, lm, draw=ev.draw, T=5)[1:5])
    img, tmpl = _frames(1, 320, 240, seed=12)[0], _landmarks(1, seed=13)[0]
    np.testing.assert_array_equal(crop_source(img, tmpl + 7.0, tmpl, device="cpu").numpy(), crop_source_reference(img, tmpl + 7.0, tmpl))


def test_bad_input_is_refused_by_name():
    f = _frames(2, 256, 256)
    lm = _landmarks(2)
    with pytest.raises(ValueError, match="uint8"):
        EmotionVideo(f.astype(np.float32) / 255, lm, seed=0, device="cpu")
    with pytest.raises(ValueError, match="C = 3 | 4"):
        EmotionVideo(np.zeros((2, 256, 256, 5), np.uint8), lm, seed=0, device="cpu")
    with pytest.raises(ValueError, match="landmarks"):
        EmotionVideo(f, lm[:1], seed=0, device="cpu")
    with pytest.raises(ValueError, match="landmarks"):
        EmotionVideo(f, lm[:, :20], seed=0, device="cpu")
    with pytest.raises(ValueError, match="empty"):
        EmotionVideo(np.zeros((0, 256, 256, 3), np.uint8), None, seed=0, device="cpu")
    with pytest.raises(ValueError, match="landmarks"):
        crop_source(f[0], lm[0][:40], lm[1], device="cpu")
    with pytest.raises(ValueError, match="radius"):
        vi.gaussian_taps(9000)


def test_c_entries_reject_bad_arguments_without_a_launch():
    L = _lib.lib()
    buf = C.c_void_p(16)                    # never dereferenced: every call below fails its argument check
    taps = (C.c_double * 1)(1.0)
    rot = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    for n, H, W, Ch, r in [(0, 10, 10, 3, 0), (1, 10, 10, 5, 0), (1, 0, 10, 3, 0), (1, 10, 10, 3, 32)]:
        assert L.eamm_op_resize_aa(0, buf, n, H, W, Ch, taps, r, taps, 0, buf, None) == _lib.ERR_ARG
        assert b"eamm_op_resize_aa" in L.eamm_last_error(None)
    for n, Ch, mode in [(0, 3, 0), (1, 2, 0), (1, 3, 2)]:
        assert L.eamm_op_similarity_warp(0, buf, n, 16, 16, Ch, buf, mode, buf, None) == _lib.ERR_ARG
    for n_src, t0, count, mx, my, mw, mh in [(0, 0, 1, 85, 160, 100, 60), (1, -1, 1, 85, 160, 100, 60), (1, 0, 0, 85, 160, 100, 60),
                                             (1, 0, 1, 200, 160, 100, 60), (1, 0, 1, 85, 160, 0, 60)]:
        assert L.eamm_op_emotion_augment(0, buf, n_src, t0, count, 0, rot, buf, None, 0, mx, my, mw, mh, buf, None) == _lib.ERR_ARG
        assert b"eamm_op_emotion_augment" in L.eamm_last_error(None)
