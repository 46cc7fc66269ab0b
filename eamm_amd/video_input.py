"""The emotion video the demo feeds ``Emotion_k`` -- its ``transformed_video`` (demo.py:484-493) -- and the cropped portrait
(demo.py:433-454, 476-477), built on the device from uint8 frames and the caller's 68-point landmarks.

    reference (host)                                                   here
    -----------------------------------------------------------------  ---------------------------------------------------------
    resize(frame, (256, 256))[..., :3]                 demo.py:490     S0  eamm_op_resize_aa (skipped at 256 x 256 input)
    np.array(frame * 255, dtype=np.uint8)              demo.py:162         truncation, inside the same kernel
    SimilarityTransform().estimate(template[:35],      demo.py:146-182 S1  similarity_transform (host, float64) +
        shape[:35]); warp(image, tform, (256, 256))                        eamm_op_similarity_warp -> float32 [N,256,256,3]
    AllAugmentationTransform(**augmentation_params)    demo.py:184-190 S2..S6 eamm_op_emotion_augment, fused, per requested
        MouthCrop, RandomFlip, RandomRotation,         augmentation.py     frame: EmotionVideo[t0:t1] -> [t1-t0,3,256,256]
        RandomPerspective, ColorJitter(0, 0, 0, 0)     :175-431
    np.resize(transformed_video, (T, 256, 256, 3))     demo.py:498-502     output frame t is source frame t mod N
    crop_image: similarity warp of the portrait,       demo.py:433-454 crop_source -> [1,3,256,256] float32
        points 0..46 onto M003_template, uint8

The stage semantics:
  S0  x / 255 (float64), Gaussian blur per shrinking axis (sigma = (in / out - 1) / 2, radius int(4 sigma + 0.5), 'mirror'
      borders; rows, then columns), linear zoom at in = (o + 0.5) in / 256 - 0.5 with mirrored neighbours; trunc(255 v)
  S1  output (x, y) samples the frame at T (x, y, 1), T the Umeyama similarity from the template's points to the frame's;
      bilinear with floor / ceil neighbours, a neighbour outside the image reads 0; float32
  S2  rows 160..219, columns 85..184 replaced by uniform [0, 1) noise (float32), fresh per source frame
  S3  horizontal flip (one coin per clip)
  S4  rotation by theta about (127.5, 127.5): input = R(theta) ((x, y) - c) + c, bilinear, zero outside
  S5  perspective: OpenCV's warpPerspective with M^-1, coordinates rounded to 1/32 pixel, BORDER_REPLICATE
  S6  rint(255 v) clipped to [0, 255], / 255, float32

Randomness: ``draw_augmentation`` either consumes Python's ``random`` and ``np.random`` (or the generators passed) in the
reference's order -- the reference run with those seeds -- or draws from ``np.random.default_rng(seed)`` with the mouth noise
made on the device by a counter-based hash (``mouth_noise`` is its numpy twin, bit for bit).

The ``*_reference`` functions are a float64 numpy model of every step (the tests check the kernels against it) and the CPU
path (a CPU ``device``).  They perform the device's float64 operations in the same order; none needs scikit-image, OpenCV or
scipy.  Landmarks are the caller's
(dlib's 68-point predictor in the demo), in the coordinates of the frames as given to S1: the 256 x 256 resized frames for the
video, the image as loaded for the portrait.  Channel order is the caller's (the demo reads the portrait as BGR with cv2.imread;
nothing here swaps channels).
"""
from __future__ import annotations

import ctypes as C
import math
import random as _py_random
from typing import Optional

import numpy as np
import torch

from .config import emotion_augmentation_config

OUT = 256
ALIGN_POINTS = 35              # demo.py:171-172: points 0..34 (jaw, eyebrows, nose)
CROP_POINTS = 47               # demo.py:447-448: points 0..46
SHIFTED_EMOTIONS = ("surprised", "fear")     # demo.py:161-162: the template is moved up by 10 pixels
TEMPLATE_SHIFT = np.array([0.0, 10.0])
TRUNCATE = 4.0                 # ndi.gaussian_filter's default
MAX_RADIUS = 31                # eamm_op_resize_aa: tap radius < 32
MAX_LAUNCH = 65535             # frames per launch (grid.y)
_G = np.uint64(0x9E3779B97F4A7C15)


# ---- configuration -------------------------------------------------------------------------------------------------------
def check_augmentation_params(params=None) -> dict:
    """The config's ``augmentation_params`` -> the normalised steps; what is not implemented is refused by name."""
    p = emotion_augmentation_config() if params is None else params
    if not isinstance(p, dict):
        raise ValueError(f"augmentation params must be a dict (the config's augmentation_params), got {type(p).__name__}")
    for key in ("resize_param", "crop_param"):
        if p.get(key) is not None:
            raise ValueError(f"augmentation params: {key} is not implemented (the shipped config has none)")
    known = {"crop_mouth_param", "rotation_param", "perspective_param", "flip_param", "jitter_param", "resize_param", "crop_param"}
    unknown = sorted(set(p) - known)
    if unknown:
        raise ValueError(f"augmentation params: unknown entries {unknown}")
    for key in ("crop_mouth_param", "rotation_param", "perspective_param", "flip_param", "jitter_param"):
        if p.get(key) is None:
            raise ValueError(f"augmentation params: {key} is required (augmentation without it is not implemented)")
    jit = p["jitter_param"]
    for name in ("brightness", "contrast", "saturation", "hue"):
        if float(jit.get(name, 0)) != 0.0:
            raise ValueError(f"augmentation params: jitter_param.{name} = {jit[name]}: ColorJitter with non-zero parameters is "
                             f"not implemented")
    flip = p["flip_param"]
    if flip.get("time_flip", False):
        raise ValueError("augmentation params: flip_param.time_flip is not implemented")
    m = p["crop_mouth_param"]
    w, h = int(m["mask_width"]), int(m["mask_height"])
    x0, y0 = int(m["center_x"]) - int(w / 2), int(m["center_y"]) - int(h / 2)      # augmentation.py:198-199
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > OUT or y0 + h > OUT:
        raise ValueError(f"augmentation params: the mouth rectangle x {x0}..{x0 + w}, y {y0}..{y0 + h} must lie inside {OUT} x {OUT}")
    deg = p["rotation_param"]["degrees"]
    if isinstance(deg, (int, float)):
        if deg < 0:
            raise ValueError("augmentation params: rotation_param.degrees must be >= 0")
        lo, hi = -float(deg), float(deg)
    else:
        if len(deg) != 2:
            raise ValueError("augmentation params: rotation_param.degrees is a number or a (min, max) pair")
        lo, hi = float(deg[0]), float(deg[1])
    pers, enl = int(p["perspective_param"]["pers_num"]), int(p["perspective_param"]["enlarge_num"])
    if pers <= 20 or enl <= 20:
        raise ValueError(f"augmentation params: pers_num and enlarge_num must exceed 20 (randint(20, n)), got {pers}, {enl}")
    return {"mouth": (x0, y0, w, h), "degrees": (lo, hi), "pers_num": pers, "enlarge_num": enl,
            "horizontal_flip": bool(flip.get("horizontal_flip", False))}


# ---- randomness ----------------------------------------------------------------------------------------------------------
def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mouth_noise(seed: int, frames, mouth_h: int = 60, mouth_w: int = 100) -> np.ndarray:
    """The device's mouth noise (include/eamm_hip.h, eamm_op_emotion_augment) of source frames ``frames``: float32
    [len(frames), mouth_h, mouth_w, 3], value = (mix64(mix64(seed + G) + ctr G) >> 40) 2^-24 with
    ctr = (frame mouth_h mouth_w + row mouth_w + col) 3 + channel + 1."""
    frames = np.asarray(frames, dtype=np.uint64).reshape(-1)
    px = np.uint64(mouth_h * mouth_w)
    with np.errstate(over="ignore"):
        key = _mix64(np.array([int(seed) % (1 << 64)], dtype=np.uint64) + _G)
        idx = np.arange(mouth_h * mouth_w * 3, dtype=np.uint64).reshape(1, mouth_h, mouth_w, 3)
        ctr = frames.reshape(-1, 1, 1, 1) * px * np.uint64(3) + idx + np.uint64(1)
        u = _mix64(key + ctr * _G) >> np.uint64(40)
    return u.astype(np.float32) * np.float32(1.0 / 16777216.0)


def draw_augmentation(n_frames: int, seed: Optional[int] = None, py_random=None, np_random=None, params=None) -> dict:
    """The clip's augmentation parameters: ``{'flip', 'angle', 'pers' [N], 'enlarge' [N]}`` plus ``'noise'`` (float32
    [N,h,w,3], host) or ``'noise_seed'``.

    Reference order (``seed`` None): ``py_random`` (default: the ``random`` module) gives random() for the time-flip check,
    random() for the horizontal flip (flip when < 0.5) and uniform(lo, hi) for the angle; ``np_random`` (default: ``np.random``)
    gives rand(h, w, 3) per frame for all frames, then per frame randint(20, pers_num), randint(2), randint(20, enlarge_num),
    randint(2) (augmentation.py:97-99, 207, 245, 279-280).  Seeded: the same quantities from ``np.random.default_rng(seed)``,
    the noise from the device hash with ``noise_seed = seed``."""
    cfg = check_augmentation_params(params)
    n = int(n_frames)
    if n < 1:
        raise ValueError(f"draw_augmentation: the video has no frames (N = {n})")
    lo, hi = cfg["degrees"]
    x0, y0, w, h = cfg["mouth"]
    if seed is not None:
        if py_random is not None or np_random is not None:
            raise ValueError("draw_augmentation: pass either seed or the reference-order generators, not both")
        rng = np.random.default_rng(int(seed))
        flip = bool(rng.random() < 0.5) and cfg["horizontal_flip"]
        angle = lo + (hi - lo) * float(rng.random())
        pers = rng.integers(20, cfg["pers_num"], n) * (1 - 2 * rng.integers(0, 2, n))
        enl = rng.integers(20, cfg["enlarge_num"], n) * (1 - 2 * rng.integers(0, 2, n))
        return {"flip": flip, "angle": angle, "pers": pers.astype(np.int64), "enlarge": enl.astype(np.int64),
                "noise_seed": int(seed) % (1 << 64)}
    pr = _py_random if py_random is None else py_random
    nr = np.random if np_random is None else np_random
    pr.random()                                                     # RandomFlip: the time-flip coin (time_flip is False)
    flip = pr.random() < 0.5 and cfg["horizontal_flip"]
    angle = pr.uniform(lo, hi)
    noise = np.stack([nr.rand(h, w, 3) for _ in range(n)]).astype(np.float32)     # MouthCrop (float64 into a float32 frame)
    pers, enl = np.empty(n, np.int64), np.empty(n, np.int64)
    for i in range(n):                                              # RandomPerspective
        pers[i] = nr.randint(20, cfg["pers_num"]) * pow(-1, nr.randint(2))
        enl[i] = nr.randint(20, cfg["enlarge_num"]) * pow(-1, nr.randint(2))
    return {"flip": bool(flip), "angle": float(angle), "pers": pers, "enlarge": enl, "noise": noise}


# ---- geometry (host, float64) --------------------------------------------------------------------------------------------
def similarity_transform(src_pts, dst_pts) -> np.ndarray:
    """skimage's ``SimilarityTransform().estimate(src, dst)`` (``_umeyama`` with scale) in float64: [P,2] / [P,2] -> [2,3], or
    vectorised over frames, [N,P,2] (or one [P,2] for all) -> [N,2,3].  Row r of the result maps (x, y, 1) of a src point to
    its dst point.  Degenerate points (all equal on either side, or not finite) raise a ValueError naming the frame."""
    src, dst = np.asarray(src_pts, dtype=np.float64), np.asarray(dst_pts, dtype=np.float64)
    single = src.ndim == 2 and dst.ndim == 2
    if src.ndim == 2:
        src = np.broadcast_to(src, dst.shape if dst.ndim == 3 else (1,) + src.shape)
    if dst.ndim == 2:
        dst = np.broadcast_to(dst, src.shape)
    if src.ndim != 3 or src.shape != dst.shape or src.shape[2] != 2 or src.shape[1] < 2:
        raise ValueError(f"similarity_transform: point sets must both be [P,2] or [N,P,2] with P >= 2, got "
                         f"{np.shape(src_pts)} / {np.shape(dst_pts)}")
    n, num = src.shape[0], src.shape[1]
    out = np.empty((n, 2, 3))
    for i in range(n):
        s, d = src[i], dst[i]
        if not (np.isfinite(s).all() and np.isfinite(d).all()):
            raise ValueError(f"similarity_transform: frame {i}: the landmarks are not finite")
        s_mean, d_mean = s.mean(axis=0), d.mean(axis=0)
        sd, dd = s - s_mean, d - d_mean
        var = sd.var(axis=0).sum()
        A = dd.T @ sd / num
        rank = np.linalg.matrix_rank(A)
        if var == 0.0 or rank == 0:
            raise ValueError(f"similarity_transform: frame {i}: degenerate landmarks (all points equal)")
        dvec = np.ones(2)
        if np.linalg.det(A) < 0:
            dvec[1] = -1.0
        U, S, V = np.linalg.svd(A)
        if rank == 1 and np.linalg.det(U) * np.linalg.det(V) <= 0:
            R = U @ np.diag([1.0, -1.0]) @ V
        elif rank == 1:
            R = U @ V
        else:
            R = U @ np.diag(dvec) @ V
        scale = 1.0 / var * (S @ dvec)
        out[i, :, 2] = d_mean - scale * (R @ s_mean)
        out[i, :, :2] = R * scale
    return out[0] if single else out


def alignment_maps(landmarks, emotion: Optional[str] = None) -> np.ndarray:
    """get_aligned_image's transforms (demo.py:146-182): [N,68,2] landmarks of the resized frames -> [N,2,3], frame 0's points
    (moved up by 10 for 'surprised' / 'fear') as the template, points 0..34 fitted per frame."""
    lm = np.asarray(landmarks, dtype=np.float64)
    template = lm[0].copy()
    if emotion in SHIFTED_EMOTIONS:
        template = template - TEMPLATE_SHIFT
    return similarity_transform(template[:ALIGN_POINTS], lm[:, :ALIGN_POINTS])


def rotation_matrix(angle: float) -> np.ndarray:
    """skimage.transform.rotate's inverse map on 256 x 256 (centre (127.5, 127.5)): [2,3], input = R (x, y, 1)."""
    c = OUT / 2.0 - 0.5
    t1 = np.array([[1.0, 0.0, c], [0.0, 1.0, c], [0.0, 0.0, 1.0]])
    r = np.deg2rad(angle)
    t2 = np.array([[math.cos(r), -math.sin(r), 0.0], [math.sin(r), math.cos(r), 0.0], [0.0, 0.0, 1.0]])
    t3 = np.array([[1.0, 0.0, -c], [0.0, 1.0, -c], [0.0, 0.0, 1.0]])
    return (t1 @ (t2 @ t3))[:2]                      # tform3 + tform2 + tform1


def perspective_params(pers, enlarge, size: int = OUT):
    """RandomPerspective's homographies (augmentation.py:279-291): (M, M^-1), each [N,3,3] float64.  M takes
    src = [(-e,-e), (-e,size+e), (size+e,-e), (size+e,size+e)] to the same points with the second x moved by +p and the fourth
    by -p (cv2.getPerspectiveTransform); warpPerspective samples the input at M^-1 (x, y, 1)."""
    p = np.asarray(pers, dtype=np.float64).reshape(-1)
    e = np.asarray(enlarge, dtype=np.float64).reshape(-1)
    n = p.shape[0]
    src = np.stack([np.stack([-e, -e], 1), np.stack([-e, size + e], 1), np.stack([size + e, -e], 1),
                    np.stack([size + e, size + e], 1)], 1)                        # [N,4,2] (x, y)
    dst = src.copy()
    dst[:, 1, 0] += p
    dst[:, 3, 0] -= p
    A = np.zeros((n, 8, 8))
    b = np.zeros((n, 8))
    for k in range(4):
        x, y, u, v = src[:, k, 0], src[:, k, 1], dst[:, k, 0], dst[:, k, 1]
        A[:, k, 0], A[:, k, 1], A[:, k, 2], A[:, k, 6], A[:, k, 7] = x, y, 1.0, -x * u, -y * u
        A[:, k + 4, 3], A[:, k + 4, 4], A[:, k + 4, 5], A[:, k + 4, 6], A[:, k + 4, 7] = x, y, 1.0, -x * v, -y * v
        b[:, k], b[:, k + 4] = u, v
    h = np.linalg.solve(A, b[..., None])[..., 0]
    M = np.concatenate([h, np.ones((n, 1))], 1).reshape(n, 3, 3)
    return M, np.linalg.inv(M)


def gaussian_taps(in_size: int, out_size: int = OUT) -> np.ndarray:
    """S0's normalised taps along one axis (ndi.gaussian_filter with sigma = max(0, (in / out - 1) / 2), truncate 4): [2r+1];
    [1.0] when the axis does not shrink."""
    sigma = max(0.0, (in_size / out_size - 1.0) / 2.0)
    if sigma <= 1e-15:
        return np.ones(1)
    r = int(TRUNCATE * sigma + 0.5)
    if r > MAX_RADIUS:
        raise ValueError(f"resize: an axis of {in_size} pixels needs a Gaussian radius of {r} (at most {MAX_RADIUS}: sides up to "
                         f"about 4000 pixels)")
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


# ---- the numpy model ------------------------------------------------------------------------------------------------------
def _mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def _resize_values(frame) -> np.ndarray:
    """S0 before the truncation: uint8 [H,W,C] -> float64 [256,256,3]."""
    f = np.asarray(frame)
    H, W = f.shape[:2]
    x = f[..., :3].astype(np.float64) / 255.0
    wy, wx = gaussian_taps(H), gaussian_taps(W)
    ry, rx = len(wy) // 2, len(wx) // 2
    rows = np.zeros_like(x)
    for i in range(2 * ry + 1):                                    # along rows (axis 0) first
        rows = rows + wy[i] * x[_mirror(np.arange(H) + i - ry, H)]
    b = np.zeros_like(x)
    for j in range(2 * rx + 1):
        b = b + wx[j] * rows[:, _mirror(np.arange(W) + j - rx, W)]
    o = np.arange(OUT, dtype=np.float64)
    cy, cx = (o + 0.5) * (H / OUT) - 0.5, (o + 0.5) * (W / OUT) - 0.5
    fy0, fx0 = np.floor(cy), np.floor(cx)
    fy, fx = (cy - fy0)[:, None, None], (cx - fx0)[None, :, None]
    y0, y1 = _mirror(fy0.astype(np.int64), H), _mirror(fy0.astype(np.int64) + 1, H)
    x0, x1 = _mirror(fx0.astype(np.int64), W), _mirror(fx0.astype(np.int64) + 1, W)
    top = (1.0 - fx) * b[y0][:, x0] + fx * b[y0][:, x1]
    bottom = (1.0 - fx) * b[y1][:, x0] + fx * b[y1][:, x1]
    return (1.0 - fy) * top + fy * bottom


def _trunc_u8(v) -> np.ndarray:
    return np.clip(np.trunc(v * 255.0), 0.0, 255.0).astype(np.uint8)


def resize_reference(frames) -> np.ndarray:
    """S0 + demo.py:162's truncation: uint8 [N,H,W,C] -> uint8 [N,256,256,3] (the frames themselves at 256 x 256)."""
    f = np.asarray(frames)
    if f.shape[1:3] == (OUT, OUT):
        return np.ascontiguousarray(f[..., :3])
    return np.stack([_trunc_u8(_resize_values(fr)) for fr in f])


def _bilinear_zero(img, r, c) -> np.ndarray:
    """skimage's bilinear_interpolation, mode 'constant', cval 0: img [H,W,3] float64 at rows r / columns c (same shape)."""
    H, W = img.shape[:2]
    fr, fc, cr, cc = np.floor(r), np.floor(c), np.ceil(r), np.ceil(c)
    dr, dc = (r - fr)[..., None], (c - fc)[..., None]

    def px(rr, ccc):
        ok = (rr >= 0) & (rr < H) & (ccc >= 0) & (ccc < W)
        ri = np.where(ok, rr, 0).astype(np.int64)
        ci = np.where(ok, ccc, 0).astype(np.int64)
        return np.where(ok[..., None], img[ri, ci], 0.0)
    tl, tr, bl, br = px(fr, fc), px(fr, cc), px(cr, fc), px(cr, cc)
    top = (1.0 - dc) * tl + dc * tr
    bottom = (1.0 - dc) * bl + dc * br
    return (1.0 - dr) * top + dr * bottom


def _grid():
    y, x = np.meshgrid(np.arange(OUT, dtype=np.float64), np.arange(OUT, dtype=np.float64), indexing="ij")
    return x, y


def warp_reference(img, m) -> np.ndarray:
    """Output (x, y) of 256 x 256 samples img [H,W,3] (float64) at m (x, y, 1), m [2,3]: S1 and S4's common warp."""
    x, y = _grid()
    c = m[0, 0] * x + m[0, 1] * y + m[0, 2]
    r = m[1, 0] * x + m[1, 1] * y + m[1, 2]
    return _bilinear_zero(img, r, c)


def perspective_reference(img, hinv) -> np.ndarray:
    """S5: cv2.warpPerspective(img, M, (256, 256), borderMode=BORDER_REPLICATE) of img [256,256,3] float64, given M^-1 [3,3]."""
    x, y = _grid()
    h = np.asarray(hinv, dtype=np.float64).reshape(9)
    X0 = h[0] * x + h[1] * y + h[2]
    Y0 = h[3] * x + h[4] * y + h[5]
    Wd = h[6] * x + h[7] * y + h[8]
    with np.errstate(divide="ignore"):
        Wd = np.where(Wd != 0.0, 32.0 / np.where(Wd != 0.0, Wd, 1.0), 0.0)
    lim = (float(np.iinfo(np.int32).min), float(np.iinfo(np.int32).max))
    X = np.rint(np.clip(X0 * Wd, *lim)).astype(np.int64)
    Y = np.rint(np.clip(Y0 * Wd, *lim)).astype(np.int64)
    sx, sy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
    xs0, xs1 = np.clip(sx, 0, OUT - 1), np.clip(sx + 1, 0, OUT - 1)
    ys0, ys1 = np.clip(sy, 0, OUT - 1), np.clip(sy + 1, 0, OUT - 1)
    w0 = (((32 - ax) * (32 - ay)) / 1024.0)[..., None]
    w1 = ((ax * (32 - ay)) / 1024.0)[..., None]
    w2 = (((32 - ax) * ay) / 1024.0)[..., None]
    w3 = ((ax * ay) / 1024.0)[..., None]
    return img[ys0, xs0] * w0 + img[ys0, xs1] * w1 + img[ys1, xs0] * w2 + img[ys1, xs1] * w3


def _landmark_array(landmarks, n, points, who) -> np.ndarray:
    lm = landmarks.detach().cpu().numpy() if isinstance(landmarks, torch.Tensor) else landmarks
    lm = np.asarray(lm, dtype=np.float64)
    if lm.ndim != 3 or lm.shape[0] != n or lm.shape[1] < points or lm.shape[2] != 2:
        raise ValueError(f"{who}: landmarks must be [N,68,2] (at least {points} points) with N = {n} frames, got {lm.shape}")
    return lm


def _frames_u8(frames, who, single=False):
    """-> uint8 numpy array or torch tensor [N,H,W,C] (C = 3 | 4); ValueError for anything else."""
    if isinstance(frames, (list, tuple)):
        frames = np.stack([np.asarray(f) for f in frames]) if len(frames) else np.zeros((0,), np.uint8)
    if isinstance(frames, np.ndarray):
        dtype_ok, shape = frames.dtype == np.uint8, frames.shape
    elif isinstance(frames, torch.Tensor):
        dtype_ok, shape = frames.dtype == torch.uint8, tuple(frames.shape)
    else:
        raise ValueError(f"{who}: frames must be a uint8 numpy array or torch tensor, got {type(frames).__name__}")
    want = 3 if single else 4
    if not dtype_ok:
        raise ValueError(f"{who}: frames must be uint8 (as read from the video / image file), got {frames.dtype}")
    if len(shape) != want or shape[-1] not in (3, 4):
        raise ValueError(f"{who}: expected {'[H,W,C]' if single else '[N,H,W,C]'} with C = 3 | 4, got {shape}")
    if min(shape) < 1:
        raise ValueError(f"{who}: the {'image' if single else 'video'} is empty ({shape})")
    return frames


def align_reference(frames, landmarks=None, emotion: Optional[str] = None) -> np.ndarray:
    """S0 + S1 in numpy: uint8 [N,H,W,C] -> float32 [N,256,256,3] (landmarks None: the resized frames / 255)."""
    f = _frames_u8(frames, "align_reference")
    f = f.cpu().numpy() if isinstance(f, torch.Tensor) else f
    r = resize_reference(f)
    if landmarks is None:
        return (r.astype(np.float64) / 255.0).astype(np.float32)
    maps = alignment_maps(_landmark_array(landmarks, len(f), ALIGN_POINTS, "align_reference"), emotion)
    return np.stack([warp_reference(r[i].astype(np.float64) / 255.0, maps[i]).astype(np.float32) for i in range(len(f))])


def augment_reference(aligned, draw: dict, params=None, t0: int = 0, t1: Optional[int] = None) -> np.ndarray:
    """S2..S6 in numpy: aligned float32 [N,256,256,3] -> float32 [t1-t0,3,256,256], output frame t from source frame t mod N."""
    cfg = check_augmentation_params(params)
    a = np.asarray(aligned)
    n = a.shape[0]
    t1 = n if t1 is None else int(t1)
    x0, y0, w, h = cfg["mouth"]
    rot = rotation_matrix(draw["angle"])
    _, hinv = perspective_params(draw["pers"], draw["enlarge"])
    out = np.empty((t1 - t0, 3, OUT, OUT), np.float32)
    for t in range(t0, t1):
        s = t % n
        img = a[s].astype(np.float64)
        noise = draw["noise"][s] if "noise" in draw else mouth_noise(draw["noise_seed"], [s], h, w)[0]
        img[y0:y0 + h, x0:x0 + w] = noise.astype(np.float64)        # S2
        if draw["flip"]:
            img = img[:, ::-1]                                        # S3
        img = warp_reference(img, rot)                                # S4
        img = perspective_reference(img, hinv[s])                     # S5
        q = np.clip(np.rint(img * 255.0), 0.0, 255.0)                 # S6
        out[t - t0] = (q / 255.0).astype(np.float32).transpose(2, 0, 1)
    return out


def emotion_video_reference(frames, landmarks=None, *, emotion: Optional[str] = None, params=None, seed: Optional[int] = None,
                            py_random=None, np_random=None, draw: Optional[dict] = None, T: Optional[int] = None) -> np.ndarray:
    """The reference's transformed_video after np.resize to T frames (demo.py:490-502): float32 [T,3,256,256] (T default N).
    ``draw`` (e.g. ``EmotionVideo.draw``) replaces the draw from ``seed`` / the generators."""
    f = _frames_u8(frames, "emotion_video_reference")
    n = f.shape[0]
    if landmarks is not None:
        _landmark_array(landmarks, n, ALIGN_POINTS, "emotion_video_reference")
    aligned = align_reference(f, landmarks, emotion)
    if draw is None:
        draw = draw_augmentation(n, seed=seed, py_random=py_random, np_random=np_random, params=params)
    return augment_reference(aligned, draw, params, 0, n if T is None else int(T))


def crop_source_reference(image, landmarks, template) -> np.ndarray:
    """crop_image (demo.py:433-454) + img_as_float32 (demo.py:476): uint8 [H,W,C] -> float32 [1,3,256,256] = trunc(255 v) / 255."""
    img = _frames_u8(image, "crop_source_reference", single=True)
    img = img.cpu().numpy() if isinstance(img, torch.Tensor) else img
    m = _crop_map(landmarks, template, "crop_source_reference")
    v = warp_reference(img[..., :3].astype(np.float64) / 255.0, m)
    q = np.clip(np.trunc(v * 255.0), 0.0, 255.0)
    return (q / 255.0).astype(np.float32).transpose(2, 0, 1)[None]


def _crop_map(landmarks, template, who) -> np.ndarray:
    lm = _landmark_array(np.asarray(landmarks, dtype=np.float64)[None], 1, CROP_POINTS, who)[0]
    tp = _landmark_array(np.asarray(template, dtype=np.float64)[None], 1, CROP_POINTS, who)[0]
    return similarity_transform(tp[:CROP_POINTS], lm[:CROP_POINTS])


# ---- the device path -----------------------------------------------------------------------------------------------------
def _device(device, frames):
    if device is not None:
        d = torch.device(device)
    elif isinstance(frames, torch.Tensor) and frames.is_cuda:
        d = frames.device
    else:
        d = torch.device("cuda", torch.cuda.current_device())
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _upload_u8(frames, dev) -> torch.Tensor:
    x = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
    return x.to(dev).contiguous()


def _resize_device(x: torch.Tensor) -> torch.Tensor:
    from . import _op
    n, H, W, Ch = (int(s) for s in x.shape)
    if (H, W) == (OUT, OUT):
        return x[..., :3].contiguous()
    wy, wx = gaussian_taps(H), gaussian_taps(W)
    ty, tx = (C.c_double * len(wy))(*wy), (C.c_double * len(wx))(*wx)
    out = torch.empty((n, OUT, OUT, 3), dtype=torch.uint8, device=x.device)
    for a in range(0, n, MAX_LAUNCH):
        b = min(n, a + MAX_LAUNCH)
        _op.call("resize_aa", x.device, x[a:b], b - a, H, W, Ch, ty, len(wy) // 2, tx, len(wx) // 2, out[a:b])
    return out


def _warp_device(x: torch.Tensor, maps: np.ndarray, mode: int) -> torch.Tensor:
    from . import _op
    n, H, W, Ch = (int(s) for s in x.shape)
    m = torch.from_numpy(np.ascontiguousarray(maps.reshape(n, 6), dtype=np.float64)).to(x.device)
    shape = (n, OUT, OUT, 3) if mode == 0 else (n, 3, OUT, OUT)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    for a in range(0, n, MAX_LAUNCH):
        b = min(n, a + MAX_LAUNCH)
        _op.call("similarity_warp", x.device, x[a:b], b - a, H, W, Ch, m[a:b], mode, out[a:b])
    return out


_IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def align_video(frames, landmarks=None, emotion: Optional[str] = None, device=None) -> torch.Tensor:
    """S0 + S1 (demo.py:490 then get_aligned_image): uint8 [N,H,W,C] frames (numpy or torch, C = 3 | 4) and their [N,68,2]
    landmarks in the RESIZED frames' coordinates -> aligned float32 [N,256,256,3] on ``device`` (default: the frames' GPU or the
    current one; a CPU device runs ``align_reference``).  ``emotion`` 'surprised' / 'fear' moves the template up by 10 pixels.
    ``landmarks`` None: the frames are taken as aligned (S1 skipped; the resized frame / 255)."""
    f = _frames_u8(frames, "align_video")
    n = int(f.shape[0])
    lm = None if landmarks is None else _landmark_array(landmarks, n, ALIGN_POINTS, "align_video")
    maps = np.broadcast_to(_IDENTITY, (n, 2, 3)) if lm is None else alignment_maps(lm, emotion)
    dev = _device(device, f)
    if dev.type != "cuda":
        return torch.from_numpy(align_reference(f, lm, emotion))
    r = _resize_device(_upload_u8(f, dev))
    return _warp_device(r, maps, 0)


def crop_source(image, landmarks, template, device=None) -> torch.Tensor:
    """The demo's source image (crop_image, demo.py:433-454, then img_as_float32): the similarity fitted from the template's
    points 0..46 onto the image's (landmarks in the image's coordinates), the image warped to 256 x 256 and truncated to uint8
    -> float32 [1,3,256,256] = k / 255 on ``device``.  ``image`` uint8 [H,W,C] (C = 3 | 4), channels kept in the caller's order
    (the demo's cv2.imread gives BGR).  ``template``: [>=47,2] (the demo's M003_template.npy)."""
    img = _frames_u8(image, "crop_source", single=True)
    m = _crop_map(landmarks, template, "crop_source")
    dev = _device(device, img)
    if dev.type != "cuda":
        return torch.from_numpy(crop_source_reference(img, landmarks, template))
    return _warp_device(_upload_u8(img, dev)[None].contiguous(), m[None], 1)


def _check_draw(draw: dict, n: int, cfg: dict):
    """A given draw must hold what the kernel reads: N perspective pairs and [N,h,w,3] float32 noise or a noise seed."""
    _, _, w, h = cfg["mouth"]
    if not all(k in draw for k in ("flip", "angle", "pers", "enlarge")) or ("noise" in draw) == ("noise_seed" in draw):
        raise ValueError("EmotionVideo: draw needs flip, angle, pers, enlarge and one of noise / noise_seed")
    if np.shape(draw["pers"]) != (n,) or np.shape(draw["enlarge"]) != (n,):
        raise ValueError(f"EmotionVideo: draw's pers / enlarge must hold N = {n} values each")
    if "noise" in draw:
        z = draw["noise"]
        if not isinstance(z, np.ndarray) or z.dtype != np.float32 or z.shape != (n, h, w, 3):
            raise ValueError(f"EmotionVideo: draw's noise must be float32 [{n},{h},{w},3], got {getattr(z, 'shape', None)}")


class EmotionVideo:
    """A lazy stand-in for the reference's ``transformed_video`` after its cyclic extension (demo.py:490-502): ``ev[t0:t1]`` is
    [t1-t0,3,256,256] float32 on the device, output frame t from source frame t mod N, computed on the CURRENT stream by one
    ``eamm_op_emotion_augment`` launch.  Works as ``emotion_frames=`` of ``animate_from_features`` / ``animate_from_audio``: the
    streamed pipeline asks for ``front_batch`` frames at a time on its front stream, so the whole [T,3,256,256] never exists.

    Construction uploads the frames, resizes and aligns them (``align_video``) and draws the clip's augmentation
    (``draw_augmentation``: ``seed`` for the seeded draw with device noise; else the reference-order draw from ``py_random`` /
    ``np_random``, by default the global ``random`` / ``np.random``, as the demo does; or a given ``draw`` dict of that form).  ``params``: the config's
    ``augmentation_params`` (default ``emotion_augmentation_config()``).  Any split of a span into slices gives the same values,
    bit for bit.  ``len(ev)`` is N, the source frames."""

    def __init__(self, frames, landmarks=None, *, emotion: Optional[str] = None, params=None, seed: Optional[int] = None,
                 py_random=None, np_random=None, draw: Optional[dict] = None, device=None):
        self.params = check_augmentation_params(params)
        self._raw_params = params
        f = _frames_u8(frames, "EmotionVideo")
        self.n_frames = n = int(f.shape[0])
        if landmarks is not None:
            _landmark_array(landmarks, n, ALIGN_POINTS, "EmotionVideo")
        self.device = _device(device, f)
        self.draw = draw if draw is not None else draw_augmentation(n, seed=seed, py_random=py_random, np_random=np_random,
                                                                    params=params)
        _check_draw(self.draw, n, self.params)
        self.aligned = align_video(f, landmarks, emotion, self.device)
        self._rot = (C.c_double * 6)(*rotation_matrix(self.draw["angle"]).reshape(6))
        _, hinv = perspective_params(self.draw["pers"], self.draw["enlarge"])
        self._hinv_host = hinv
        self._hinv = torch.from_numpy(np.ascontiguousarray(hinv.reshape(n, 9))).to(self.device)
        self._noise = torch.from_numpy(self.draw["noise"]).to(self.device) if "noise" in self.draw else None
        self._ready = None
        if self.device.type == "cuda":
            self._ready = torch.cuda.Event()
            self._ready.record(torch.cuda.current_stream(self.device))

    def __len__(self) -> int:
        return self.n_frames

    @property
    def shape(self):
        return (self.n_frames, 3, OUT, OUT)

    def __getitem__(self, idx) -> torch.Tensor:
        if isinstance(idx, slice):
            if idx.step not in (None, 1):
                raise ValueError("EmotionVideo: only contiguous spans (step 1)")
            t0 = 0 if idx.start is None else int(idx.start)
            t1 = self.n_frames if idx.stop is None else int(idx.stop)
            if t0 < 0 or t1 < t0:
                raise ValueError(f"EmotionVideo: a span t0:t1 with 0 <= t0 <= t1, got {t0}:{t1}")
            return self._frames(t0, t1)
        t = int(idx)
        if t < 0:
            raise ValueError(f"EmotionVideo: frame indices are >= 0 (they wrap modulo N), got {t}")
        return self._frames(t, t + 1)[0]

    def materialize(self, T: Optional[int] = None) -> torch.Tensor:
        """The whole transformed video of a T-frame clip: [T,3,256,256] (T default N)."""
        return self[0:self.n_frames if T is None else int(T)]

    def _frames(self, t0: int, t1: int) -> torch.Tensor:
        if self.device.type != "cuda":
            return torch.from_numpy(augment_reference(self.aligned.numpy(), self.draw, self._raw_params, t0, t1))
        from . import _op
        dev = self.device
        out = torch.empty((t1 - t0, 3, OUT, OUT), dtype=torch.float32, device=dev)
        if t1 == t0:
            return out
        stream = torch.cuda.current_stream(dev)
        stream.wait_event(self._ready)
        for t in (self.aligned, self._hinv, self._noise):
            if t is not None:
                t.record_stream(stream)
        x0, y0, w, h = self.params["mouth"]
        for a in range(t0, t1, MAX_LAUNCH):
            b = min(t1, a + MAX_LAUNCH)
            _op.call("emotion_augment", dev, self.aligned, self.n_frames, a, b - a, int(self.draw["flip"]), self._rot, self._hinv,
                     self._noise, self.draw.get("noise_seed", 0), x0, y0, w, h, out[a - t0:b - t0], stream=stream)
        return out
