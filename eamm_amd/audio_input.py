"""From a waveform and a head-pose array to the audio network's inputs -- the reference's ``test_auido`` front end
(demo.py:286-354) -- and ``animate_from_audio``, the end-to-end call from what the demo takes (a 16 kHz recording, a pose array
and a portrait) to the clip's frames.

    reference (host)                                                    here
    ------------------------------------------------------------------  ------------------------------------------------------
    librosa.load(in_file, sr=16000)                    demo.py:314      read_wav (16-bit PCM at 16 kHz only: no resampling)
    speech padded with 1920 zeros on each side         demo.py:316-317  ``pad`` of the kernel (virtual zeros)
    python_speech_features.mfcc(speech, 16000,         demo.py:318      mfcc: eamm_op_mfcc (csrc/mfcc.hip) for a GPU tensor,
        winstep=0.01)                                                       mfcc_reference (float64 numpy) for a CPU one
    28-row windows of coefficients 1..12, every 4 rows demo.py:326-333  mfcc_windows (one strided copy)
    pose[:, :6], repeated / One-Euro smoothed, mirror-  demo.py:297-307, prepare_pose
        tiled or cut to T; smooth_pose(pose, pose_long)    335-341, 456-472
    audio_feature(example_image, input_mfcc, pose)     demo.py:352      animate_from_audio -> animate_from_features

``mfcc_reference`` is written from the algorithm (python_speech_features 0.6 / 0.6.1 with its defaults), not from the package:
pre-emphasis 0.97; 400-sample frames every 160 samples with a rectangular window, zero-filled past the signal's end; the power
spectrum |rfft(frame, 512)|^2 / 512; the frame energy (the sum of the 257 bins); 26 triangular mel filters over 0..8000 Hz on
integer bins; log; the orthonormal DCT-II keeping 13; the lifter 1 + 11 sin(pi n / 22); coefficient 0 replaced by log(energy).
An energy or filter sum of exactly 0 becomes DBL_EPSILON first.
"""
from __future__ import annotations

import wave

import numpy as np
import torch
import torch.distributed as dist

from .pipeline import animate_from_features

SAMPLE_RATE = 16000
FRAME, STEP, NFFT, NFILT, NCEP, LIFTER, PREEMPH = 400, 160, 512, 26, 13, 22, 0.97
DEMO_PAD = 1920                       # demo.py:316-317
WINDOW_ROWS, WINDOW_STEP, WINDOW_SKIP = 28, 4, 6   # input_mfcc windows: rows 4t .. 4t+27 of coefficients 1..12 (demo.py:326-333)
EPS = float(np.finfo(np.float64).eps)
# the reference's pose filter (demo.py:302)
POSE_FILTER = dict(mincutoff=0.004, beta=0.7, dcutoff=1.0, freq=100.0)


def _hz2mel(hz):
    return 2595.0 * np.log10(1.0 + hz / 700.0)


def _mel2hz(mel):
    return 700.0 * (10.0 ** (mel / 2595.0) - 1.0)


def mel_edges() -> np.ndarray:
    """The 28 integer bin edges of the 26 mel filters: floor((NFFT + 1) * mel2hz(linspace(hz2mel(0), hz2mel(8000), 28)) / 16000)."""
    mel = np.linspace(_hz2mel(0.0), _hz2mel(SAMPLE_RATE / 2), NFILT + 2)
    return np.floor((NFFT + 1) * _mel2hz(mel) / SAMPLE_RATE).astype(np.int64)


def mel_filterbank() -> np.ndarray:
    """[26, 257] float64: filter j rises as (i - b_j) / (b_j+1 - b_j) over [b_j, b_j+1) and falls as (b_j+2 - i) / (b_j+2 - b_j+1)
    over [b_j+1, b_j+2)."""
    b = mel_edges()
    fb = np.zeros((NFILT, NFFT // 2 + 1))
    for j in range(NFILT):
        for i in range(b[j], b[j + 1]):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(b[j + 1], b[j + 2]):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def dct_matrix() -> np.ndarray:
    """[13, 26] float64: the first 13 rows of the orthonormal DCT-II of length 26."""
    n = np.arange(NCEP)[:, None]
    m = np.arange(NFILT)[None, :]
    scale = np.where(n == 0, np.sqrt(1.0 / NFILT), np.sqrt(2.0 / NFILT))
    return scale * np.cos(np.pi * n * (2 * m + 1) / (2 * NFILT))


def lifter() -> np.ndarray:
    return 1.0 + (LIFTER / 2.0) * np.sin(np.pi * np.arange(NCEP) / LIFTER)


def mfcc_frames(n_samples: int, pad: int = DEMO_PAD) -> int:
    """F = 1 if L <= 400 else 1 + ceil((L - 400) / 160), L = n_samples + 2 pad (0 for an empty signal)."""
    if n_samples < 1:
        return 0
    L = int(n_samples) + 2 * int(pad)
    return 1 if L <= FRAME else 1 + -(-(L - FRAME) // STEP)


def min_window_samples(pad: int = DEMO_PAD) -> int:
    """Fewest samples that give one input_mfcc window (F >= 28): 721 with the demo's pad of 1920."""
    need = FRAME + (WINDOW_ROWS - 2) * STEP + 1            # L > 400 + 26 * 160 <=> ceil((L - 400) / 160) >= 27
    return max(1, need - 2 * int(pad))


def frames_of(signal: np.ndarray, pad: int = DEMO_PAD) -> np.ndarray:
    """[F, 400] float64: the pre-emphasised frames of the padded signal (zero past its end)."""
    x = np.concatenate([np.zeros(pad), np.asarray(signal, dtype=np.float64).reshape(-1), np.zeros(pad)])
    y = np.append(x[0], x[1:] - PREEMPH * x[:-1])
    F = mfcc_frames(len(signal), pad)
    y = np.concatenate([y, np.zeros((F - 1) * STEP + FRAME - len(y))]) if (F - 1) * STEP + FRAME > len(y) else y
    idx = np.arange(F)[:, None] * STEP + np.arange(FRAME)[None, :]
    return y[idx]


def power_spectrum(frames: np.ndarray) -> np.ndarray:
    """[F, 257]: |rfft(frame, 512)|^2 / 512."""
    return np.abs(np.fft.rfft(frames, NFFT, axis=-1)) ** 2 / NFFT


def mfcc_reference(signal, pad: int = DEMO_PAD) -> np.ndarray:
    """python_speech_features.mfcc(concat(zeros(pad), signal, zeros(pad)), 16000, winstep=0.01) in float64: [F, 13]."""
    signal = np.asarray(signal, dtype=np.float64).reshape(-1)
    if signal.size < 1:
        raise ValueError("mfcc_reference: the signal is empty")
    p = power_spectrum(frames_of(signal, pad))
    energy = p.sum(axis=1)
    energy = np.where(energy == 0, EPS, energy)
    feat = p @ mel_filterbank().T
    feat = np.where(feat == 0, EPS, feat)
    out = (np.log(feat) @ dct_matrix().T) * lifter()
    out[:, 0] = np.log(energy)
    return out


def _check_waveform(waveform, who: str):
    """-> (torch tensor [N,S] or [1,S], batched?) -- a ValueError for a wrong type, dtype, rank or an empty signal."""
    if isinstance(waveform, np.ndarray):
        if not (np.issubdtype(waveform.dtype, np.floating)):
            raise ValueError(f"{who}: the waveform must be floating point in [-1, 1], got numpy {waveform.dtype}")
        waveform = torch.from_numpy(np.ascontiguousarray(waveform))
    if not isinstance(waveform, torch.Tensor):
        raise ValueError(f"{who}: the waveform must be a torch tensor or a numpy array, got {type(waveform).__name__}")
    if not waveform.dtype.is_floating_point:
        raise ValueError(f"{who}: the waveform must be floating point in [-1, 1], got {waveform.dtype}")
    if waveform.dim() not in (1, 2):
        raise ValueError(f"{who}: the waveform must be [S] or [N,S], got {tuple(waveform.shape)}")
    batched = waveform.dim() == 2
    w = waveform if batched else waveform[None]
    if w.shape[0] < 1 or w.shape[1] < 1:
        raise ValueError(f"{who}: the waveform is empty ({tuple(waveform.shape)})")
    return w, batched


def _mfcc(w: torch.Tensor, pad: int) -> torch.Tensor:
    """[N,S] -> [N,F,13] float32 on w's device."""
    n, S = int(w.shape[0]), int(w.shape[1])
    if pad < 0:
        raise ValueError(f"mfcc: pad must be >= 0, got {pad}")
    if not w.is_cuda:
        rows = [mfcc_reference(w[i].detach().to(torch.float64).numpy(), pad) for i in range(n)]
        return torch.from_numpy(np.stack(rows).astype(np.float32))
    from . import _lib, _op
    x = w.detach().to(torch.float32).contiguous()
    F = int(_lib.lib().eamm_op_mfcc_frames(S, int(pad)))
    out = torch.empty((n, F, NCEP), device=x.device, dtype=torch.float32)
    _op.call("mfcc", x.device, x, S, n, S, int(pad), out)
    return out


def mfcc(waveform, pad: int = DEMO_PAD) -> torch.Tensor:
    """MFCC of a waveform [S] (-> [F,13]) or of N clips of equal length [N,S] (-> [N,F,13]), float32, each clip padded with
    ``pad`` zeros on each side (demo.py:316-318).  A GPU tensor runs ``eamm_op_mfcc`` on the current stream; a CPU tensor or a
    numpy array goes through ``mfcc_reference`` (float64) and is cast, on the CPU."""
    w, batched = _check_waveform(waveform, "mfcc")
    out = _mfcc(w, int(pad))
    return out if batched else out[0]


def _windows(m: torch.Tensor) -> torch.Tensor:
    """[N,F,13] MFCC -> [N,T,28,12] windows, T = F // 4 - 6: window t = rows 4t .. 4t+27, coefficients 1..12."""
    n, F = int(m.shape[0]), int(m.shape[1])
    T = F // WINDOW_STEP - WINDOW_SKIP
    m = m.contiguous()
    view = m.as_strided((n, T, WINDOW_ROWS, NCEP - 1), (F * NCEP, WINDOW_STEP * NCEP, NCEP, 1), m.storage_offset() + 1)
    return view.contiguous()


def _check_window_length(S: int, pad: int, who: str):
    if S < min_window_samples(pad):
        raise ValueError(f"{who}: {S} samples give no input_mfcc window with pad {pad}: at least {min_window_samples(pad)} samples "
                         f"are needed (28 MFCC rows)")


def mfcc_windows(waveform, pad: int = DEMO_PAD) -> torch.Tensor:
    """The reference's ``input_mfcc`` (demo.py:326-333): [T,28,12] for a waveform [S] ([N,T,28,12] for [N,S]), window t holding
    MFCC rows 4t .. 4t+27 and coefficients 1..12, T = F // 4 - 6.  A ValueError when T would be < 1 (fewer than 721 samples
    at the demo's pad of 1920)."""
    w, batched = _check_waveform(waveform, "mfcc_windows")
    _check_window_length(int(w.shape[1]), int(pad), "mfcc_windows")
    out = _windows(_mfcc(w, int(pad)))
    return out if batched else out[0]


def _one_euro_rows(pose: np.ndarray, mincutoff: float, beta: float, dcutoff: float, freq: float) -> np.ndarray:
    """filter1.OneEuroFilter.process applied row after row IN PLACE, as demo.py:302-306 does (``pose[j] = f.process(pose[j])``).

    The filter keeps a reference to the row it was given as its previous raw value, and the assignment then overwrites that row
    with the filtered one -- so the derivative of row j is taken against the FILTERED row j-1.  float64 throughout, in
    filter1.py:13-47's operation order."""
    out = np.array(pose, dtype=np.float64, copy=True)
    te = 1.0 / freq

    def alpha(cutoff):
        tau = 1.0 / (2 * np.pi * cutoff)
        return 1.0 / (1.0 + tau / te)

    prev = None              # x_filter's previous raw value == previous filtered row (aliased)
    edx = None               # dx_filter's previous filtered value
    for j in range(out.shape[0]):
        x = out[j].copy()
        dx = 0.0 if prev is None else (x - prev) * freq
        edx = dx if edx is None else alpha(dcutoff) * dx + (1.0 - alpha(dcutoff)) * edx
        cutoff = mincutoff + beta * np.abs(edx)
        s = x if prev is None else alpha(cutoff) * x + (1.0 - alpha(cutoff)) * prev
        out[j] = s
        prev = out[j].copy()
    return out


def _pose_rows(pose, who: str) -> np.ndarray:
    if isinstance(pose, torch.Tensor):
        pose = pose.detach().cpu().numpy()
    a = np.asarray(pose, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] not in (6, 7):
        if a.size == 0 or a.size % 7:
            raise ValueError(f"{who}: a pose array is [P,7], [P,6] or a flat multiple of 7 values, got {a.shape}")
        a = a.reshape(-1, 7)
    if a.shape[0] < 1:
        raise ValueError(f"{who}: the pose array is empty")
    return a[:, :6]


def prepare_pose(pose, steps: int, smooth: bool = True, pose_long=None) -> torch.Tensor:
    """The pose track of ``test_auido`` (demo.py:297-307, 335-341): float32 [steps, 6].

    ``pose``: [P,7], [P,6] or a flat array (reshaped to (-1,7)), columns 0..5 kept.  ``pose_long`` (demo.py:456-463,
    ``smooth_pose``): the track is first formed as pose[0] + (pose_long - pose_long[0]).  P == 1: the row is repeated 100 times and
    not smoothed; otherwise, with ``smooth``, One-Euro (mincutoff 0.004, beta 0.7, dcutoff 1, freq 100) row after row in float64.
    Then, when P < steps, (pose, pose[::-1]) is tiled int((steps - P) / P / 2) + 2 times; the result is cut to ``steps``."""
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"prepare_pose: steps must be >= 1, got {steps}")
    p = _pose_rows(pose, "prepare_pose")
    if pose_long is not None:                                    # demo.py:456-463
        long_ = _pose_rows(pose_long, "prepare_pose")
        p = p[:1] + (long_ - long_[:1])
    if len(p) == 1:
        p = np.repeat(p, 100, axis=0)
    elif smooth:
        p = _one_euro_rows(p, **POSE_FILTER)
    P = len(p)
    if P < steps:
        n = int((steps - P) / P / 2) + 2
        p = np.tile(np.concatenate((p, p[::-1]), axis=0), (n, 1))
    return torch.from_numpy(np.ascontiguousarray(p[:steps], dtype=np.float32))


def read_wav(path) -> np.ndarray:
    """16-bit PCM WAV at 16 kHz, mono or multi-channel (channels averaged, as librosa.load(mono=True) does) -> float32 [S],
    int16 / 32768.  Other rates and sample widths are refused: there is no resampling here."""
    with wave.open(str(path), "rb") as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if width != 2:
            raise ValueError(f"read_wav: {path}: {8 * width}-bit samples; only 16-bit PCM is read")
        if rate != SAMPLE_RATE:
            raise ValueError(f"read_wav: {path}: {rate} Hz; only {SAMPLE_RATE} Hz is read (resample the file first)")
        raw = f.readframes(n)
    x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768.0)
    x = x.reshape(-1, ch)
    return np.ascontiguousarray(x[:, 0] if ch == 1 else x.mean(axis=1, dtype=np.float32))


@torch.no_grad()
def animate_from_audio(generator, kp_detector, audio_feature, kp_detector_a, source_image, waveform, pose, *, smooth_pose: bool = True,
                       pose_long=None, audio_weight: float = 1.6, **kwargs):
    """The demo's whole path from a waveform: ``test_auido`` (demo.py:286-354) then ``make_animation_smooth`` (demo.py:194-282).

    ``waveform``: [S] float at 16 kHz (``read_wav``); ``pose``: the demo's pose array ([P,7], [P,6] or flat).  The MFCC windows are
    computed on the model's device (``mfcc_windows``, one launch plus one copy, before anything else of the clip), the pose track
    by ``prepare_pose(pose, T, smooth_pose, pose_long)``; then this returns exactly what
    ``animate_from_features(generator, kp_detector, audio_feature.decon, kp_detector_a, source_image, None,
    audio_feature=audio_feature, audio=windows, pose=pose_T, audio_weight=audio_weight, **kwargs)`` returns.  With
    ``return_keypoints`` the dict also holds ``mfcc`` [F,13].  Under a process group the ranks > 0 pass None for ``source_image``,
    ``waveform`` and ``pose`` (rank 0's inputs are broadcast)."""
    backend = kwargs.get("backend")
    dev = backend.device if backend is not None else next(generator.parameters()).device
    group = kwargs.get("group")
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    if waveform is None or pose is None:
        if waveform is not None or pose is not None or not (distributed and dist.get_rank(group) > 0):
            raise ValueError("animate_from_audio: waveform and pose are required (only ranks > 0 of a process group pass None)")
        return animate_from_features(generator, kp_detector, audio_feature.decon, kp_detector_a, source_image, None,
                                     audio_weight=audio_weight, **kwargs)
    w, batched = _check_waveform(waveform, "animate_from_audio")
    if batched:
        raise ValueError(f"animate_from_audio: one clip's waveform [S], got {tuple(waveform.shape)}")
    _check_window_length(int(w.shape[1]), DEMO_PAD, "animate_from_audio")
    m = _mfcc(w.to(dev, torch.float32), DEMO_PAD)
    windows = _windows(m)[0]
    pose_t = prepare_pose(pose, windows.shape[0], smooth=smooth_pose, pose_long=pose_long)
    res = animate_from_features(generator, kp_detector, audio_feature.decon, kp_detector_a, source_image, None,
                                audio_feature=audio_feature, audio=windows, pose=pose_t, audio_weight=audio_weight, **kwargs)
    if kwargs.get("return_keypoints"):
        res[2]["mfcc"] = m[0]
    return res

