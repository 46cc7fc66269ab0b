"""CPU checks of the waveform front end (eamm_amd.audio_input): the float64 MFCC oracle against independent pieces, frame and
window counts (library and Python agree), the pose track of demo.py:test_auido, and read_wav."""
import ctypes
import wave

import numpy as np
import pytest
import scipy.fft
import torch

from eamm_amd import _lib, audio_input as ai, mfcc, mfcc_reference, mfcc_windows, prepare_pose, read_wav

EDGES = [0, 2, 4, 7, 10, 13, 16, 20, 24, 29, 34, 40, 46, 53, 60, 68, 77, 87, 97, 109, 122, 136, 152, 169, 188, 209, 231, 256]


def voiced(S, seed=0):
    rs = np.random.RandomState(seed)
    t = np.arange(S) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * 180 * t) + 0.1 * np.sin(2 * np.pi * 1230 * t) + 0.02 * rs.standard_normal(S)
    x[S // 3:S // 2] = 0.0
    return x.astype(np.float32)


def test_dct_equals_scipy():
    x = np.random.RandomState(1).standard_normal((5, 26))
    ours = x @ ai.dct_matrix().T
    np.testing.assert_allclose(ours, scipy.fft.dct(x, type=2, norm="ortho", axis=1)[:, :13], rtol=0, atol=1e-12)


def test_power_spectrum_equals_direct_dft():
    frames = ai.frames_of(voiced(3000), 1920)[[0, 5, 12, 20]]
    n = np.arange(400)[None, :]
    k = np.arange(257)[:, None]
    W = np.exp(-2j * np.pi * k * n / 512)                      # the zero-extended frame's 512-point DFT, O(N^2)
    direct = np.abs(frames @ W.T) ** 2 / 512
    got = ai.power_spectrum(frames)
    assert got.shape == direct.shape == (4, 257)
    assert np.abs(got - direct).max() <= 1e-12 * np.abs(direct).max()


def test_filterbank_edges_and_shape():
    assert ai.mel_edges().tolist() == EDGES
    fb = ai.mel_filterbank()
    assert fb.shape == (26, 257) and not fb[:, 256].any()
    assert fb[2, 7] == 1.0 and fb[2, 4] == 0.0 and fb[2, 10] == 0.0 and fb[2, 5] == pytest.approx(1 / 3)   # edges 4, 7, 10
    assert (np.count_nonzero(fb, axis=0)[1:256] <= 2).all()


def test_all_zero_signal():
    out = mfcc_reference(np.zeros(5000), pad=0)
    eps = np.finfo(np.float64).eps
    assert np.all(out[:, 0] == np.log(eps))
    row = (np.full(26, np.log(eps)) @ ai.dct_matrix().T) * (1 + 11 * np.sin(np.pi * np.arange(13) / 22))
    np.testing.assert_allclose(out[:, 1:], np.broadcast_to(row[1:], out[:, 1:].shape), rtol=0, atol=1e-12)


def test_pre_emphasis_and_framing():
    x = np.arange(1, 1001, dtype=np.float64)
    fr = ai.frames_of(x, pad=2)
    xp = np.concatenate([[0, 0], x, [0, 0]])
    y = np.concatenate([[xp[0]], xp[1:] - 0.97 * xp[:-1]])
    assert fr.shape == (ai.mfcc_frames(1000, 2), 400) == (5, 400)
    np.testing.assert_array_equal(fr[1], y[160:560])
    np.testing.assert_array_equal(fr[-1][:1004 - 640], y[640:])            # zero past L, not -0.97 * the last sample
    assert not fr[-1][1004 - 640:].any()


@pytest.mark.parametrize("pad", [0, 1920])
@pytest.mark.parametrize("S", [1, 399, 400, 401, 560, 720, 721, 16000])
def test_frame_counts(S, pad):
    L = S + 2 * pad
    want = 1 if L <= 400 else 1 + int(np.ceil((L - 400) / 160))
    assert ai.mfcc_frames(S, pad) == want
    assert _lib.lib().eamm_op_mfcc_frames(S, pad) == want
    assert mfcc_reference(np.ones(S), pad).shape == (want, 13)


def test_mfcc_entry_rejects_bad_arguments_without_a_launch():
    L = _lib.lib()
    buf = (ctypes.c_float * 16)()
    for n_samples, n_clips in ((0, 1), (10, 0)):
        assert L.eamm_op_mfcc(0, buf, n_samples, n_clips, 10, 0, buf, None) == _lib.ERR_ARG
        assert b"eamm_op_mfcc" in L.eamm_last_error(None)
    assert L.eamm_op_mfcc_frames(0, 0) == 0


def test_window_rows_and_count():
    F = 60
    m = torch.tensor([[100 * r + c for c in range(13)] for r in range(F)], dtype=torch.float32)[None]
    w = ai._windows(m)[0]
    assert w.shape == (F // 4 - 6, 28, 12)
    for t in range(w.shape[0]):                  # demo.py:326-333: ind = t + 3, rows (ind - 3) * 4 .. (ind + 4) * 4, columns 1:
        np.testing.assert_array_equal(w[t].numpy(), m[0, 4 * t:4 * t + 28, 1:].numpy())


def test_window_boundary_720_721():
    assert ai.min_window_samples(1920) == 721 and ai.mfcc_frames(720) == 27 and ai.mfcc_frames(721) == 28
    x = voiced(721)
    with pytest.raises(ValueError, match="721"):
        mfcc_windows(x[:720])
    w = mfcc_windows(x)
    assert w.shape == (1, 28, 12)
    np.testing.assert_allclose(w[0].numpy(), mfcc_reference(x)[:28, 1:].astype(np.float32), rtol=0, atol=0)


def test_cpu_mfcc_is_the_oracle_cast():
    x = voiced(4000)
    np.testing.assert_array_equal(mfcc(x).numpy(), mfcc_reference(x).astype(np.float32))
    b = np.stack([x, voiced(4000, seed=3)])
    got = mfcc(torch.from_numpy(b), pad=0)
    assert got.shape == (2, ai.mfcc_frames(4000, 0), 13)
    np.testing.assert_array_equal(got[1].numpy(), mfcc_reference(b[1], 0).astype(np.float32))


def test_waveform_errors():
    for bad in (np.zeros(1000, np.int16), torch.zeros(1000, dtype=torch.complex64), torch.zeros(2, 3, 1000), torch.zeros(0), [0.0] * 900):
        with pytest.raises(ValueError):
            mfcc_windows(bad)


def euro64(x, mincutoff=0.004, beta=0.7, dcutoff=1.0, freq=100.0):
    """filter1.OneEuroFilter over the rows as demo.py:302-306 applies it in place: the previous raw row IS the previous output."""
    te = 1.0 / freq
    alpha = lambda c: 1.0 / (1.0 + (1.0 / (2 * np.pi * c)) / te)
    out, edx = x.copy(), 0.0                     # row 0 passes through; the derivative filter starts from dx = 0
    for j in range(1, len(x)):
        dx = (x[j] - out[j - 1]) * freq
        edx = alpha(dcutoff) * dx + (1 - alpha(dcutoff)) * edx
        a = alpha(mincutoff + beta * np.abs(edx))
        out[j] = a * x[j] + (1 - a) * out[j - 1]
    return out


def test_pose_single_row_repeats_without_smoothing():
    p = np.arange(7, dtype=np.float64)[None] * 0.1
    out = prepare_pose(p, 250)
    assert out.shape == (250, 6) and out.dtype == torch.float32
    np.testing.assert_array_equal(out.numpy(), np.broadcast_to(p[:, :6].astype(np.float32), (250, 6)))
    assert prepare_pose(p.reshape(-1), 30).shape == (30, 6)


def test_pose_mirror_tiling():
    p = np.random.RandomState(2).uniform(-1, 1, (3, 7))
    out = prepare_pose(p, 10, smooth=False)
    # n = int((10 - 3) / 3 / 2) + 2 = 3: (0 1 2 2 1 0) x 3, cut to 10
    idx = [0, 1, 2, 2, 1, 0, 0, 1, 2, 2]
    np.testing.assert_array_equal(out.numpy(), p[idx, :6].astype(np.float32))


def test_pose_longer_and_equal():
    p = np.random.RandomState(3).uniform(-1, 1, (20, 6))
    np.testing.assert_array_equal(prepare_pose(p, 12, smooth=False).numpy(), p[:12].astype(np.float32))
    np.testing.assert_array_equal(prepare_pose(p, 20, smooth=False).numpy(), p.astype(np.float32))


def test_pose_smoothing_recurrence():
    p = np.random.RandomState(4).uniform(-0.3, 0.3, (40, 7))
    got = ai._one_euro_rows(p[:, :6], **ai.POSE_FILTER)
    assert np.abs(got - euro64(p[:, :6])).max() <= 1e-12
    np.testing.assert_array_equal(prepare_pose(p, 40).numpy(), got.astype(np.float32))
    assert np.abs(got - p[:, :6]).max() > 1e-3                      # it does smooth


def test_pose_long():
    start = np.array([[0.1, 0.2, 0.3, 1.0, 2.0, 3.0, 9.0]])
    long_ = np.random.RandomState(5).uniform(-1, 1, (15, 7))
    want = euro64((start + (long_ - long_[0]))[:, :6])
    np.testing.assert_allclose(prepare_pose(start, 15, pose_long=long_).numpy(), want.astype(np.float32), rtol=0, atol=0)


def write_wav(path, data, rate=16000):
    data = np.asarray(data, dtype=np.int16)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if data.ndim == 1 else data.shape[1])
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(data.astype("<i2").tobytes())


def test_read_wav_mono_and_stereo(tmp_path):
    rs = np.random.RandomState(6)
    mono = rs.randint(-32768, 32768, 1234)
    write_wav(tmp_path / "m.wav", mono)
    got = read_wav(tmp_path / "m.wav")
    assert got.dtype == np.float32 and got.shape == (1234,)
    np.testing.assert_array_equal(got, mono.astype(np.float32) / 32768)
    st = rs.randint(-32768, 32768, (999, 2))
    write_wav(tmp_path / "s.wav", st)
    got = read_wav(str(tmp_path / "s.wav"))
    assert got.shape == (999,)
    np.testing.assert_allclose(got, (st[:, 0] + st[:, 1]) / 65536.0, rtol=0, atol=1e-7)


def test_read_wav_refuses_other_rates(tmp_path):
    write_wav(tmp_path / "h.wav", np.zeros(100), rate=44100)
    with pytest.raises(ValueError, match="44100"):
        read_wav(tmp_path / "h.wav")


def test_against_python_speech_features_when_present():
    psf = pytest.importorskip("python_speech_features")
    x = voiced(20000).astype(np.float64)
    padded = np.concatenate([np.zeros(1920), x, np.zeros(1920)])
    np.testing.assert_allclose(mfcc_reference(x), psf.mfcc(padded, 16000, winstep=0.01), rtol=0, atol=1e-9)
