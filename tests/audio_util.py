"""Shared by the audio front-end tests: the test signal family of test_gpu_audio.py, a float64 restatement of the mel POWER
spectrogram (hand-cut frames, numpy.fft.rfft, the module's own filterbank in float64) and the front-end's tolerances:

  * mel power: 2e-5 of the clip's largest value (test_audio_cpu.py::test_mel_power_against_a_third_party_implementation);
  * 0.02 dB on the bins above 1e-6 of that maximum, which must be at least 99 % of all bins;
  * 2e-3 absolute on the normalised output (one unit = 19.9 dB).

The fp32 torch backend, on the inputs of test_gpu_audio_hip.py, lies within 3.8e-7 / 6.1e-6 of float64 and keeps >= 99.86 % of
the bins: the bounds leave the existing path more than 50 x of room."""
import functools

import numpy as np
import torch

POWER_REL, DB_ABS, KEEP_REL, KEEP_SHARE, OUT_ABS = 2e-5, 0.02, 1e-6, 0.99, 2e-3


def _wave(n_samples, seed, gain=1.0, sample_rate=44100):
    """two tones plus 0.02 Gaussian noise (the family of test_gpu_audio.py), by length"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(int(n_samples)) / float(sample_rate)
    return gain * (0.3 * torch.sin(2 * torch.pi * 440.0 * t) + 0.1 * torch.sin(2 * torch.pi * (1000.0 + 500.0 * seed) * t + 1.0)
                   + 0.02 * torch.randn(t.numel(), generator=g))


def mel_power_f64(x, fe) -> np.ndarray:
    """waveform [samples] -> mel power [n_mels, 1 + samples // hop] in float64 with the parameters and the filterbank of `fe`"""
    x = np.asarray(x, dtype=np.float64)
    n_fft, win, hop = fe.n_fft, fe.win_length, fe.hop_length
    w = np.zeros(n_fft)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)      # periodic Hann, centred in the frame
    xp = np.pad(x, (n_fft // 2, n_fft // 2), mode="reflect")
    frames = 1 + len(x) // hop
    power = np.empty((n_fft // 2 + 1, frames))
    for t in range(frames):
        power[:, t] = np.abs(np.fft.rfft(xp[t * hop:t * hop + n_fft] * w)) ** 2
    return fe.fb.detach().cpu().double().numpy().T @ power


@functools.lru_cache(maxsize=None)
def wave_and_power(n_samples, seed, gain, fe_key):
    """(waveform, float64 mel power) of one test clip, computed once; fe_key = (sample_rate, n_mels) of a 20 ms / 10 ms front-end"""
    import avformer_amd as A
    fe = A.audio.MelFrontEnd(sample_rate=fe_key[0], n_mels=fe_key[1], sample_len_secs=1)
    x = _wave(n_samples, seed, gain, fe_key[0])
    return x, mel_power_f64(x.numpy(), fe)


def assert_mel_power_close(got, ref, what="", live=None):
    """got (tensor or array) against the float64 `ref`: POWER_REL of the maximum, DB_ABS on the kept bins, KEEP_SHARE kept.
    live: optional bool [n_mels], False for a filter without any non-zero weight (128 filters at 48 kHz: the lowest ones are
    narrower than a bin).  Such a row is zero by construction on both sides: it must be exactly zero, and it is left out of the
    kept share, which is about the bins that carry a value."""
    got = np.asarray(got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max()
    rel = np.abs(got - ref).max() / scale
    if live is not None:
        live = np.asarray(live, dtype=bool)
        assert not got[~live].any() and not ref[~live].any(), what
        got, ref = got[live], ref[live]
    keep = ref > KEEP_REL * scale
    db = np.abs(10 * np.log10(np.maximum(got, 1e-300)) - 10 * np.log10(np.maximum(ref, 1e-300)))[keep].max()
    print(f"{what}: mel power rel {rel:.3g}, dB on kept bins {db:.3g}, kept {keep.mean():.4f}")
    assert rel < POWER_REL, (what, rel)
    assert keep.mean() >= KEEP_SHARE, (what, keep.mean())
    assert db < DB_ABS, (what, db)


def assert_features_close(got, ref, what=""):
    got = np.asarray(got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref).max()
    print(f"{what}: normalised output max abs err {err:.3g}")
    assert err < OUT_ABS, (what, err)
