"""Shared by the audio-bank tests: an independent numpy restatement of how the reference's data set cuts the audio window of a
sample, the test bank with its case list, and the float64 references, computed once.

The reference's data set class (dataloader/aff2compdataset.py) cannot be imported here - it needs lmdb, cv2 and torchaudio -, so the
assembler's parity is unpinned by a reference fixture; it is held to this restatement of the cited lines instead:

  audio = torchaudio.load(audio_file,
            num_frames=min(sample_len_frames, max(int((time_stamps[index] / 1000) * sample_rate),
                                                  int(window_size * sample_rate))),                    (aff2compdataset.py:218-223)
            offset=max(int((time_stamps[index] / 1000) * sample_rate - sample_len_frames + audio_shift_samples), 0))  (:224-226)
  try: audio_features = audio_transform(audio)                                                          (:227-228)
  except: audio = torch.zeros(1, sample_len_frames); audio_features = audio_transform(audio)            (:229-232)
  if audio.shape[1] < sample_len_frames: features right-aligned in int(sample_len_secs / window_stride + 1) zero columns  (:234-238)
  audio_features = audio_spec_transform(audio_features)                                                 (:240-241)
  if audio.shape[1] < sample_len_frames: audio right-aligned in sample_len_frames zeros                 (:243-246)

``load(offset, num_frames)`` is ``wav[offset : offset + num_frames]`` (a load past the end of the file returns what is there).
The transform raises where torch's reflect padding does: for a clip of at most n_fft / 2 samples.  ``offset``'s ``int()`` is taken
of the float expression as the reference writes it; sample_len_frames and audio_shift_samples are integers far below 2^53, so it
equals ``E - N + shift`` with ``E = int((time_stamps[index] / 1000) * sample_rate)`` whenever the result is positive, and the
``max(.., 0)`` hides the difference where it is not.  Two points are this project's own definitions and not the reference's: an
absent wav and an ``index`` outside ``[0, F)`` give silence.

The test waveforms are the ``_wave`` family of audio_util.py rounded to the int16 grid (x * 2**-15), so that ONE set of float64
references serves the fp32 bank and the int16 bank."""
import functools

import numpy as np
import torch

from audio_util import KEEP_REL, _wave, mel_power_f64
from oracle.audio_front_end import mel_features

SAMPLE_RATE, WINDOW_SIZE, WINDOW_STRIDE = 44100, 20e-3, 10e-3
SAMPLE_LEN_SECS, SHIFT_SECS = 1, 0.5                     # N = 44100, full = 101, shift = 22050
N, W, SHIFT, HOP, HALF, FULL = 44100, 882, 22050, 441, 512, 101
WAV_LENGTHS = (100000, 30000, 400, 0)                    # longer than N; shorter than N; never audible; absent

# (wav, end_sample) of every sample of the test data set; CASES names what each one is there for
SAMPLES = (
    (0, 441),        # E < w: num = w
    (0, 60000),      # got == N exactly
    (0, 100000),     # cut by EOF: off = 77950, got = 22050
    (0, 121537),     # off = 99487: got = 513, the shortest audible window
    (0, 121538),     # got = 512: silent
    (0, 4409), (0, 4410), (0, 4411),   # a hop multiple and its neighbours
    (1, 60000),      # off = 37950 >= L = 30000: got = 0
    (1, 25000),      # the short wav, whole window inside
    (1, 40000),      # the short wav, cut by EOF: off = 17950, got = 12050
    (2, 3000),       # the 400-sample wav: got = 400
    (3, 30000),      # the absent wav
    (0, 30001),      # odd offsets and lengths: num = 30001, off = 7951
)
F = len(SAMPLES)
INDEX = tuple(range(F)) + (-1, F)                        # every sample, then the two indices outside the data set


def time_stamps_ms() -> np.ndarray:
    """float64 [F]: time stamps with fractional milliseconds whose int((ts / 1000) * sample_rate) is SAMPLES' end_sample"""
    ts = np.array([(e + 0.5) / (SAMPLE_RATE / 1000) for _, e in SAMPLES], dtype=np.float64)
    for t, (_, e) in zip(ts.tolist(), SAMPLES):
        assert int((t / 1000) * SAMPLE_RATE) == e, (t, e)
    return ts


@functools.lru_cache(maxsize=None)
def waves_i16():
    """the test wavs as int16 tensors"""
    gains = (1.0, 0.3, 1.0, 1.0)
    return tuple(torch.round(_wave(n, 3 + v, gains[v]) * 32768.0).clamp(-32768, 32767).to(torch.int16)
                 for v, n in enumerate(WAV_LENGTHS))


def waves_f32():
    return tuple(x.to(torch.float32) * 2.0 ** -15 for x in waves_i16())


def reference_window(wav: np.ndarray, time_stamp_ms: float):
    """(audio float [N], clip or None): ``audio`` as ``get_audio_feature`` returns it, and the samples its transform ran on (None:
    the transform raised and ran on N zeros)"""
    sample_len_frames = SAMPLE_LEN_SECS * SAMPLE_RATE
    audio_shift_samples = SHIFT_SECS * SAMPLE_RATE
    num_frames = min(sample_len_frames, max(int((time_stamp_ms / 1000) * SAMPLE_RATE), int(WINDOW_SIZE * SAMPLE_RATE)))
    offset = max(int((time_stamp_ms / 1000) * SAMPLE_RATE - sample_len_frames + audio_shift_samples), 0)
    audio = wav[offset:offset + num_frames]
    clip = audio
    try:
        if len(audio) <= HALF:
            raise ValueError("reflect padding needs more samples than it adds")
    except ValueError:
        audio, clip = np.zeros(sample_len_frames, dtype=wav.dtype), None
    if len(audio) < sample_len_frames:
        _audio = np.zeros(sample_len_frames, dtype=wav.dtype)
        _audio[-len(audio):] = audio
        audio = _audio
    return audio, clip


def reference_table(index=INDEX) -> np.ndarray:
    """int64 [B, 2]: (offset into the concatenated wavs, got) of every window the loop transforms, (-1, 0) for a silent one"""
    wavs = [x.numpy() for x in waves_f32()]
    starts = np.cumsum((0,) + WAV_LENGTHS[:-1])
    ts = time_stamps_ms()
    table = np.empty((len(index), 2), dtype=np.int64)
    for b, i in enumerate(index):
        table[b] = (-1, 0)
        if i < 0 or i >= F:                               # this project's definition: silent
            continue
        v = SAMPLES[i][0]
        if WAV_LENGTHS[v] == 0:                           # this project's definition: silent
            continue
        _, clip = reference_window(wavs[v], float(ts[i]))
        if clip is not None:
            offset = max(int((float(ts[i]) / 1000) * SAMPLE_RATE - N + SHIFT), 0)
            table[b] = (starts[v] + offset, len(clip))
    return table


def assert_cases_present() -> None:
    """every case the tests are about is in the table: a changed constant cannot silently drop one"""
    table = reference_table()
    got = {i: int(table[b, 1]) for b, i in enumerate(INDEX)}
    raw = {}                                              # got before the audibility test, by the rule's integers
    for i, (v, e) in enumerate(SAMPLES):
        off = max(e - N + SHIFT, 0)
        raw[i] = (e, off, max(0, min(min(N, max(e, W)), WAV_LENGTHS[v] - off)), WAV_LENGTHS[v])
    has = lambda pred: any(pred(i, *raw[i]) for i in range(F))
    assert has(lambda i, e, off, g, L: e < W and got[i] == W), "E < w"
    assert has(lambda i, e, off, g, L: got[i] == N), "got == N"
    assert has(lambda i, e, off, g, L: L >= N and HALF < got[i] < min(N, e) and off + g == L), "cut by EOF"
    for want in (513, 4409, 4410, 4411):
        assert has(lambda i, e, off, g, L: got[i] == want), want
    assert has(lambda i, e, off, g, L: g == 512 and got[i] == 0), "got == 512 is silent"
    assert has(lambda i, e, off, g, L: L > 0 and off >= L and got[i] == 0), "off >= L"
    assert has(lambda i, e, off, g, L: L == 400 and g == 400 and got[i] == 0), "the 400-sample wav"
    assert has(lambda i, e, off, g, L: L == 0 and got[i] == 0), "the absent wav"
    assert INDEX[-2:] == (-1, F) and table[-2:].tolist() == [[-1, 0], [-1, 0]], "index -1 and F"
    assert has(lambda i, e, off, g, L: 0 < L < N and got[i] > HALF), "a wav shorter than N"


@functools.lru_cache(maxsize=None)
def reference_batch():
    """(audio float32 [B, 1, N], power [B] of float64 [n_mels, frames] or None, features float64 [B, n_mels, FULL]) of INDEX: the
    float64 route, every window at its own length"""
    import avformer_amd as A
    fe = A.audio.MelFrontEnd(sample_len_secs=SAMPLE_LEN_SECS)
    wavs = [x.numpy() for x in waves_f32()]
    ts = time_stamps_ms()
    audio = np.zeros((len(INDEX), 1, N), dtype=np.float32)
    power, feats = [], np.empty((len(INDEX), fe.n_mels, FULL))
    silent = mel_features(np.zeros(N), sample_len_secs=SAMPLE_LEN_SECS)
    for b, i in enumerate(INDEX):
        clip = None
        if 0 <= i < F and WAV_LENGTHS[SAMPLES[i][0]] > 0:
            audio[b, 0], clip = reference_window(wavs[SAMPLES[i][0]], float(ts[i]))
        power.append(None if clip is None else mel_power_f64(clip, fe))
        feats[b] = silent if clip is None else mel_features(clip, sample_len_secs=SAMPLE_LEN_SECS)
    return audio, tuple(power), feats


def kept_share(ref: np.ndarray) -> float:
    """the share of bins of a float64 mel power that assert_mel_power_close keeps"""
    return float((ref > KEEP_REL * np.abs(ref).max()).mean())


def make_bank(dtype=torch.float32):
    import avformer_amd as A
    waves = waves_i16() if dtype == torch.int16 else waves_f32()
    return A.audio_bank.AudioBank.from_waves(waves, [v for v, _ in SAMPLES], time_stamps_ms(), SAMPLE_RATE)


def check_against_float64(power, feats, what="") -> None:
    """power / feats [B, 1, n_mels, FULL] of INDEX against reference_batch, clip by clip with audio_util's bounds"""
    from audio_util import assert_features_close, assert_mel_power_close
    _, ref_power, ref_feats = reference_batch()
    for b, i in enumerate(INDEX):
        tag = f"{what} index {i}"
        p = power[b, 0].detach().cpu()
        if ref_power[b] is None:
            assert not p.any(), tag
        else:
            frames = ref_power[b].shape[1]
            assert not p[:, :FULL - frames].any(), tag
            assert_mel_power_close(p[:, FULL - frames:], ref_power[b], tag)
        assert_features_close(feats[b, 0], ref_feats[b], tag)
