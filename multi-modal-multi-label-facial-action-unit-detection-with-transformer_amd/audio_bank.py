"""Audio windows assembled from a resident waveform bank: the last host stage of the audio stream, on the device.

The reference's data set cuts the audio of a sample out of the video's wav by its time stamp, on the host
(dataloader/aff2compdataset.py:214-247; testset.py:164-198 repeats it).  With ``N = sample_len_secs * sample_rate`` (55, 441000),
``w = int(window_size * sample_rate)`` (882), ``shift = audio_shift_secs * sample_rate`` (57; opts.py:39, default 5 s),
``hop = 441``, ``half = n_fft / 2 = 512`` and ``full = int(sample_len_secs / window_stride + 1)`` (1001), for sample ``i`` with
``E = end_sample[i] = int((time_stamps[i] / 1000) * sample_rate)`` whose wav has ``L`` samples:

  * ``num = min(N, max(E, w))``: ``torchaudio.load(num_frames=...)``                                              (220-223)
  * ``off = max(E - N + shift, 0)``: ``torchaudio.load(offset=...)``                                              (224-226)
  * ``got = max(0, min(num, L - off))``: a load past the end of the file returns what is there
  * ``got > half``: the clip is ``wav[off : off + got]``.  It has ``1 + got // hop`` (<= ``full``) frames of mel power, computed
    on exactly those samples, with the reflect padding at THEIR ends (228); they are right-aligned in ``full`` columns, the
    columns in front are 0, before the dB conversion (234-241).  ``audio`` is the same samples right-aligned in ``N`` zeros
    (243-246).
  * ``got <= half`` (``got == 0`` included): the transform raises - reflect padding needs more than ``half`` samples - and the
    ``except`` replaces the clip by ``N`` zeros (227-232): all ``full`` columns are 0 power, every output is
    ``(-100 - mean) / std``, and ``audio`` is all zeros.

Zero-padding a short window to ``N`` samples first is NOT this transform: the frames that straddle the start of the audio differ.

This project's definitions, not the reference's (which would raise before its ``try``; nothing on the device can): a sample whose
wav is absent (``L == 0``) takes the silent case, and so does an ``index`` outside ``[0, F)``.

Neighbouring samples share all but about 1/30 s of their 10 s, so a host-assembled batch carries almost every sample again each
step (64 windows: 113 MB of fp32).  Here the waveforms stay on the device as one 1-D tensor - the bank, fp32 or int16 - and only
``index [B]`` travels per step.  ``E`` is computed once on the host in float64 when the bank is built (NumPy float64 is the
arithmetic of the reference's Python floats; ``int()`` truncates toward zero); the device sees integers only.

``backend="torch"`` (default) is the definition on any device: the window table is read on the host and the torch path of the
front end's transform runs once per distinct length.  ``backend="hip"`` is one launch of csrc/mel_bank.hip per method (plus the
existing dB launch for ``features``), with ``index`` read by the kernel: no host synchronisation, capturable.

Parity: unpinned by a reference fixture (the data set class needs lmdb, cv2 and torchaudio, which are not importable here);
checked against an independent numpy restatement of the cited lines (tests/audio_bank_util.py).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch
from torch import nn

from . import ops
from .audio import MelFrontEnd

BACKENDS = ("torch", "hip")
WAVE_DTYPES = (torch.float32, torch.int16)
INT16_SCALE = 2.0 ** -15   # an int16 sample x is worth x * 2**-15 (exact in fp32): the loader's documented normalisation


def end_samples(time_stamps_ms, sample_rate: int) -> np.ndarray:
    """int64 [F]: ``int((time_stamps[i] / 1000) * sample_rate)`` in float64, truncated toward zero (aff2compdataset.py:222)"""
    ts = np.asarray(time_stamps_ms, dtype=np.float64)
    return np.trunc((ts / 1000) * sample_rate).astype(np.int64)


class AudioBank:
    """The waveforms of a data set split on one device: ``wave`` fp32 / int16 [total] (the wavs one after the other),
    ``wav_start`` / ``wav_len`` int64 [V] (where wav v lies in ``wave``; a length of 0 is an absent wav), ``wav_of`` int32 [F] (the
    wav of every sample - not ``video_db_nr``: the ``_left`` / ``_right`` videos share one wav, testset.py:166) and ``end_sample``
    int64 [F].  All contiguous, all on the device of ``wave``."""

    def __init__(self, wave: torch.Tensor, wav_start: torch.Tensor, wav_len: torch.Tensor, wav_of: torch.Tensor,
                 end_sample: torch.Tensor):
        if not torch.is_tensor(wave) or wave.dtype not in WAVE_DTYPES or wave.dim() != 1 or wave.numel() < 1:
            raise ValueError("wave must be a 1-D fp32 or int16 tensor with at least one sample")
        if not torch.is_tensor(wav_start) or wav_start.dtype != torch.int64 or wav_start.dim() != 1 or wav_start.numel() < 1:
            raise ValueError("wav_start must be an int64 tensor [V] with V >= 1")
        V = wav_start.numel()
        if not torch.is_tensor(wav_len) or wav_len.dtype != torch.int64 or tuple(wav_len.shape) != (V,):
            raise ValueError(f"wav_len must be an int64 tensor [{V}]")
        if not torch.is_tensor(wav_of) or wav_of.dtype != torch.int32 or wav_of.dim() != 1 or wav_of.numel() < 1:
            raise ValueError("wav_of must be an int32 tensor [F] with F >= 1")
        F = wav_of.numel()
        if not torch.is_tensor(end_sample) or end_sample.dtype != torch.int64 or tuple(end_sample.shape) != (F,):
            raise ValueError(f"end_sample must be an int64 tensor [{F}]")
        tensors = (("wave", wave), ("wav_start", wav_start), ("wav_len", wav_len), ("wav_of", wav_of), ("end_sample", end_sample))
        for name, t in tensors:
            if t.device != wave.device:
                raise ValueError(f"{name} is on {t.device}, the waveforms on {wave.device}")
        for name, t in tensors:
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if bool(((wav_start < 0) | (wav_len < 0) | (wav_start > wave.numel()) | (wav_len > wave.numel() - wav_start)).any()):
            raise ValueError(f"wav_start + wav_len must lie inside wave ({wave.numel()} samples)")
        if bool(((wav_of < 0) | (wav_of >= V)).any()):
            raise ValueError(f"wav_of must lie in [0, {V})")
        self.wave, self.wav_start, self.wav_len, self.wav_of, self.end_sample = wave, wav_start, wav_len, wav_of, end_sample

    @classmethod
    def from_waves(cls, waves: Sequence[torch.Tensor], wav_of, time_stamps_ms, sample_rate: int = 44100) -> "AudioBank":
        """``waves``: 1-D tensors of one dtype (an empty one is an absent wav), ``wav_of`` [F] the wav of every sample,
        ``time_stamps_ms`` [F] the data set's time stamps"""
        if len(waves) < 1 or any(not torch.is_tensor(x) or x.dim() != 1 for x in waves):
            raise ValueError("waves must be a non-empty sequence of 1-D tensors")
        if any(x.dtype != waves[0].dtype or x.device != waves[0].device for x in waves):
            raise ValueError("the waveforms must have one dtype and one device")
        device = waves[0].device
        lens = torch.tensor([x.numel() for x in waves], dtype=torch.int64)
        starts = torch.cumsum(lens, 0) - lens
        wave = torch.cat(list(waves)) if int(lens.sum()) > 0 else torch.zeros(1, dtype=waves[0].dtype, device=device)
        wav_of = torch.as_tensor(np.asarray(wav_of), dtype=torch.int32)
        end = torch.from_numpy(end_samples(time_stamps_ms, sample_rate))
        return cls(wave.contiguous(), starts.to(device), lens.to(device), wav_of.to(device), end.to(device))

    def __len__(self) -> int:
        return self.wav_of.numel()

    @property
    def device(self) -> torch.device:
        return self.wave.device

    @property
    def n_wavs(self) -> int:
        return self.wav_start.numel()

    def to(self, device) -> "AudioBank":
        return AudioBank(self.wave.to(device), self.wav_start.to(device), self.wav_len.to(device), self.wav_of.to(device),
                         self.end_sample.to(device))


class AudioAssembler(nn.Module):
    """The audio windows of ``index`` int64 [B] out of an ``AudioBank``, by the rule of the module docstring, for the transform of
    ``front_end`` (a ``MelFrontEnd``: its ``sample_len_frames``, ``win_length``, ``hop_length``, ``n_fft`` and ``full_frames``).

    ``window_table(bank, index, front_end)`` -> int64 [B, 2]: the window's offset into ``bank.wave`` and ``got``, or ``(-1, 0)``
    for a silent one.  Plain torch, any device.
    ``forward(bank, index, front_end)`` -> ``audio`` fp32 [B, 1, N]: the window right-aligned in zeros.
    ``mel_power(bank, index, front_end)`` -> fp32 [B, 1, n_mels, full]: mel power, every window transformed at its own length.
    ``features(bank, index, front_end)`` -> fp32 [B, 1, n_mels, full]: the tensor ``data['audio_features']`` holds.

    ``backend="torch"`` (default): the table is read on the host, the torch transform runs once per distinct length.
    ``backend="hip"``: one launch of csrc/mel_bank.hip per method (``features``: plus the dB launch of csrc/mel.hip); the bank must
    be on the GPU (no CPU fallback) and ``front_end`` a ``MelFrontEnd(backend="hip")``; under ``no_grad``; ``index`` is read on
    the device.  ``forward`` gives the same bits on both; ``mel_power`` / ``features`` rows are those of ``front_end`` on the
    window's own samples."""

    def __init__(self, audio_shift_secs: int = 5, backend: str = "torch"):
        super().__init__()
        if backend not in BACKENDS:
            raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
        if isinstance(audio_shift_secs, bool) or not isinstance(audio_shift_secs, (int, float)) or audio_shift_secs < 0:
            raise ValueError(f"audio_shift_secs must be a number of at least 0, got {audio_shift_secs!r}")
        self.audio_shift_secs, self.backend = audio_shift_secs, backend

    def _rule(self, front_end: MelFrontEnd):
        """(N, w, shift, half, hop, full) of the rule, integers"""
        N = int(front_end.sample_len_frames)
        shift = int(self.audio_shift_secs * front_end.sample_rate)                               # aff2compdataset.py:57
        full = front_end.full_frames
        if full < 1 + N // front_end.hop_length:
            raise ValueError(f"a window of {N} samples has {1 + N // front_end.hop_length} frames, full_frames is {full}")
        return N, front_end.win_length, shift, front_end.n_fft // 2, front_end.hop_length, full

    def _check(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd, table_only: bool = False) -> None:
        if not isinstance(bank, AudioBank):
            raise ValueError(f"bank must be an AudioBank, got {type(bank).__name__}")
        if not isinstance(front_end, MelFrontEnd):
            raise ValueError(f"front_end must be a MelFrontEnd, got {type(front_end).__name__}")
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1:
            raise ValueError("index must be an int64 tensor [B] with B >= 1")
        if index.device != bank.device:
            raise ValueError(f"index is on {index.device}, the bank on {bank.device}")
        if table_only:
            return
        if front_end.window.device != bank.device:
            raise ValueError(f"the front end is on {front_end.window.device}, the bank on {bank.device}")
        if self.backend == "hip":
            if not bank.wave.is_cuda:
                raise RuntimeError("AudioAssembler (HIP) needs its bank on the MI355X; there is no CPU fallback - "
                                   "use backend='torch' on the host")
            if front_end.backend != "hip":
                raise ValueError("AudioAssembler (HIP) runs the transform in its own launch: front_end must be "
                                 "MelFrontEnd(backend='hip')")

    def window_table(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd) -> torch.Tensor:
        self._check(bank, index, front_end, table_only=True)
        N, w, shift, half, _, _ = self._rule(front_end)
        ok = (index >= 0) & (index < len(bank))
        i = torch.where(ok, index, torch.zeros_like(index))
        E, v = bank.end_sample[i], bank.wav_of[i].to(torch.int64)
        L, start = bank.wav_len[v], bank.wav_start[v]
        num = torch.clamp(torch.clamp(E, min=w), max=N)                                          # aff2compdataset.py:220-223
        off = torch.clamp(E - N + shift, min=0)                                                  # :224-226
        got = torch.clamp(torch.minimum(num, L - off), min=0)
        ok = ok & (got > half)                                                                   # :227-232
        return torch.stack([torch.where(ok, start + off, torch.full_like(off, -1)), torch.where(ok, got, torch.zeros_like(got))], 1)

    def _windows(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd):
        """the table on the host, grouped by length: [(got, rows, offsets)]"""
        table = self.window_table(bank, index, front_end).cpu()
        groups = {}
        for b, (first, got) in enumerate(table.tolist()):
            if got > 0:
                groups.setdefault(got, []).append((b, first))
        return [(got, [b for b, _ in rows], [f for _, f in rows]) for got, rows in sorted(groups.items())]

    def _clips(self, bank: AudioBank, got: int, offsets) -> torch.Tensor:
        """fp32 [len(offsets), got]: the windows of one length"""
        x = torch.stack([bank.wave[f:f + got] for f in offsets])
        return x.to(torch.float32) * INT16_SCALE if x.dtype == torch.int16 else x

    def _torch_audio(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd) -> torch.Tensor:
        N = self._rule(front_end)[0]
        audio = torch.zeros(index.numel(), 1, N, dtype=torch.float32, device=bank.device)
        for got, rows, offsets in self._windows(bank, index, front_end):
            audio[rows, 0, N - got:] = self._clips(bank, got, offsets)                           # aff2compdataset.py:243-246
        return audio

    def _torch_power(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd) -> torch.Tensor:
        full = self._rule(front_end)[5]
        mel = torch.zeros(index.numel(), 1, front_end.n_mels, full, dtype=torch.float32, device=bank.device)
        for got, rows, offsets in self._windows(bank, index, front_end):
            p = front_end.mel_power(self._clips(bank, got, offsets))                             # [rows, n_mels, 1 + got // hop]
            mel[rows, 0, :, full - p.shape[-1]:] = p                                             # aff2compdataset.py:234-238
        return mel

    def _hip_power(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd, normalise: bool) -> torch.Tensor:
        N, _, shift, _, hop, full = self._rule(front_end)
        with torch.no_grad():
            mel, peak = ops.mel_power_bank(bank.wave, bank.wav_start, bank.wav_len, bank.wav_of, bank.end_sample, index.contiguous(),
                                           N, shift, front_end.window, front_end.fb, front_end.bin_lo, front_end.bin_hi,
                                           front_end.n_fft, hop, full)
            if normalise:
                ops.mel_db_norm(mel, peak, 1, front_end.top_db, front_end.mean, front_end.std)
        return mel.unsqueeze(1)

    def forward(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd) -> torch.Tensor:
        self._check(bank, index, front_end)
        if self.backend != "hip":
            return self._torch_audio(bank, index, front_end)
        N, w, shift, _, _, _ = self._rule(front_end)
        with torch.no_grad():
            return ops.wave_gather(bank.wave, bank.wav_start, bank.wav_len, bank.wav_of, bank.end_sample, index.contiguous(), N, w,
                                   shift).unsqueeze(1)

    def mel_power(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd) -> torch.Tensor:
        self._check(bank, index, front_end)
        if self.backend == "hip":
            return self._hip_power(bank, index, front_end, False)
        return self._torch_power(bank, index, front_end)

    def features(self, bank: AudioBank, index: torch.Tensor, front_end: MelFrontEnd) -> torch.Tensor:
        self._check(bank, index, front_end)
        if self.backend == "hip":
            return self._hip_power(bank, index, front_end, True)
        return front_end.db_norm(self._torch_power(bank, index, front_end))
