"""CPU (no GPU needed): ``audio_bank.AudioBank`` / ``AudioAssembler(backend="torch")`` against the numpy restatement of the
reference's window rule (audio_bank_util.py) and, through it, against float64: the window table exactly, ``forward`` bit for bit,
``mel_power`` / ``features`` clip by clip at the clip's own length within the front-end's bounds (audio_util.py)."""
import numpy as np
import pytest
import torch

import avformer_amd as A
import audio_bank_util as U
from audio_util import KEEP_SHARE

AudioBank, AudioAssembler = A.audio_bank.AudioBank, A.audio_bank.AudioAssembler


@pytest.fixture(scope="module")
def fe():
    return A.audio.MelFrontEnd(sample_len_secs=U.SAMPLE_LEN_SECS)


@pytest.fixture(scope="module")
def asm():
    return AudioAssembler(audio_shift_secs=U.SHIFT_SECS)


def _index():
    return torch.tensor(U.INDEX, dtype=torch.int64)


def test_the_case_list_is_complete(fe):
    U.assert_cases_present()
    assert (fe.sample_len_frames, fe.win_length, fe.hop_length, fe.n_fft // 2, fe.full_frames) == (U.N, U.W, U.HOP, U.HALF, U.FULL)


def test_window_table_equals_the_restatement(fe, asm):
    table = asm.window_table(U.make_bank(), _index(), fe)
    assert table.dtype == torch.int64 and tuple(table.shape) == (len(U.INDEX), 2)
    assert np.array_equal(table.numpy(), U.reference_table())


def test_from_waves_truncates_like_python_floats():
    """int((ts / 1000) * sample_rate) of Python floats, for time stamps with fractional milliseconds and for whole ones whose
    product is not exact in binary"""
    ts = [0.0, 33.3667, 1000.0 / 3, 2267.573696, 9999.999999, 123456.789, 1.0 / 44.1, 40.0 / 44.1 * 3, 29.0, 58.0, 290.0]
    bank = AudioBank.from_waves([torch.zeros(10)], [0] * len(ts), ts, 44100)
    assert bank.end_sample.dtype == torch.int64
    assert bank.end_sample.tolist() == [int((t / 1000) * 44100) for t in ts]
    assert U.make_bank().end_sample.tolist() == [e for _, e in U.SAMPLES]
    assert len(U.make_bank()) == U.F and U.make_bank().n_wavs == len(U.WAV_LENGTHS)
    assert U.make_bank().wav_len.tolist() == list(U.WAV_LENGTHS)


def test_forward_is_bit_equal_to_the_restatement(fe, asm):
    audio = asm(U.make_bank(), _index(), fe)
    assert audio.dtype == torch.float32 and tuple(audio.shape) == (len(U.INDEX), 1, U.N)
    assert np.array_equal(audio.numpy(), U.reference_batch()[0])


def test_the_float64_reference_keeps_enough_bins():
    for b, ref in enumerate(U.reference_batch()[1]):
        assert ref is None or U.kept_share(ref) >= KEEP_SHARE, (U.INDEX[b], U.kept_share(ref))


def test_features_and_mel_power_against_float64(fe, asm):
    bank, index = U.make_bank(), _index()
    power, feats = asm.mel_power(bank, index, fe), asm.features(bank, index, fe)
    for t in (power, feats):
        assert t.dtype == torch.float32 and tuple(t.shape) == (len(U.INDEX), 1, 64, U.FULL)
    U.check_against_float64(power, feats, "torch")
    for b in np.nonzero(U.reference_table()[:, 1] == 0)[0]:     # silence is ONE value, (-100 - mean) / std in fp32 arithmetic
        assert torch.equal(feats[b, 0], feats[b, 0, 0, 0].expand(64, U.FULL)), U.INDEX[b]
        assert abs(float(feats[b, 0, 0, 0]) - (-100 + 14.8) / 19.895) < 1e-6, U.INDEX[b]


def test_zero_padding_the_waveform_first_is_another_transform(fe, asm):
    """the frames that straddle the start of a short window differ from those of the window padded to N samples"""
    b = U.INDEX.index(2)                                   # cut by EOF: 22050 samples
    bank, index = U.make_bank(), _index()[b:b + 1]
    got = asm.features(bank, index, fe)[0, 0]
    padded = fe(asm(bank, index, fe)[0, 0])
    assert (got - padded).abs().max().item() > 0.1
    assert (got[:, -40:] - padded[:, -40:]).abs().max().item() < 1e-4   # far from the start the frames are the same


def test_int16_bank_equals_the_fp32_bank_of_the_same_samples(fe, asm):
    b16, b32, index = U.make_bank(torch.int16), U.make_bank(), _index()
    assert b16.wave.dtype == torch.int16 and b32.wave.dtype == torch.float32
    assert torch.equal(asm.window_table(b16, index, fe), asm.window_table(b32, index, fe))
    assert torch.equal(asm(b16, index, fe), asm(b32, index, fe))
    assert torch.equal(asm.mel_power(b16, index, fe), asm.mel_power(b32, index, fe))
    assert torch.equal(asm.features(b16, index, fe), asm.features(b32, index, fe))


def test_bank_validation():
    wave, start, length = torch.zeros(100), torch.tensor([0, 60]), torch.tensor([60, 40])
    wav_of, end = torch.tensor([0, 1, 1], dtype=torch.int32), torch.tensor([5, 6, 7])
    AudioBank(wave, start, length, wav_of, end)
    AudioBank(wave.to(torch.int16), start, length, wav_of, end)
    for bad in ((wave.double(), start, length, wav_of, end), (wave.view(10, 10), start, length, wav_of, end),
                (wave, start.int(), length, wav_of, end), (wave, start, length[:1], wav_of, end),
                (wave, start, length, wav_of.long(), end), (wave, start, length, wav_of, end.int()),
                (wave, start, length, wav_of, end[:2]), (wave, start, length, wav_of, end.to("meta")),
                (wave.to("meta"), start, length, wav_of, end), (wave[::2], start // 2, length // 2, wav_of, end)):
        with pytest.raises(ValueError):
            AudioBank(*bad)
    with pytest.raises(ValueError, match="inside wave"):
        AudioBank(wave, start, torch.tensor([60, 41]), wav_of, end)
    with pytest.raises(ValueError, match="inside wave"):
        AudioBank(wave, torch.tensor([-1, 60]), length, wav_of, end)
    for bad_of in ([0, 2, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match=r"wav_of must lie in \[0, 2\)"):
            AudioBank(wave, start, length, torch.tensor(bad_of, dtype=torch.int32), end)
    with pytest.raises(ValueError, match="one dtype"):
        AudioBank.from_waves([torch.zeros(4), torch.zeros(4, dtype=torch.int16)], [0], [0.0], 44100)


def test_assembler_validation(fe, asm):
    bank, index = U.make_bank(), _index()
    with pytest.raises(ValueError, match="backend"):
        AudioAssembler(backend="cuda")
    with pytest.raises(ValueError, match="audio_shift_secs"):
        AudioAssembler(audio_shift_secs=-1)
    with pytest.raises(ValueError, match="AudioBank"):
        asm(bank.wave, index, fe)
    with pytest.raises(ValueError, match="MelFrontEnd"):
        asm(bank, index, None)
    for bad in (index.int(), index[:0], index.view(2, -1)):
        with pytest.raises(ValueError, match="index must be"):
            asm(bank, bad, fe)
    with pytest.raises(ValueError, match="index is on"):
        asm(bank, index.to("meta"), fe)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AudioAssembler(audio_shift_secs=U.SHIFT_SECS, backend="hip").features(bank, index, fe)
