"""-m gpu: ``audio_bank.AudioAssembler(backend="hip")`` - csrc/mel_bank.hip - on the case batch of audio_bank_util.py: against
float64 clip by clip at the clip's own length (audio_util's bounds), bit for bit against ``MelFrontEnd(backend="hip")`` on every
window's own slice (the source changes addresses, not arithmetic), and the gather bit for bit against the torch backend for fp32
and int16 banks at every placement of source and destination inside their 16-byte chunks."""
import numpy as np
import pytest
import torch

import avformer_amd as A
import audio_bank_util as U
from audio_util import OUT_ABS, _wave

pytestmark = pytest.mark.gpu

AudioBank, AudioAssembler = A.audio_bank.AudioBank, A.audio_bank.AudioAssembler


@pytest.fixture(scope="module")
def fe():
    return A.audio.MelFrontEnd(sample_len_secs=U.SAMPLE_LEN_SECS, backend="hip").cuda()


@pytest.fixture(scope="module")
def asm():
    return AudioAssembler(audio_shift_secs=U.SHIFT_SECS, backend="hip")


@pytest.fixture(scope="module")
def ref_asm():
    return AudioAssembler(audio_shift_secs=U.SHIFT_SECS)


@pytest.fixture(scope="module")
def index():
    return torch.tensor(U.INDEX, dtype=torch.int64).cuda()


@pytest.fixture(scope="module", params=[torch.float32, torch.int16], ids=["fp32", "int16"])
def bank(request):
    return U.make_bank(request.param).to("cuda")


def test_features_and_mel_power_against_float64(bank, index, fe, asm):
    U.assert_cases_present()
    power, feats = asm.mel_power(bank, index, fe), asm.features(bank, index, fe)
    for t in (power, feats):
        assert t.dtype == torch.float32 and tuple(t.shape) == (len(U.INDEX), 1, 64, U.FULL) and t.is_cuda and not t.requires_grad
    U.check_against_float64(power, feats, f"hip {bank.wave.dtype}")


def test_ragged_rows_are_the_dense_kernel_on_each_window(bank, index, fe, asm, ref_asm):
    table = ref_asm.window_table(bank, index, fe).cpu().tolist()
    assert np.array_equal(np.array(table), U.reference_table())
    power, feats = asm.mel_power(bank, index, fe), asm.features(bank, index, fe)
    silent_in = torch.zeros(U.N, device="cuda")
    silent_power, silent_feats = fe.mel_power(silent_in), fe(silent_in)
    assert not silent_power.any()
    for b, (first, got) in enumerate(table):
        if got == 0:
            assert not power[b, 0].any(), U.INDEX[b]
            assert torch.equal(feats[b, 0], silent_feats), U.INDEX[b]
            continue
        clip = bank.wave[first:first + got]
        clip = clip.to(torch.float32) * 2.0 ** -15 if clip.dtype == torch.int16 else clip
        p = fe.mel_power(clip)
        assert p.shape[-1] == 1 + got // U.HOP
        assert not power[b, 0, :, :U.FULL - p.shape[-1]].any(), U.INDEX[b]
        assert torch.equal(power[b, 0, :, U.FULL - p.shape[-1]:], p), U.INDEX[b]
        assert torch.equal(feats[b, 0], fe(clip)), U.INDEX[b]


@pytest.mark.parametrize("dst_shift", [0, 1, 2, 3])
@pytest.mark.parametrize("src_shift", [0, 1, 2, 3])
def test_gather_is_bit_equal_at_every_alignment(bank, index, fe, asm, ref_asm, src_shift, dst_shift):
    """the bank 0, 4, 8 and 12 bytes behind a 16-byte boundary, surrounded by NaN (32767 for int16); the destination 0, 4, 8 and
    12 bytes behind one, inside a guarded buffer"""
    i16 = bank.wave.dtype == torch.int16
    lead = src_shift * (2 if i16 else 1) + 8
    total = bank.wave.numel()
    buf = torch.full((total + 32,), 32767 if i16 else float("nan"), dtype=bank.wave.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[lead:lead + total] = bank.wave
    moved = AudioBank(buf[lead:lead + total], bank.wav_start, bank.wav_len, bank.wav_of, bank.end_sample)
    assert moved.wave.data_ptr() % 16 == 4 * src_shift
    want = ref_asm(bank, index, fe)
    assert np.array_equal(want.cpu().numpy(), U.reference_batch()[0])

    B = index.numel()
    guard = torch.full((B * U.N + 16,), -7.0, device="cuda")
    out = guard[4 + dst_shift:4 + dst_shift + B * U.N].view(B, U.N)
    assert out.data_ptr() % 16 == 4 * dst_shift
    N, w, shift = U.N, U.W, U.SHIFT
    A.ops.wave_gather(moved.wave, moved.wav_start, moved.wav_len, moved.wav_of, moved.end_sample, index, N, w, shift, out=out)
    assert not torch.isnan(out).any() and out.abs().max().item() < 0.9      # nothing outside the bank was read
    assert torch.equal(out.view(B, 1, U.N), want)
    assert (guard[:4 + dst_shift] == -7.0).all() and (guard[4 + dst_shift + B * U.N:] == -7.0).all()
    if dst_shift == 0:
        got = asm(moved, index, fe)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, 1, U.N)
        assert torch.equal(got, want)


def test_mel_output_is_guarded_and_repeatable(bank, index, fe, asm):
    B = index.numel()
    n = B * 64 * U.FULL
    guard = torch.full((n + 64,), -7.0, device="cuda")
    out = guard[32:32 + n].view(B, 64, U.FULL)
    A.ops.mel_power_bank(bank.wave, bank.wav_start, bank.wav_len, bank.wav_of, bank.end_sample, index, U.N, U.SHIFT, fe.window, fe.fb,
                         fe.bin_lo, fe.bin_hi, fe.n_fft, fe.hop_length, U.FULL, out=out)
    assert (guard[:32] == -7.0).all() and (guard[32 + n:] == -7.0).all()
    assert torch.equal(out.view(B, 1, 64, U.FULL), asm.mel_power(bank, index, fe))
    assert torch.equal(asm.features(bank, index, fe), asm.features(bank, index, fe))


def test_a_quiet_clip_keeps_its_own_floor(fe, asm):
    loud, quiet = _wave(60000, 1, 30.0), _wave(60000, 2, 1e-5)
    pair = AudioBank.from_waves([loud, quiet], [0, 1], [1000.0, 1000.0]).to("cuda")
    both = asm.features(pair, torch.tensor([0, 1]).cuda(), fe)
    for b in (0, 1):
        assert torch.equal(both[b], asm.features(pair, torch.tensor([b]).cuda(), fe)[0]), b
    assert both[1].min().item() < both[0].min().item() - 1.0
    first, got = AudioAssembler(audio_shift_secs=U.SHIFT_SECS).window_table(pair, torch.tensor([1]).cuda(), fe)[0].tolist()
    assert (first, got) == (60000 + U.SHIFT, 60000 - U.SHIFT)               # E = N: off = shift, cut by EOF
    assert torch.equal(both[1, 0], fe(pair.wave[first:first + got]))


def test_capture_and_replay(bank, fe, asm):
    """memset + two launches, index read on the device: a plain serial graph"""
    static = torch.tensor(U.INDEX[:8], dtype=torch.int64).cuda()
    asm.features(bank, static, fe)                                          # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = asm.features(bank, static, fe)
    other = torch.tensor(U.INDEX[-8:], dtype=torch.int64).cuda()
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    assert torch.equal(got, asm.features(bank, other, fe))
    assert not torch.equal(got, asm.features(bank, torch.tensor(U.INDEX[:8], dtype=torch.int64).cuda(), fe))


def test_hip_backend_validation(bank, index, fe, asm):
    with pytest.raises(ValueError, match="backend='hip'"):
        asm.features(bank, index, A.audio.MelFrontEnd(sample_len_secs=U.SAMPLE_LEN_SECS).cuda())
    with pytest.raises(ValueError, match="index is on"):
        asm.features(bank, index.cpu(), fe)
    with pytest.raises(RuntimeError, match="overlaps the bank"):
        w32 = bank.wave if bank.wave.dtype == torch.float32 else bank.wave.view(torch.float32)
        A.ops.wave_gather(bank.wave, bank.wav_start, bank.wav_len, bank.wav_of, bank.end_sample, index[:1], 64, U.W, U.SHIFT,
                          out=w32[:64].view(1, 64))


def test_full_size_batch():
    """B = 64 ten-second windows, consecutive samples of a 60 s wav"""
    fe10 = A.audio.MelFrontEnd(backend="hip").cuda()
    ts = 20000.0 + np.arange(64) * (1000.0 / 30)
    bank = AudioBank.from_waves([_wave(60 * 44100, 5)], [0] * 64, ts).to("cuda")
    index = torch.arange(64).cuda()
    y = AudioAssembler(backend="hip").features(bank, index, fe10)
    assert tuple(y.shape) == (64, 1, 64, 1001) and y.dtype == torch.float32 and torch.isfinite(y).all()
    want = AudioAssembler().features(bank, index, A.audio.MelFrontEnd().cuda())
    assert (y - want).abs().max().item() < OUT_ABS
