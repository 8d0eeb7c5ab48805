"""-m gpu: ``audio.MelFrontEnd(backend="hip")`` - the fused kernels of csrc/mel.hip - against float64: the mel power
against a numpy restatement with the module's own filterbank (audio_util.mel_power_f64), the normalised features against
oracle/audio_front_end.py.  Tolerances are the front-end's own (audio_util.py): 2e-5 of the clip's largest mel power, 0.02 dB on
the bins above 1e-6 of it (>= 99 % of the bins), 2e-3 on the normalised output.  One-second front-ends (full_frames = 101)
keep every case small; one case runs the ten-second default."""
import numpy as np
import pytest
import torch

import avformer_amd as A
from audio_util import _wave, assert_features_close, assert_mel_power_close, mel_power_f64, wave_and_power
from oracle.audio_front_end import mel_features

pytestmark = pytest.mark.gpu

LENGTHS = (513, 881, 882, 1323, 4409, 4410, 4411, 44100, 50000)   # smallest legal clip; one window; a hop multiple and its
GAINS = (1.0, 1e-5, 30.0)                                         # neighbours; exactly full_frames; more frames than that


@pytest.fixture(scope="module")
def fe():
    return A.audio.MelFrontEnd(sample_len_secs=1, backend="hip").cuda()


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("samples", LENGTHS)
def test_mel_power_and_features_against_float64(fe, samples, gain):
    x, ref = wave_and_power(samples, samples % 7, gain, (44100, 64))
    frames = 1 + samples // 441
    p = fe.mel_power(x.cuda())
    assert p.shape == (64, frames) and p.dtype == torch.float32 and p.is_cuda and not p.requires_grad
    assert_mel_power_close(p, ref, f"S={samples} gain={gain}")
    y = fe(x.cuda())
    assert y.shape == (64, max(frames, 101)) and y.dtype == torch.float32
    assert_features_close(y, mel_features(x.numpy(), sample_len_secs=1), f"S={samples} gain={gain}")


def test_edge_frames_reflect_the_clip_ends(fe):
    """a ramp plus noise has no symmetry a wrong reflection index could hide behind; the first and last two frames (the ones
    that read reflected samples) are held to the tolerance against THEIR OWN maximum"""
    g = torch.Generator().manual_seed(11)
    x = torch.linspace(-0.5, 1.0, 2000) + 0.05 * torch.randn(2000, generator=g)
    ref = mel_power_f64(x.numpy(), fe)
    p = fe.mel_power(x.cuda())
    assert p.shape == ref.shape == (64, 5)
    for t in (0, 1, 3, 4):
        assert_mel_power_close(p[:, t:t + 1], ref[:, t:t + 1], f"frame {t}")


def test_short_clip_is_left_padded_with_floor_frames(fe):
    x, ref = wave_and_power(4410, 0, 1.0, (44100, 64))
    y = fe(x.cuda()).cpu()
    assert y.shape == (64, 101)
    floor = (10 * np.log10(ref.max()) - 80.0 + 14.8) / 19.895
    pad = y[:, :101 - 11]
    assert torch.equal(pad, pad[0, 0].expand_as(pad)) and abs(float(pad[0, 0]) - floor) < 2e-3
    assert_features_close(y[:, -11:], mel_features(x.numpy(), sample_len_secs=1)[:, -11:], "last 11 columns")


def test_digital_silence(fe):
    y = fe(torch.zeros(2000).cuda())
    assert y.shape == (64, 101)
    want = torch.tensor(np.float32((-100 + 14.8) / 19.895))
    assert torch.equal(y.cpu(), want.expand(64, 101)), (y.min().item(), y.max().item(), want.item())


def test_clips_are_clamped_in_their_own_group(fe):
    S = 5000
    clips = torch.stack([_wave(S, i, g) for i, g in enumerate((1.0, 1e-3, 30.0, 1e-5))]).cuda()
    y2 = fe(clips)                                   # [4, S]: one clip per row
    y3 = fe(clips[:, None])                          # [4, 1, S]
    assert y2.shape == (4, 64, 101) and y3.shape == (4, 1, 64, 101)
    for i in range(4):
        assert torch.equal(y2[i], fe(clips[i])), i
        assert torch.equal(y3[i], fe(clips[i][None, None])[0]), i
        assert torch.equal(y3[i, 0], y2[i]), i
    pairs = clips.reshape(2, 2, S)                   # [2, 2, S]: a clip is two channels, clamped against their common peak
    y = fe(pairs)
    assert y.shape == (2, 2, 64, 101)
    for i in range(2):
        assert torch.equal(y[i], fe(pairs[i:i + 1])[0]), i
    want = A.audio.MelFrontEnd(sample_len_secs=1).cuda()(pairs)
    assert (y - want).abs().max().item() < 2e-3
    assert not torch.equal(y[0, 1], y2[1])           # the quiet channel sits on the loud channel's floor, not on its own


def test_two_calls_give_the_same_bits(fe):
    x = torch.stack([_wave(50000, 3), _wave(50000, 4, 1e-3)]).cuda()
    assert torch.equal(fe(x), fe(x)) and torch.equal(fe.mel_power(x), fe.mel_power(x))


@pytest.mark.parametrize("n_mels", [40, 128])
def test_other_configuration(n_mels):
    """48 kHz: window 960, hop 480, n_fft still 1024; 40 filters leave lanes idle, 128 take two filters per lane"""
    fe48 = A.audio.MelFrontEnd(sample_rate=48000, n_mels=n_mels, sample_len_secs=1, backend="hip").cuda()
    assert (fe48.n_fft, fe48.win_length, fe48.hop_length) == (1024, 960, 480)
    live = (fe48.bin_hi > fe48.bin_lo).cpu().numpy()
    assert live.all() == (n_mels == 40)
    for samples in (5000, 50000):
        x, ref = wave_and_power(samples, 2, 1.0, (48000, n_mels))
        p = fe48.mel_power(x.cuda())
        assert p.shape == (n_mels, 1 + samples // 480)
        assert_mel_power_close(p, ref, f"48k n_mels={n_mels} S={samples}", live)
        y = fe48(x.cuda())
        assert y.shape == (n_mels, max(1 + samples // 480, 101))
        assert_features_close(y, mel_features(x.numpy(), sample_rate=48000, n_mels=n_mels, sample_len_secs=1),
                              f"48k n_mels={n_mels} S={samples}")


def test_input_dtype_and_layout(fe):
    x = _wave(6000, 5).cuda()
    x16 = x.to(torch.float16)
    assert torch.equal(fe(x16), fe(x16.float()))
    assert torch.equal(fe(x.double()), fe(x))                      # (the test signal's fp64 copy rounds back to itself)
    wide = torch.stack([_wave(12000, 6), _wave(12000, 7)]).cuda()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(fe(view), fe(view.contiguous()))
    with pytest.raises(ValueError, match="512"):
        fe(torch.zeros(512).cuda())
    with pytest.raises(ValueError, match="512"):
        fe.mel_power(torch.zeros(3, 512).cuda())


def test_full_size_clips():
    fe10 = A.audio.MelFrontEnd(backend="hip").cuda()
    clips = [_wave(441000, 0), _wave(441000, 1, 1e-3)]
    y = fe10(torch.stack(clips)[:, None].cuda())
    assert y.shape == (2, 1, 64, 1001) and y.dtype == torch.float32 and y.is_cuda
    for i, c in enumerate(clips):
        assert_features_close(y[i, 0], mel_features(c.numpy()), f"clip {i}")


def test_capture_and_replay(fe):
    """memset + two launches, no allocation or synchronisation inside the library: a plain serial graph"""
    static = torch.stack([_wave(4410, 0), _wave(4410, 1, 1e-3)]).cuda()
    fe(static)                                                     # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe(static)
    other = torch.stack([_wave(4410, 2, 30.0), _wave(4410, 3, 1e-5)]).cuda()
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    assert torch.equal(got, fe(other))
    assert not torch.equal(got, fe(torch.stack([_wave(4410, 0), _wave(4410, 1, 1e-3)]).cuda()))
