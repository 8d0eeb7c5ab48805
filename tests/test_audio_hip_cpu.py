"""CPU (no GPU needed): the host side of ``audio.MelFrontEnd(backend="hip")`` - the backend switch and what it refuses, the
filterbank's bin ranges the kernel sums over, an unchanged state_dict, and the argument checks of avf_mel_power /
avf_mel_db_norm, which refuse bad arguments on the host before anything is launched."""
import ctypes

import pytest
import torch

import avformer_amd as A
from audio_util import _wave


def test_torch_is_the_default_backend_and_unchanged():
    plain, named = A.audio.MelFrontEnd(sample_len_secs=1), A.audio.MelFrontEnd(sample_len_secs=1, backend="torch")
    assert plain.backend == "torch" and named.backend == "torch"
    x = torch.stack([_wave(5000, 0), _wave(5000, 1, 1e-3)])
    assert torch.equal(plain(x), named(x)) and torch.equal(plain.mel_power(x), named.mel_power(x))
    assert torch.equal(plain(x[:, None]), named(x[:, None]))
    assert [n for n, _ in plain.named_buffers()] == ["window", "fb"]


def test_hip_backend_has_no_cpu_fallback():
    fe = A.audio.MelFrontEnd(sample_len_secs=1, backend="hip")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe(_wave(5000, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe.mel_power(_wave(5000, 0)[None])


def test_unknown_backend_is_refused():
    with pytest.raises(ValueError, match="backend"):
        A.audio.MelFrontEnd(backend="triton")
    with pytest.raises(ValueError, match="backend"):
        A.audio.MelFrontEnd(backend="")


def test_hip_backend_refuses_another_n_fft_at_construction():
    with pytest.raises(ValueError, match="n_fft"):
        A.audio.MelFrontEnd(sample_rate=16000, window_size=25e-3, backend="hip")       # 400 samples -> n_fft 512
    assert A.audio.MelFrontEnd(sample_rate=16000, window_size=25e-3).n_fft == 512       # the torch backend takes it
    fe = A.audio.MelFrontEnd(sample_rate=48000, n_mels=40, sample_len_secs=1, backend="hip")
    assert (fe.n_fft, fe.win_length, fe.hop_length, fe.full_frames) == (1024, 960, 480, 101)


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=48000, n_mels=40)], ids=["default", "48k-40"])
def test_bin_ranges_cover_the_filterbank_and_are_tight(kw):
    fe = A.audio.MelFrontEnd(backend="hip", **kw)
    fb, lo, hi = fe.fb, fe.bin_lo, fe.bin_hi
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.shape == hi.shape == (fe.n_mels,)
    lo2, hi2 = A.audio.mel_bin_ranges(fb)
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2)
    k = torch.arange(fb.shape[0])[:, None]
    inside = (k >= lo[None]) & (k < hi[None])
    assert bool((fb[~inside] == 0).all())                       # every non-zero of fb lies inside its filter's range
    assert bool((lo >= 0).all()) and bool((hi <= fb.shape[0]).all()) and bool((lo <= hi).all())
    for m in range(fe.n_mels):
        if bool((fb[:, m] == 0).all()):
            assert int(lo[m]) == int(hi[m])
        else:
            assert float(fb[int(lo[m]), m]) != 0.0 and float(fb[int(hi[m]) - 1, m]) != 0.0, m
    assert int((hi - lo).sum()) < 0.05 * fb.numel()            # (the dense matmul multiplies > 95 % zeros)


def test_bin_ranges_of_an_all_zero_filter_are_empty():
    fb = torch.zeros(513, 3)
    fb[7:9, 0] = 1.0
    fb[512, 2] = 0.5
    lo, hi = A.audio.mel_bin_ranges(fb)
    assert lo.tolist() == [7, 0, 512] and hi.tolist() == [9, 0, 513]


def test_state_dict_is_the_same_for_both_backends():
    a, b = A.audio.MelFrontEnd(backend="torch"), A.audio.MelFrontEnd(backend="hip")
    assert list(a.state_dict()) == list(b.state_dict()) == []
    b.load_state_dict(a.state_dict(), strict=True)
    assert torch.equal(a.fb, b.fb) and torch.equal(a.window, b.window)


def test_entry_points_check_their_arguments_on_the_host():
    """every refusal names its argument and comes before a launch: no GPU is needed, no pointer is dereferenced"""
    A._build.build()
    lib = A._lib.load()
    p = ctypes.c_void_p(4096)

    def power(audio=p, rows=2, samples=4410, window=p, win=882, n_fft=1024, hop=441, fb=p, lo=p, hi=p, n_mels=64, full=101,
              rpc=1, mel=p, peak=p):
        return lib.avf_mel_power(audio, rows, samples, window, win, n_fft, hop, fb, lo, hi, n_mels, full, rpc, mel, peak, None)

    def norm(mel=p, peak=p, rows=2, n_mels=64, frames=101, rpc=1):
        return lib.avf_mel_db_norm(mel, peak, rows, n_mels, frames, rpc, 80.0, -14.8, 19.895, None)

    for bad, name in ((dict(audio=None), b"audio"), (dict(window=None), b"window"), (dict(fb=None), b"fb"),
                      (dict(lo=None), b"bin_lo"), (dict(hi=None), b"bin_hi"), (dict(mel=None), b"mel is null"),
                      (dict(peak=None), b"peak"), (dict(samples=512), b"samples"), (dict(n_fft=2048), b"n_fft"),
                      (dict(n_fft=512, samples=4410), b"n_fft"), (dict(win=1025), b"win_length"), (dict(n_mels=0), b"n_mels"),
                      (dict(n_mels=129), b"n_mels"), (dict(hop=0), b"hop"), (dict(rpc=3), b"rows_per_clip"),
                      (dict(rows=0), b"rows")):
        assert power(**bad) != 0, bad
        assert name in lib.avf_last_error(), (bad, lib.avf_last_error())
    for bad, name in ((dict(mel=None), b"mel"), (dict(peak=None), b"peak"), (dict(n_mels=0), b"n_mels"),
                      (dict(n_mels=129), b"n_mels"), (dict(rpc=3), b"rows_per_clip"), (dict(frames=0), b"frames")):
        assert norm(**bad) != 0, bad
        assert name in lib.avf_last_error(), (bad, lib.avf_last_error())
