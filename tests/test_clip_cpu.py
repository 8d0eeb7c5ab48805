"""CPU (no GPU needed): ``clip.ClipFrontEnd`` - the torch backend bitwise against the numpy restatement of the reference's clip
transform (clip_util.py), the 256-entry table the HIP backend indexes, ``draw_flips``, ``invert``, what the constructor and the
HIP backend refuse, and the host-side argument checks of avf_clip_normalize / avf_clip_denormalize."""
import ctypes

import numpy as np
import pytest
import torch

import avformer_amd as A
from clip_util import RGB, RGBM, STATS, all_values_clip, random_clip, reference_transform, same_bits

CK = [(C, k) for C in (1, 3, 4) for k in range(1, C + 1)]


@pytest.mark.parametrize("layout", ["cthw", "tchw"])
@pytest.mark.parametrize("C,k", CK)
def test_torch_backend_equals_the_numpy_restatement_bitwise(C, k, layout):
    mean, std = STATS[C]
    clip = random_clip(2, 3, 4, 5, C, seed=10 * C + k)
    for dtype in (torch.float32, torch.bfloat16):
        fe = A.clip.ClipFrontEnd(mean, std, channels=k, layout=layout, out_dtype=dtype)
        for flip in (None, [True, False], [True, True]):
            want = reference_transform(clip.numpy(), mean, std, flip, k, layout, dtype == torch.bfloat16)
            got = fe(clip, None if flip is None else torch.tensor(flip))
            assert got.dtype == dtype and got.is_contiguous()
            assert got.shape == ((2, k, 3, 4, 5) if layout == "cthw" else (2, 3, k, 4, 5))
            assert same_bits(got, want), (dtype, flip)
            if flip is not None:                                    # uint8 flags are the same flags
                assert same_bits(fe(clip, torch.tensor(flip, dtype=torch.uint8)), want)
            for b in range(2):                                      # a 4-D clip: the same planes without the batch axis
                one = fe(clip[b], None if flip is None else torch.tensor(flip[b:b + 1]))
                assert one.shape == want.shape[1:] and same_bits(one, want[b]), (dtype, flip, b)


def test_default_is_the_rgb_clip_transform_of_the_reference():
    fe = A.clip.ClipFrontEnd()
    assert (fe.backend, fe.layout, fe.out_dtype, fe.in_channels, fe.channels) == ("torch", "cthw", torch.float32, 3, 3)
    assert (A.clip.RGB_MEAN, A.clip.RGB_STD) == RGB and (A.clip.RGBM_MEAN, A.clip.RGBM_STD) == RGBM
    clip = random_clip(1, 2, 3, 4, 3, seed=1)
    assert same_bits(fe(clip), reference_transform(clip.numpy(), *RGB))
    mask = A.clip.ClipFrontEnd(A.clip.RGBM_MEAN, A.clip.RGBM_STD, channels=1)   # k = 1 of RGB + mask: the mask alone
    clip4 = random_clip(1, 2, 3, 4, 4, seed=2)
    want = reference_transform(clip4.numpy(), *RGBM)[:, 3:]
    assert same_bits(mask(clip4), want)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_lut_is_the_torch_backends_output_for_every_byte_value(C):
    mean, std = STATS[C]
    fe = A.clip.ClipFrontEnd(mean, std)
    assert fe.lut.shape == (C, 256) and fe.lut.dtype == torch.float32
    clip = all_values_clip(C)                                       # [1, 1, 16, 16, C]
    y = fe(clip)                                                    # [1, C, 1, 16, 16]
    for c in range(C):
        assert sorted(clip[0, 0, :, :, c].flatten().tolist()) == list(range(256))
        assert same_bits(y[0, c, 0], fe.lut[c][clip[0, 0, :, :, c].long()]), c
    v = np.arange(256).astype(np.float32) / 255                     # ... and the restated op sequence on the byte values
    for c in range(C):
        row = v.copy()
        row -= np.float32(mean[c])
        row /= np.float32(std[c])
        assert same_bits(fe.lut[c], torch.from_numpy(row)), c


def test_black_frame_gives_minus_mean_over_std_exactly():
    fe = A.clip.ClipFrontEnd(A.clip.RGBM_MEAN, A.clip.RGBM_STD)
    y = fe(torch.zeros(1, 2, 3, 4, 4, dtype=torch.uint8))
    for c in range(4):
        want = torch.tensor(-np.float32(A.clip.RGBM_MEAN[c]) / np.float32(A.clip.RGBM_STD[c]))
        assert same_bits(y[0, c], want.expand(2, 3, 4).contiguous()), c


def test_draw_flips():
    g = torch.Generator().manual_seed(5)
    a = A.clip.draw_flips(64, generator=g)
    b = A.clip.draw_flips(64, generator=torch.Generator().manual_seed(5))
    assert a.dtype == torch.bool and a.shape == (64,) and a.device.type == "cpu" and torch.equal(a, b)
    assert 0 < int(a.sum()) < 64
    assert not A.clip.draw_flips(16, p=0.0).any() and A.clip.draw_flips(16, p=1.0).all()
    assert torch.equal(a, torch.rand(64, generator=torch.Generator().manual_seed(5)) < 0.5)


@pytest.mark.parametrize("layout", ["cthw", "tchw"])
def test_invert_is_within_one_grey_level(layout):
    for C in (1, 3, 4):
        fe = A.clip.ClipFrontEnd(*STATS[C], layout=layout)
        clip = torch.cat([random_clip(1, 2, 16, 16, C, seed=C), all_values_clip(C, T=2)])
        back = fe.invert(fe(clip))
        assert back.dtype == torch.uint8 and back.shape == clip.shape and back.is_contiguous()
        d = back.int() - clip.int()
        assert int(d.max()) <= 0 and int(d.min()) >= -1, (int(d.min()), int(d.max()))   # truncation, as in the reference
        assert fe.invert(fe(clip[0])).shape == clip[0].shape
        assert torch.equal(fe.invert(fe(clip[0])), back[0])
        flipped = fe.invert(fe(clip, torch.tensor([True, False])))          # a flip is not undone
        assert torch.equal(flipped[1], back[1]) and torch.equal(flipped[0], back[0].flip(2))


def test_invert_clamps_and_maps_nan_to_zero():
    fe = A.clip.ClipFrontEnd((0.5,), (0.25,))
    x = torch.tensor([-1e9, -2.0 - 1e-3, -2.0, 0.0, 2.0, 2.0 + 1e-3, 1e9, float("inf"), float("-inf"), float("nan"),
                      (200.0 / 255 - 0.5) / 0.25, 1e-3]).view(1, 1, 1, 1, 12)
    want = [0, 0, 0, 127, 255, 255, 255, 255, 0, 0, None, 127]
    got = fe.invert(x).flatten().tolist()
    for i, w in enumerate(want):
        if w is not None:
            assert got[i] == w, (i, got[i], w)
    assert got[10] in (199, 200)
    assert torch.equal(fe.invert(x.to(torch.bfloat16)), fe.invert(x.to(torch.bfloat16).float()))
    with pytest.raises(ValueError, match="channels"):
        A.clip.ClipFrontEnd(channels=1).invert(torch.zeros(1, 1, 2, 2, 2))


def test_constructor_refusals():
    F = A.clip.ClipFrontEnd
    for bad in ("triton", ""):
        with pytest.raises(ValueError, match="backend"):
            F(backend=bad)
    with pytest.raises(ValueError, match="layout"):
        F(layout="thwc")
    for bad in (torch.float16, torch.float64, torch.uint8):
        with pytest.raises(ValueError, match="out_dtype"):
            F(out_dtype=bad)
    with pytest.raises(ValueError, match="mean"):
        F(mean=(0.5, 0.5), std=(0.2,))
    with pytest.raises(ValueError, match="channels"):
        F(mean=(0.5,) * 5, std=(0.2,) * 5)
    with pytest.raises(ValueError, match="channels"):
        F(mean=(), std=())
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="channels"):
            F(channels=bad)
    fe = F()
    with pytest.raises(ValueError, match="uint8"):
        fe(torch.zeros(1, 2, 3, 4, 3))
    with pytest.raises(ValueError, match="channels"):
        fe(torch.zeros(1, 2, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="flip"):
        fe(torch.zeros(2, 2, 3, 4, 3, dtype=torch.uint8), torch.tensor([True]))
    with pytest.raises(ValueError, match="flip"):
        fe(torch.zeros(2, 2, 3, 4, 3, dtype=torch.uint8), torch.tensor([1.0, 0.0]))


def test_hip_backend_has_no_cpu_fallback():
    fe = A.clip.ClipFrontEnd(backend="hip")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe(torch.zeros(1, 2, 3, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe.invert(torch.zeros(1, 3, 2, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ops.clip_normalize(torch.zeros(1, 2, 3, 4, 3, dtype=torch.uint8), fe.lut)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ops.clip_denormalize(torch.zeros(1, 3, 2, 3, 4), fe.mean_t, fe.std_t)


def test_state_dict_is_empty_for_both_backends():
    a, b = A.clip.ClipFrontEnd(backend="torch"), A.clip.ClipFrontEnd(backend="hip")
    assert list(a.state_dict()) == list(b.state_dict()) == []
    b.load_state_dict(a.state_dict(), strict=True)
    assert same_bits(a.lut, b.lut) and [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    assert list(a.parameters()) == []


def test_entry_points_check_their_arguments_on_the_host():
    """every refusal names its argument and comes before a launch: no GPU is needed, no pointer is dereferenced"""
    A._build.build()
    lib = A._lib.load()
    p = ctypes.c_void_p(4096)

    def norm(src=p, B=2, T=2, H=3, W=5, C=3, k=3, lut=p, flip=p, dst=p, dtype=A._lib.F32, layout=A._lib.CLIP_CTHW):
        return lib.avf_clip_normalize(src, B, T, H, W, C, k, lut, flip, dst, dtype, layout, None)

    def denorm(src=p, dtype=A._lib.F32, layout=A._lib.CLIP_CTHW, B=2, T=2, H=3, W=5, C=3, mean=p, std=p, dst=p):
        return lib.avf_clip_denormalize(src, dtype, layout, B, T, H, W, C, mean, std, dst, None)

    for bad, name in ((dict(src=None), b"src is null"), (dict(lut=None), b"lut is null"), (dict(dst=None), b"dst is null"),
                      (dict(B=0), b"B is"), (dict(T=0), b"T is"), (dict(H=-1), b"H is"), (dict(W=0), b"W is"),
                      (dict(C=0), b"C is"), (dict(C=5, k=5), b"C is"), (dict(k=0), b"k is"), (dict(k=4), b"k is"),
                      (dict(dtype=2), b"out_dtype"), (dict(dtype=-1), b"out_dtype"), (dict(layout=2), b"layout"),
                      (dict(dst=ctypes.c_void_p(4098)), b"dst is not aligned"), (dict(B=1 << 31), b"too large"),
                      (dict(B=1 << 20, T=1 << 10, H=1 << 20, W=1 << 20), b"too large")):
        assert norm(**bad) != 0, bad
        assert name in lib.avf_last_error() and b"clip_normalize" in lib.avf_last_error(), (bad, lib.avf_last_error())
    for bad, name in ((dict(src=None), b"src is null"), (dict(mean=None), b"mean is null"), (dict(std=None), b"std is null"),
                      (dict(dst=None), b"dst is null"), (dict(B=0), b"B is"), (dict(T=0), b"T is"), (dict(H=0), b"H is"),
                      (dict(W=-3), b"W is"), (dict(C=0), b"C is"), (dict(C=5), b"C is"), (dict(dtype=2), b"in_dtype"),
                      (dict(layout=-1), b"layout"), (dict(src=ctypes.c_void_p(4097), dtype=A._lib.BF16), b"src is not aligned")):
        assert denorm(**bad) != 0, bad
        assert name in lib.avf_last_error() and b"clip_denormalize" in lib.avf_last_error(), (bad, lib.avf_last_error())
