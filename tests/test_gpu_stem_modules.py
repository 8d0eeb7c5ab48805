"""-m gpu: the fused stem at the module level - ``FrozenResFormer(backend="hip", stem="hip")``, ``FrozenAudioModel(backend="hip")``
and the avformer built on both (csrc/stem.hip in front of csrc/conv.hip) against the reference's stem fixture (G21) and against
their own defining ``backend="torch"``.

Intermediates are stored in bf16, so the measure is the project's bf16-mode cap for outputs: relative
Frobenius error <= 1.5e-2.  ``FrozenAudioModel`` is held to its own torch backend: no reference fixture pins it (the reference
builds its AudioModel from torchvision).  Measured on an MI355X: DESIGN.md section 9."""
import pytest
import torch

import backbone_util as bu
from gpu_util import rel_fro
from test_stem_modules_cpu import g21

pytestmark = pytest.mark.gpu

CAP = 1.5e-2


@pytest.fixture(scope="module")
def A():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A


@pytest.fixture(scope="module")
def model():
    """one FrozenResFormer on the device; the tests switch its backend and stem"""
    return bu.resformer("torch").cuda()


@pytest.fixture(scope="module")
def audio(A):
    torch.manual_seed(2021)
    return bu.randomize_batchnorm(A.FrozenAudioModel(), 2022).eval().cuda()


def _randn(shape, seed=5):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _alive(y):
    return bool(torch.isfinite(y).all()) and float(y.abs().mean()) > 0.05


class _Counting:
    """counts the calls of ``module.name`` while the block runs"""

    def __init__(self, module, name):
        self.module, self.name, self.calls = module, name, 0

    def __enter__(self):
        self.orig = getattr(self.module, self.name)

        def wrapper(*a, **kw):
            self.calls += 1
            return self.orig(*a, **kw)
        setattr(self.module, self.name, wrapper)
        return self

    def __exit__(self, *exc):
        setattr(self.module, self.name, self.orig)


def test_g21_through_the_stem_kernel_matches_the_reference_fixture(A):
    sd, x, want = g21()
    wp, sc, sh = A.ops.stem_pack_weight(*[sd[k].cuda() for k in ("conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var")],
                                        eps=1e-5)
    got = A.ops.stem_nchw(x.cuda(), wp, sc, sh, out_dtype=torch.float32)
    assert got.shape == (2, 10, 8, 64)
    err = rel_fro(got.permute(0, 3, 1, 2), want)
    print(f"STEMMODSTAT g21 fp32 out rel_fro {err:.3e}")
    assert err <= CAP and _alive(got)
    err = rel_fro(A.ops.stem_nchw(x.cuda(), wp, sc, sh).float().permute(0, 3, 1, 2), want)
    print(f"STEMMODSTAT g21 bf16 out rel_fro {err:.3e}")
    assert err <= CAP


@pytest.mark.parametrize("shape", [(2, 3, 112, 112), (1, 2, 3, 112, 112)], ids=["frames", "clip"])
def test_resformer_with_the_hip_stem_matches_the_torch_backend(model, shape):
    x = _randn(shape)
    with torch.no_grad():
        want = model.set_backend("torch", stem="torch")(x)
        got = model.set_backend("hip", stem="hip")(x)
    assert got.shape == want.shape == (2, 512) and got.dtype == torch.float32 and _alive(got) and _alive(want)
    err = rel_fro(got, want)
    print(f"STEMMODSTAT resformer stem=hip {shape} rel_fro {err:.3e}")
    assert err <= CAP


@pytest.mark.parametrize("shape", [(2, 1, 64, 1001), (2, 1, 64, 130)], ids=["mel1001", "mel130"])
def test_audio_model_hip_matches_its_torch_backend(audio, shape):
    x = _randn(shape, seed=8)
    with torch.no_grad():
        want = audio.set_backend("torch")(x)
        got = audio.set_backend("hip")(x)
    assert got.shape == want.shape == (2, 512) and got.dtype == torch.float32 and _alive(got) and _alive(want)
    err = rel_fro(got, want)
    print(f"STEMMODSTAT audio_model {shape} rel_fro {err:.3e}")
    assert err <= CAP


def test_the_stem_switch_chooses_between_one_launch_and_the_torch_stem(A, model):
    x = _randn((2, 3, 112, 112))
    with torch.no_grad(), _Counting(A.ops, "stem_nchw") as stem, _Counting(A.backbone, "to_nhwc") as conv:
        fused = model.set_backend("hip", stem="hip")(x).clone()
        assert (stem.calls, conv.calls) == (1, 0)
        plain = model.set_backend("hip", stem="torch")(x).clone()
        assert (stem.calls, conv.calls) == (1, 1)
    assert not torch.equal(fused, plain) and rel_fro(fused, plain) <= CAP   # (another rounding order, the same function)


def test_packed_stem_follows_the_parameters(model):
    x = _randn((2, 3, 112, 112))
    model.set_backend("hip", stem="hip")
    with torch.no_grad():
        y0, s0 = model(x).clone(), model.stem_nhwc(x).float()
        model.conv1.weight.mul_(-0.5)                                 # in place: the version counter moves
        y1, s1 = model(x).clone(), model.stem_nhwc(x).float()
        want1 = model.set_backend("torch", stem="torch")(x)
        # relu(-a / 2) for relu(a): the stem's map is another one; a stale image would return y0's bits.  (The pooled
        # features move less: the later BatchNorms renormalise.)
        assert rel_fro(s1, s0) > 0.1 and not torch.equal(y1, y0) and rel_fro(y1, want1) <= CAP
        assert rel_fro(s1.permute(0, 3, 1, 2), model.stem(x)) <= CAP
        other = bu.resformer("torch", seed=99).state_dict()           # a second state dict: the load hook
        model.load_state_dict(other)
        want2 = model(x)
        y2 = model.set_backend("hip", stem="hip")(x)
        assert rel_fro(y2, y1) > 0.1 and rel_fro(y2, want2) <= CAP
        model.load_state_dict(bu.resformer("torch").state_dict())      # back to the module fixture's weights
        assert torch.equal(model(x), y0)


def test_hip_paths_refuse_to_cut_a_graph(model, audio):
    for m, x in ((model.set_backend("hip", stem="hip"), _randn((2, 3, 112, 112))), (audio.set_backend("hip"), _randn((2, 1, 64, 130)))):
        assert any(p.requires_grad for p in m.parameters())
        with pytest.raises(RuntimeError, match="forward-only: it computes no gradients"):
            m(x)
        with torch.no_grad():
            y = m(x)
        flags = [p.requires_grad for p in m.parameters()]
        try:
            for p in m.parameters():
                p.requires_grad_(False)
            assert torch.equal(m(x), y)                               # every parameter frozen: runs with grad mode on
            with pytest.raises(RuntimeError, match="forward-only"):
                m(x.clone().requires_grad_(True))
        finally:
            for p, f in zip(m.parameters(), flags):
                p.requires_grad_(f)


@pytest.mark.parametrize("which", ["resformer", "audio_model"])
def test_captured_forward_replays_bit_for_bit(model, audio, which):
    m, shape = (model.set_backend("hip", stem="hip"), (2, 3, 112, 112)) if which == "resformer" else (audio.set_backend("hip"), (2, 1, 64, 130))
    static_x = _randn(shape)
    with torch.no_grad():
        eager = m(static_x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                m(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(static_x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        x2 = _randn(shape, seed=6)
        static_x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, m(x2))


def test_avformer_on_both_frozen_streams_keeps_the_contract(A):
    torch.manual_seed(4)
    m = A.build_model("avformer", task="AU", video_backbone="resnet18_frozen_fused", audio_backbone="resnet18_frozen")
    bu.randomize_batchnorm(m.video_model, 8)
    bu.randomize_batchnorm(m.audio_model, 9)
    m = m.cuda().eval()
    for stream in (m.video_model, m.audio_model):                     # avformer.py:78-85
        for p in stream.parameters():
            p.requires_grad_(False)
    g = torch.Generator().manual_seed(9)
    batch = {"clip": torch.randn(2, 3, 16, 112, 112, generator=g).cuda(), "audio_features": torch.randn(2, 1, 64, 1001, generator=g).cuda()}
    with torch.no_grad():
        out = m(batch)
        m.video_model.video_model.s_former.set_backend("torch", stem="torch")
        m.audio_model.audio_model.set_backend("torch")
        want = m(batch)
    assert out.shape == want.shape == (2, 21) and bool(torch.isfinite(out).all()) and bool((out[:, 12:] == 0).all())
    assert float(want[:, :12].abs().mean()) > 1e-3
    err = rel_fro(out, want)
    print(f"STEMMODSTAT avformer both streams rel_fro {err:.3e}")
    assert err <= CAP
