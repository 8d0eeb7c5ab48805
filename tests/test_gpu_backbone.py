"""-m gpu: the frozen ResNet stages at the module level - ``FrozenBasicBlock`` / ``FrozenResFormer`` with ``backend="hip"``
(csrc/conv.hip) against the reference's fixture and against their own defining ``backend="torch"``.

Intermediates are stored in bf16, so the measure is the project's bf16-mode cap for outputs: relative
Frobenius error <= 1.5e-2.  Measured on an MI355X: G20 chain 2.3e-3, whole module 1.7e-3."""
import pytest
import torch

import backbone_util as bu
from gpu_util import rel_fro

pytestmark = pytest.mark.gpu

CAP = 1.5e-2


@pytest.fixture(scope="module")
def A():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A


@pytest.fixture(scope="module")
def model():
    """one FrozenResFormer on the device; the tests switch its backend"""
    return bu.resformer("torch").cuda()


def _frames(shape, seed=5):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def test_g20_chain_on_the_hip_backend_matches_the_reference_fixture(A):
    sd, x, want = bu.g20()
    chain = bu.g20_chain("hip")
    chain.load_state_dict(sd)
    chain = chain.cuda()
    with torch.no_grad():
        got = chain(x.cuda())
    assert got.shape == want.shape and got.dtype == torch.float32
    err = rel_fro(got, want)
    print(f"BACKBONESTAT g20_chain rel_fro {err:.3e}")
    assert err <= CAP
    # the zero-padded channels (48 -> 64) stay exactly zero through both blocks
    with torch.no_grad():
        y = chain[0].forward_nhwc(A.backbone.to_nhwc(x.cuda(), 32))
    assert y.shape == (2, 4, 3, 64) and bool((y[..., 48:] == 0).all())


@pytest.mark.parametrize("shape", [(2, 3, 112, 112), (1, 2, 3, 112, 112)], ids=["frames", "clip"])
def test_whole_module_hip_matches_torch_backend(model, shape):
    x = _frames(shape)
    with torch.no_grad():
        want = model.set_backend("torch")(x)
        got = model.set_backend("hip")(x)
    assert got.shape == want.shape == (2, 512) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert float(want.abs().mean()) > 0.05  # the activations did not die on the way
    err = rel_fro(got, want)
    print(f"BACKBONESTAT resformer {shape} rel_fro {err:.3e}")
    assert err <= CAP


def test_packed_weights_follow_the_parameters(model):
    x = _frames((2, 3, 112, 112))
    model.set_backend("hip")
    with torch.no_grad():
        y0 = model(x).clone()
        model.layer4[1].conv2.weight.mul_(-0.5)                      # in place: the version counter moves
        y1 = model(x).clone()
        want1 = model.set_backend("torch")(x)
        assert rel_fro(y1, y0) > 0.1 and rel_fro(y1, want1) <= CAP
        other = bu.resformer("torch", seed=99).state_dict()          # a second state dict: the load hook
        model.load_state_dict(other)
        want2 = model(x)
        y2 = model.set_backend("hip")(x)
        assert rel_fro(y2, y1) > 0.1 and rel_fro(y2, want2) <= CAP
        model.load_state_dict(bu.resformer("torch").state_dict())     # back to the module fixture's weights
        assert torch.equal(model(x), y0)


def test_hip_backend_refuses_to_cut_a_graph(model):
    x = _frames((2, 3, 112, 112))
    model.set_backend("hip")
    assert model.pos_embedding.requires_grad
    with pytest.raises(RuntimeError, match="forward-only: it computes no gradients"):
        model(x)
    with torch.no_grad():
        y = model(x)
    flags = [p.requires_grad for p in model.parameters()]
    try:
        for p in model.parameters():
            p.requires_grad_(False)
        assert torch.equal(model(x), y)                               # every parameter frozen: runs with grad mode on
        with pytest.raises(RuntimeError, match="forward-only"):
            model(x.clone().requires_grad_(True))
    finally:
        for p, f in zip(model.parameters(), flags):
            p.requires_grad_(f)


def test_captured_forward_replays_bit_for_bit(model):
    x = _frames((2, 3, 112, 112))
    model.set_backend("hip")
    static_x = x.clone()
    with torch.no_grad():
        eager = model(static_x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(static_x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        x2 = _frames((2, 3, 112, 112), seed=6)
        static_x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, model(x2))


def test_avformer_video_stream_on_the_frozen_backbone(A):
    torch.manual_seed(4)
    m = A.build_model("avformer", task="AU", video_backbone="resnet18_frozen")
    bu.randomize_batchnorm(m.video_model, 8)
    m = m.cuda().eval()
    for stream in (m.video_model, m.audio_model):                     # avformer.py:78-85
        for p in stream.parameters():
            p.requires_grad_(False)
    g = torch.Generator().manual_seed(9)
    batch = {"clip": torch.randn(2, 3, 16, 112, 112, generator=g).cuda(), "audio_features": torch.randn(2, 512, generator=g).cuda()}
    out = m(batch)
    assert out.shape == (2, 21) and bool(torch.isfinite(out).all()) and bool((out[:, 12:] == 0).all())
    m.get_au_loss(out, (torch.rand(2, 12, generator=g) > 0.5).float().cuda()).backward()
    with_grad = {n.split(".")[0] for n, p in m.named_parameters() if p.grad is not None}
    assert with_grad == {"au_head"}, with_grad
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.au_head.parameters())
