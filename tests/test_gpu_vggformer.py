"""-m gpu: the vggformer path at the module level - ``FrozenBottleneck`` / ``FrozenVGGFace2`` / ``VGGFormer`` (vggface2.py) and the
registry model on ``backend="hip"`` against the reference's fixture (G22) and against the modules' own defining
``backend="torch"``, never against the hip path itself.  All on the relative Frobenius error.

Caps of every forward case: the contract value - 1.5e-2 with ``conv_dtype="bf16"`` (the project's bf16 cap),
1e-3 in parity mode (``conv_dtype="f32"``, and ``compute_dtype="f32"`` for ``VGGFormer``) - and 3 x the figure measured on an
MI355X for that case, tests/golden/vggformer_measured.json (the project's calibration rule).  The G22 chain in parity mode is
also held to 1 / 16 of the bf16 figure of the same test, as tests/test_gpu_backbone_f32.py argues: a path that still rounds one
map or one operand to bf16 lands within about 2 x of the bf16 figure.

The bf16 cases run the fused stem (``stem="hip"``: the ceil-mode pool of csrc/stem.hip), the parity cases the torch stem (the
stem kernel has no parity form).  Each case prints "VGGFORMERSTAT <name> <figure>" before it asserts."""
import json
import os

import pytest
import torch

import vggformer_util as vu
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BF16_CAP, PARITY = 1.5e-2, 1e-3
MEASURED = json.load(open(os.path.join(GOLDEN, "vggformer_measured.json")))


@pytest.fixture(scope="module")
def A():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A


@pytest.fixture(scope="module")
def former_bf16(A):
    """one VGGFormer in the throughput form: conv path and token section bf16, the stem on its kernel"""
    return vu.vggformer("hip", stem="hip", conv_dtype="bf16", compute_dtype="bf16").eval().cuda()


@pytest.fixture(scope="module")
def former_f32(A):
    """one VGGFormer in parity mode throughout: torch stem, conv_dtype f32, compute_dtype f32"""
    return vu.vggformer("hip", stem="torch", conv_dtype="f32", compute_dtype="f32").eval().cuda()


def _caps(name, err, contract):
    print(f"VGGFORMERSTAT {name} rel_fro {err:.3e}")
    assert err <= contract, f"{name}: {err} against the contract {contract}"
    assert err <= 3.0 * MEASURED[name]["rel_fro"], f"{name}: {err} against the measured {MEASURED[name]['rel_fro']}"


def test_g22_chain_on_hip_matches_the_reference_fixture(A):
    sd, x, want = vu.g22_chain_fixture()
    chain = vu.g22_chain("hip")
    chain.load_state_dict(sd)
    chain = chain.cuda()
    with torch.no_grad():
        bf16 = chain(x.cuda())
        y16 = chain[0].forward_nhwc(A.backbone.to_nhwc(x.cuda(), 64))
        for blk in chain:
            blk.set_conv_dtype("f32")
        f32 = chain(x.cuda())
        y32 = chain[0].forward_nhwc(A.backbone.to_nhwc(x.cuda(), 64, torch.float32))
    assert bf16.shape == f32.shape == want.shape == (2, 128, 4, 3) and bf16.dtype == f32.dtype == torch.float32
    e16, e32 = vu.rel_fro(bf16.cpu(), want), vu.rel_fro(f32.cpu(), want)
    _caps("g22_chain_bf16", e16, BF16_CAP)
    _caps("g22_chain_f32", e32, PARITY)
    assert e32 <= e16 / 16.0, f"parity mode {e32} against bf16's {e16}"
    # NHWC maps in the mode's type, 48 -> 64 input channels zero-padded, 64 output channels (no padding to show)
    assert y16.dtype == torch.bfloat16 and y32.dtype == torch.float32 and y16.shape == y32.shape == (2, 7, 5, 64)


def test_extractor_matches_its_torch_backend(former_bf16, former_f32):
    x = vu.frames().cuda()
    for name, m, contract in (("vggface2_bf16", former_bf16.VGG_model, BF16_CAP), ("vggface2_f32", former_f32.VGG_model, PARITY)):
        stem = m.stem_backend
        with torch.no_grad():
            want = m.set_backend("torch", stem="torch")(x)
            got = m.set_backend("hip", stem=stem)(x)
            nhwc = m.forward_nhwc(x)
        assert got.shape == want.shape == (2, 2048, 4, 4) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        assert float(want.abs().mean()) > 0.05 and float((want == 0).float().mean()) < 0.7      # the activations did not die
        assert nhwc.shape == (2, 4, 4, 2048) and nhwc.dtype == (torch.bfloat16 if name.endswith("bf16") else torch.float32)
        _caps(name, vu.rel_fro(got, want), contract)


def test_vggformer_matches_its_torch_backend(former_bf16, former_f32):
    x = vu.frames().cuda()
    for name, m, contract in (("vggformer_bf16", former_bf16, BF16_CAP), ("vggformer_f32", former_f32, PARITY)):
        stem = m.stem_backend
        with torch.no_grad():
            want = m.set_backend("torch", stem="torch")(x)
            got = m.set_backend("hip", stem=stem)(x)
            got5 = m(x.view(1, 2, 3, 112, 112))
        assert got.shape == want.shape == (2, 512) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        assert float(want.abs().mean()) > 0.05 and torch.equal(got5, got)
        _caps(name, vu.rel_fro(got, want), contract)


def test_more_positions_than_patches_is_refused(A):
    m = A.VGGFormer(num_patches=9, backend="hip", stem="hip").cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="num_patches = 9"):
        m(torch.zeros(1, 3, 112, 112, device="cuda"))                      # 4 x 4 = 16 positions


def test_gradients_in_parity_mode_match_the_torch_backend(former_f32):
    m = former_f32.train()                                                   # the extractor's BatchNorm stays eval-mode
    x = vu.frames().cuda()
    grads = {}
    for backend in ("hip", "torch"):
        m.set_backend(backend, stem="torch")
        m.zero_grad(set_to_none=True)
        out = m(x)
        out.square().sum().backward()
        grads[backend] = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        assert not any(n.startswith("VGG_model.") for n in grads[backend])
        assert all(p.grad is None for p in m.VGG_model.parameters())
    m.set_backend("hip", stem="torch").eval().zero_grad(set_to_none=True)
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert set(grads["hip"]) == set(grads["torch"]) == set(trainable) and {"conv.weight", "pos_embedding"} <= set(trainable)
    worst = {n: vu.rel_fro(grads["hip"][n], grads["torch"][n]) for n in trainable}
    print("VGGFORMERSTAT gradients worst " + ", ".join(f"{n} {e:.2e}" for n, e in sorted(worst.items(), key=lambda kv: -kv[1])[:4]))
    assert len(trainable) == 13 and all(float(grads["torch"][n].abs().max()) > 0 for n in trainable)
    assert bool((grads["hip"]["pos_embedding"][:, 16:] == 0).all())           # 4 x 4 positions of the 49
    for n, e in worst.items():
        assert e <= PARITY, f"{n}: {e}"


def test_the_guard_is_on_the_input_only(former_bf16):
    m = former_bf16.set_backend("hip", stem="hip")
    x = vu.frames().cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):
        m(x)
    out = m(x.detach())                                                       # trainable parameters behind the extractor: a graph
    assert out.requires_grad
    with pytest.raises(RuntimeError, match="forward-only"):
        with torch.enable_grad():
            m.VGG_model.layer1[0].forward_nhwc(torch.zeros(1, 8, 8, 64, device="cuda").requires_grad_(True))


def test_packed_images_follow_an_in_place_weight_change(A):
    sd, x, _ = vu.g22_chain_fixture()
    chain = vu.g22_chain("hip")
    chain.load_state_dict(sd)
    chain, x = chain.cuda(), x.cuda()

    def torch_backend():
        for blk in chain:
            blk.backend = "torch"
        y = chain(x)
        for blk in chain:
            blk.backend = "hip"
        return y

    with torch.no_grad():
        y0 = chain(x).clone()
        key0 = chain[1]._packed[0]
        chain[1].conv2.weight.mul_(-0.5)                                      # in place: the version counter moves
        chain[2].bn3.running_var.add_(0.25)
        y1 = chain(x).clone()
        assert chain[1]._packed[0] != key0 and vu.rel_fro(y1, y0) > 0.05 and vu.rel_fro(y1, torch_backend()) <= BF16_CAP
        chain.load_state_dict(sd)                                             # the load hook
        assert chain[1]._packed is None and torch.equal(chain(x), y0)
        chain[0].conv1.weight.data.mul_(2.0)                                  # through .data: the counters do not see it
        assert torch.equal(chain(x), y0)
        chain[0].refresh_weights()
        y2 = chain(x)
        assert not torch.equal(y2, y0) and vu.rel_fro(y2, torch_backend()) <= BF16_CAP


def test_captured_eval_forward_replays_bit_for_bit(former_bf16):
    m = former_bf16.set_backend("hip", stem="hip").eval()
    static_x = vu.frames().cuda()
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
        x2 = vu.frames(seed=6).cuda()
        static_x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, m(x2))


@pytest.fixture(scope="module")
def task_model(A):
    torch.manual_seed(11)
    m = A.build_model("vggformer", modality="A;V", task="AU")
    vu.randomise_batchnorm(m.video_model.s_former.VGG_model, torch.Generator().manual_seed(12))
    return m.cuda()


def test_registry_model_maps_a_clip_to_the_21_columns(task_model):
    clip = torch.randn(2, 3, 16, 112, 112, generator=torch.Generator().manual_seed(13)).cuda()
    with torch.no_grad():
        out = task_model.eval()({"clip": clip})
    assert out.shape == (2, 21) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())


def test_one_backward_under_task_au_reaches_every_trainable_parameter(task_model):
    m = task_model.train()
    s = m.video_model.s_former
    assert s.backend == "hip" and s.stem_backend == "hip"                     # the frozen extractor on the HIP conv path
    g = torch.Generator().manual_seed(14)
    clip = torch.randn(2, 3, 16, 112, 112, generator=g).cuda()
    y = (torch.rand(2, 12, generator=g) > 0.5).float().cuda()
    m.zero_grad(set_to_none=True)
    loss = m.get_au_loss(m({"clip": clip}), y)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for n, p in m.named_parameters():
        if n.startswith("video_model.s_former.VGG_model."):
            assert not p.requires_grad and p.grad is None, n
        else:
            assert p.requires_grad and p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    m.zero_grad(set_to_none=True)
