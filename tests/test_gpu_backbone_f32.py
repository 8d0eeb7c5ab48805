"""-m gpu: the frozen backbone in parity mode at the module level - ``conv_dtype="f32"`` (csrc/conv_f32.hip: fp32 maps, bf16x3
products) on ``FrozenBasicBlock`` / ``FrozenResFormer`` / ``FrozenAudioModel`` / ``FrozenVideoModel``, against the reference's
fixture (G20) and against the modules' own defining ``backend="torch"``, never against the hip path itself.

Three caps on each of the three cases, all on the relative Frobenius error:
  (a) <= 1e-3: the parity contract;
  (b) <= 3 x the value measured on an MI355X for that case, tests/golden/conv_f32_measured.json (the project's calibration rule);
  (c) <= 1 / 16 of what ``conv_dtype="bf16"`` shows on the same input in the same test: a path that still rounds one map or one
      operand to bf16 lands within about 2 x of the bf16 figure; bf16x3's worst case per product is 3 * 2^-16 against bf16's
      2^-8, so a sixteenth separates the two with room for the fp32 floor of the torch backend."""
import json
import os

import pytest
import torch

import backbone_util as bu
from conftest import GOLDEN
from gpu_util import rel_fro

pytestmark = pytest.mark.gpu

PARITY = 1e-3
MEASURED = json.load(open(os.path.join(GOLDEN, "conv_f32_measured.json")))


@pytest.fixture(scope="module")
def A():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A


@pytest.fixture(scope="module")
def model(A):
    """one FrozenResFormer in parity mode throughout (token section and conv stages); the tests switch backend and conv dtype"""
    torch.manual_seed(2020)
    m = A.FrozenResFormer(backend="hip", compute_dtype="f32", conv_dtype="f32")
    return bu.randomize_batchnorm(m, 2021).eval().cuda()


def _randn(shape, seed=5):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _caps(name, err, err_bf16):
    print(f"BACKBONEF32STAT {name} rel_fro f32 {err:.3e} bf16 {err_bf16:.3e}")
    assert err <= PARITY, f"{name}: (a) {err}"
    assert err <= 3.0 * MEASURED[name]["rel_fro"], f"{name}: (b) {err} against the measured {MEASURED[name]['rel_fro']}"
    assert err <= err_bf16 / 16.0, f"{name}: (c) {err} against bf16's {err_bf16}"


def test_g20_chain_in_parity_mode_matches_the_reference_fixture(A):
    sd, x, want = bu.g20()
    chain = bu.g20_chain("hip")
    chain.load_state_dict(sd)
    chain = chain.cuda()
    with torch.no_grad():
        bf16 = chain(x.cuda())
        for blk in chain:
            blk.set_conv_dtype("f32")
        got = chain(x.cuda())
        y = chain[0].forward_nhwc(A.backbone.to_nhwc(x.cuda(), 32, torch.float32))
    assert got.shape == want.shape and got.dtype == torch.float32
    _caps("g20_chain", rel_fro(got, want), rel_fro(bf16, want))
    # fp32 throughout, and the zero-padded channels (48 -> 64) stay exactly zero
    assert y.dtype == torch.float32 and y.shape == (2, 4, 3, 64) and bool((y[..., 48:] == 0).all())


def test_whole_module_in_parity_mode_matches_its_torch_backend(model):
    x = _randn((2, 3, 112, 112))
    with torch.no_grad():
        want = model.set_backend("torch")(x)
        got = model.set_backend("hip").set_conv_dtype("f32")(x)
        bf16 = model.set_conv_dtype("bf16")(x)
    model.set_conv_dtype("f32")
    assert got.shape == want.shape == (2, 512) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert float(want.abs().mean()) > 0.05  # the activations did not die on the way
    _caps("resformer", rel_fro(got, want), rel_fro(bf16, want))


def test_audio_model_in_parity_mode_matches_its_torch_backend(A):
    torch.manual_seed(2021)
    audio = bu.randomize_batchnorm(A.FrozenAudioModel(conv_dtype="f32"), 2022).eval().cuda()
    x = _randn((2, 1, 64, 130), seed=8)
    with torch.no_grad():
        want = audio.set_backend("torch")(x)
        got = audio.set_backend("hip")(x)
        bf16 = audio.set_conv_dtype("bf16")(x)
    assert got.shape == want.shape == (2, 512) and got.dtype == torch.float32 and float(want.abs().mean()) > 0.05
    _caps("audio_model", rel_fro(got, want), rel_fro(bf16, want))


def test_set_conv_dtype_switches_and_rebuilds(model):
    x = _randn((2, 3, 112, 112))
    blk = model.set_backend("hip").layer1[0]
    with torch.no_grad():
        y32 = model.set_conv_dtype("f32")(x).clone()
        assert blk.conv_dtype == "f32" and isinstance(blk._packed[1][0][0], tuple)              # (w_hi, w_lo)
        y16 = model.set_conv_dtype("bf16")(x).clone()
        assert blk.conv_dtype == "bf16" and blk._packed[1][0][0].dtype == torch.bfloat16        # one image
        assert 0 < rel_fro(y16, y32) < 1.5e-2
        assert torch.equal(model.set_conv_dtype("f32")(x), y32)
    with pytest.raises(ValueError, match="'bf16', 'f32'"):
        model.set_conv_dtype("fp32")
    with pytest.raises(ValueError, match="stem='hip' with conv_dtype='f32'"):
        model.set_backend("hip", stem="hip")
    assert model.conv_dtype == "f32" and model.stem_backend == "torch"


def test_packed_images_follow_the_parameters(model):
    x = _randn((2, 3, 112, 112))
    model.set_backend("hip").set_conv_dtype("f32")
    saved = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        y0 = model(x).clone()
        model.layer4[1].conv2.weight.mul_(-0.5)                      # in place: the version counter moves
        y1 = model(x).clone()
        want1 = model.set_backend("torch")(x)
        assert rel_fro(y1, y0) > 0.1 and rel_fro(y1, want1) <= PARITY
        torch.manual_seed(99)
        other = bu.randomize_batchnorm(type(model)(compute_dtype="f32"), 100).state_dict()   # a second state dict: the load hook
        model.load_state_dict(other)
        want2 = model(x)
        y2 = model.set_backend("hip")(x)
        assert rel_fro(y2, y1) > 0.1 and rel_fro(y2, want2) <= PARITY
        model.load_state_dict(saved)                                  # back to the module fixture's weights
        assert torch.equal(model(x), y0)


def test_parity_mode_refuses_to_cut_a_graph(model):
    x = _randn((2, 3, 112, 112))
    model.set_backend("hip").set_conv_dtype("f32")
    assert model.pos_embedding.requires_grad
    with pytest.raises(RuntimeError, match="forward-only: it computes no gradients"):
        model(x)
    with torch.no_grad():
        model(x)
        with pytest.raises(RuntimeError, match="forward-only"):
            with torch.enable_grad():
                model.layer1[0].forward_nhwc(torch.zeros(1, 8, 8, 64, device="cuda").requires_grad_(True))


def test_captured_forward_replays_bit_for_bit(model):
    x = _randn((2, 3, 112, 112))
    model.set_backend("hip").set_conv_dtype("f32")
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
        x2 = _randn((2, 3, 112, 112), seed=6)
        static_x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, model(x2))


def test_frame_features_on_a_five_frame_bank_runs_in_parity_mode(A):
    torch.manual_seed(77)
    m = bu.randomize_batchnorm(A.FrozenVideoModel(backend="hip", compute_dtype="f32", conv_dtype="f32"), 78).eval().cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(79)
    frames = (torch.randint(0, 192, (5, 1, 1, 3), generator=g) + torch.randint(0, 64, (5, 112, 112, 3), generator=g)).clamp(1, 255)
    bank = A.frames.FrameBank(frames.to(torch.uint8), torch.zeros(5, dtype=torch.int32)).to("cuda")
    fe = A.clip.ClipFrontEnd(layout="tchw", channels=3, backend="hip").cuda()
    got = m.frame_features(bank, fe, chunk=3)
    m.s_former.set_backend("torch")
    want = m.frame_features(bank, fe, chunk=3)
    assert got.features.shape == (5, 512) and got.features.dtype == torch.float32 and bool(torch.isfinite(got.features).all())
    err, err_black = rel_fro(got.features, want.features), rel_fro(got.black, want.black)
    print(f"BACKBONEF32STAT frame_features rel_fro {err:.3e} black {err_black:.3e}")
    assert err <= PARITY and err_black <= PARITY
