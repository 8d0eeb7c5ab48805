"""CPU (no GPU needed): the modules of vggface2.py in their defining ``backend="torch"`` form reproduce the reference's own
``Bottleneck`` chain and ceil-mode stem (fixtures G22, tests/golden/make_golden_vggformer.py), ``VGGFormer`` keeps the reference's
state_dict schema and freezes what the reference freezes, ``load_pretrain_vgg`` reads the VGGFace2 pickle format, the registry
builds ``vggformer`` for the three modalities, and nothing behind ``backend="hip"`` falls back to the CPU."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import avformer_amd as A
import vggformer_util as vu
from conftest import GOLDEN


def test_bottleneck_chain_reproduces_the_reference_fixture():
    sd, x, want = vu.g22_chain_fixture()
    chain = vu.g22_chain("torch")
    res = chain.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    got = chain(x)
    assert got.shape == want.shape == (2, 128, 4, 3) and float((want != 0).float().mean()) >= 0.25
    # the same fp32 ops as the reference's: fp32 round-off of sums of up to 9 * 32 products of order 1 at most (a different CPU
    # or thread count may order the sums differently)
    err = float((got.detach() - want).abs().max())
    print(f"G22 chain, torch backend: max abs error {err:.3e}")
    assert err <= 1e-5
    assert torch.equal(chain.train()(x), chain.eval()(x))       # BatchNorm keeps using its running statistics


def test_stem_reproduces_the_reference_fixture():
    sd, pairs = vu.g22_stem_fixture()
    m = A.FrozenVGGFace2(layers=(1, 1, 1, 1))
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and not any(k.startswith(("conv1.", "bn1.")) for k in res.missing_keys)
    assert m.maxpool.ceil_mode and m.maxpool.padding == 0
    for x, want in pairs:
        got = m.train().stem(x)
        assert got.shape == want.shape and tuple(got.shape[2:]) == A.ops.stem_out_hw(*x.shape[2:], pool="ceil")
        err = float((got.detach() - want).abs().max())
        print(f"G22 stem {tuple(x.shape)}, torch backend: max abs error {err:.3e}")
        assert err <= 1e-5


def test_vggformer_state_dict_is_the_references():
    with open(os.path.join(GOLDEN, "g22_vggformer_keys.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)]
    sd = A.VGGFormer().state_dict()
    assert len(want) == 331 and [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert want[0][0] == "pos_embedding" and tuple(sd["conv.weight"].shape) == (512, 2048, 1, 1)


def test_the_extractor_is_frozen_and_the_rest_trains():
    m = A.VGGFormer()
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen == {n for n, _ in m.named_parameters() if n.startswith("VGG_model.")} and len(frozen) == 159
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert {"conv.weight", "pos_embedding"} <= trainable and all(n.startswith("spatial_transformer.") for n in trainable - {"conv.weight", "pos_embedding"})
    # the reference's initialisation (vggformer.py:79-85)
    w = m.VGG_model.layer3[0].conv2.weight
    assert abs(float(w.std()) - (2.0 / (9 * 256)) ** 0.5) < 2e-3 and float(m.VGG_model.layer1[0].bn3.weight.min()) == 1.0


def test_load_pretrain_vgg_reads_the_pickle_of_numpy_arrays(tmp_path):
    m = A.VGGFormer()
    g = np.random.default_rng(0)
    weights = {"conv1.weight": g.standard_normal((64, 3, 7, 7)).astype(np.float32),
               "bn1.running_mean": g.standard_normal(64).astype(np.float32),
               "layer4.2.conv3.weight": g.standard_normal((2048, 512, 1, 1)).astype(np.float32),
               "fc.weight": g.standard_normal((8631, 8)).astype(np.float32)}   # the classifier of resnet50_ft: no counterpart
    path = os.path.join(tmp_path, "resnet50_ft_weight.pkl")
    with open(path, "wb") as f:
        pickle.dump(weights, f, protocol=2)
    before = m.VGG_model.layer1[0].conv1.weight.clone()
    res = m.load_pretrain_vgg(path)
    assert res.unexpected_keys == ["fc.weight"] and "layer1.0.conv1.weight" in res.missing_keys
    sd = m.VGG_model.state_dict()
    for k in ("conv1.weight", "bn1.running_mean", "layer4.2.conv3.weight"):
        assert torch.equal(sd[k], torch.from_numpy(weights[k]))
    assert torch.equal(m.VGG_model.layer1[0].conv1.weight, before)
    assert not any(p.requires_grad for p in m.VGG_model.parameters())


def test_extractor_activations_neither_die_nor_blow_up():
    """the weights the GPU test compares the backends on: every stage of the torch backend keeps its activations of order 1"""
    m = vu.extractor("torch")
    with torch.no_grad():
        h = m.stem(vu.frames())
        assert tuple(h.shape) == (2, 64, 28, 28)
        for stage in (m.layer1, m.layer2, m.layer3, m.layer4):
            h = stage(h)
            std, dead = float(h.std()), float((h == 0).float().mean())
            assert 0.1 < std < 10.0 and dead < 0.7, (std, dead)
    assert tuple(h.shape) == (2, 2048, 4, 4)


def test_registry_builds_vggformer_for_the_three_channel_counts():
    for modality, channels in (("A;V", 3), ("A;V;M", 4), ("M", 1)):
        m = A.build_model("vggformer", modality=modality, task="AU")
        s = m.video_model.s_former
        assert isinstance(s, A.VGGFormer) and s.backend == "hip" and s.stem_backend == "hip" and m.num_channels == channels
        assert s.VGG_model.conv1.in_channels == channels and isinstance(m.video_model.t_former, A.TFormer)
        assert m.modes == ["clip"] and m.task == "AU" and hasattr(m, "get_au_loss")
    sd = m.state_dict()
    assert tuple(sd["video_model.t_former.pos_embedding"].shape) == (1, 17, 512)
    assert tuple(sd["fc.0.weight"].shape) == (256, 512) and tuple(sd["fc.3.weight"].shape) == (21, 256) and "fc.1.running_var" in sd
    assert "video_model.s_former.VGG_model.layer4.2.bn3.running_var" in sd
    assert A.models.REFERENCE_TASK_LOSSES["vggformer"] == ("ce", "bce", (2.0, 1.0))
    ref = A.build_model("vggformer", task="ALL", task_losses="reference")
    assert isinstance(ref.loss_EX, A.CrossEntropyEX) and isinstance(ref.loss_AU, A.AULoss) and isinstance(ref.loss_VA, A.CCCLoss)
    torch_m = A.build_model("vggformer", backend="torch", stem="torch", backbone_dtype="f32", compute_dtype="f32")
    assert torch_m.video_model.s_former.backend == "torch"
    # the registry's other entries are what they were
    assert set(A.MODEL_REGISTRY) >= {"avformer", "avformer_synthetic", "sformer", "vformer", "tformer", "vggformer"}
    with pytest.raises(KeyError):
        A.build_model("dsformer")


def test_the_fused_stem_has_no_parity_form():
    for make in (lambda: A.FrozenVGGFace2(backend="hip", stem="hip", conv_dtype="f32"),
                 lambda: A.VGGFormer(backend="hip", stem="hip", conv_dtype="f32"),
                 lambda: A.build_model("vggformer", backbone_dtype="f32"),
                 lambda: A.FrozenVGGFace2(backend="hip", stem="hip").set_conv_dtype("f32")):
        with pytest.raises(ValueError, match="no parity form"):
            make()
    with pytest.raises(ValueError, match="needs backend='hip'"):
        A.FrozenVGGFace2(backend="torch", stem="hip")
    assert A.build_model("vggformer", backbone_dtype="f32", stem="torch").video_model.s_former.conv_dtype == "f32"
    assert A.FrozenVGGFace2(backend="hip", stem="torch", conv_dtype="f32").layer2[0].conv_dtype == "f32"
    with pytest.raises(ValueError, match="conv_dtype"):
        A.FrozenBottleneck(64, 16, conv_dtype="f16")


def test_hip_backend_has_no_cpu_fallback():
    sd, x, _ = vu.g22_chain_fixture()
    chain = vu.g22_chain("hip")
    chain.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chain(x)
    for stem in ("torch", "hip"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.FrozenVGGFace2(backend="hip", stem=stem)(torch.zeros(1, 3, 112, 112))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.VGGFormer(backend="hip", stem=stem)(torch.zeros(1, 3, 112, 112))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.VGGFormer(backend="torch")(torch.zeros(1, 3, 112, 112))            # the token section is the HIP Transformer either way
    with pytest.raises(ValueError, match="backend"):
        A.FrozenBottleneck(64, 16, backend="triton")


def test_the_blocks_share_one_base_and_basicblock_is_what_it_was():
    _FrozenBlock = A.backbone._FrozenBlock
    assert issubclass(A.FrozenBottleneck, _FrozenBlock) and issubclass(A.FrozenBasicBlock, _FrozenBlock)
    for name in ("_pack", "_state_key", "refresh_weights", "set_conv_dtype", "_load_from_state_dict", "forward_nhwc", "forward"):
        assert getattr(A.FrozenBottleneck, name) is getattr(A.FrozenBasicBlock, name) is getattr(_FrozenBlock, name), name
    assert A.backbone.CONV_DTYPES == ("bf16", "f32")
    assert A.former_models.FROZEN_BACKBONES == ("resnet18_frozen", "resnet18_frozen_fused")
    assert A.FrozenBasicBlock.expansion == 1 and A.FrozenBottleneck.expansion == 4
