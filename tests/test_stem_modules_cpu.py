"""CPU (no GPU needed): the stem of ``FrozenResFormer`` on its defining torch backend reproduces the reference's fixture (G21,
tests/golden/make_golden_stem.py); ``FrozenAudioModel`` carries torchvision's ResNet18 state_dict schema (written out below:
torchvision is not a dependency) and loads the reference's audio checkpoints; the registry takes the new names; the stem kernel's
host-side entry points exist and answer; nothing behind ``stem="hip"`` / ``backend="hip"`` falls back to the CPU.

``FrozenAudioModel`` is held to its own torch backend (tests/test_gpu_stem_modules.py): no reference fixture pins it, because
the reference builds its AudioModel from torchvision, which is not installed where the fixtures are generated."""
import ctypes
import importlib
import os

import pytest
import torch

import avformer_amd as A
from conftest import load_golden, split_golden


def g21():
    """-> (state dict of conv1 / bn1, input [2, 3, 37, 29], the reference's output [2, 64, 10, 8])"""
    p, _, r = split_golden(load_golden("g21_stem"))
    sd = {k: (torch.as_tensor(v, dtype=torch.long) if k.endswith("num_batches_tracked") else v) for k, v in p.items()}
    return sd, r["x"], r["y"]


def test_g21_stem_on_the_torch_backend_reproduces_the_reference_fixture():
    sd, x, want = g21()
    assert set(sd) == {"conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked"}
    m = A.FrozenResFormer()
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    for train in (False, True):  # "frozen": train() does not switch the BatchNorm to batch statistics
        m.train(train)
        with torch.no_grad():
            got = m.stem(x)
        assert got.shape == want.shape == (2, 64, 10, 8)
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert float((want == 0).float().mean()) < 0.5 and float(want.abs().mean()) > 0.1


def _resnet18_schema(in_channels=1):
    """torchvision.models.resnet18().state_dict() without fc.*: [(key, shape)] in order"""
    def bn(prefix, n):
        return [(prefix + ".weight", (n,)), (prefix + ".bias", (n,)), (prefix + ".running_mean", (n,)), (prefix + ".running_var", (n,)),
                (prefix + ".num_batches_tracked", ())]
    out = [("conv1.weight", (64, in_channels, 7, 7))] + bn("bn1", 64)
    inplanes = 64
    for i, planes in enumerate((64, 128, 256, 512), start=1):
        for b in range(2):
            p = f"layer{i}.{b}"
            out += [(p + ".conv1.weight", (planes, inplanes if b == 0 else planes, 3, 3))] + bn(p + ".bn1", planes)
            out += [(p + ".conv2.weight", (planes, planes, 3, 3))] + bn(p + ".bn2", planes)
            if b == 0 and inplanes != planes:
                out += [(p + ".downsample.0.weight", (planes, inplanes, 1, 1))] + bn(p + ".downsample.1", planes)
        inplanes = planes
    return out


def test_audio_model_state_dict_is_resnet18_under_resnet():
    sd = A.FrozenAudioModel().state_dict()
    want = [("resnet." + k, s) for k, s in _resnet18_schema(1)]
    assert len(want) == 120
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want


def test_audio_model_torch_backend_shapes_and_frozen_batchnorm():
    torch.manual_seed(3)
    m = A.FrozenAudioModel()
    x = torch.randn(2, 1, 64, 130)
    with torch.no_grad():
        y = m.eval()(x)
        assert y.shape == (2, 512) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
        assert torch.equal(m.train()(x), y)
    assert m.modes == ["audio_features"] and isinstance(m.resnet.fc, torch.nn.Identity)


def test_audio_checkpoint_with_prefixes_and_stray_fc_keys_loads(tmp_path):
    """an AudioFormer checkpoint as the reference saves it - DataParallel's ``module.`` in front of ``audio_model.resnet.*``, the
    22-way fc of audio.py:26-27 still inside - lands on every key of the ResNet18, both into an AudioFormer (the default renames)
    and into a bare FrozenAudioModel (checkpoint.AUDIO_MODEL_RENAMES); the fc keys are reported and skipped (strict=False)"""
    torch.manual_seed(11)
    src = A.FrozenAudioModel()
    with torch.no_grad():
        src.resnet.bn1.running_mean.normal_()
    ckpt = {"module.audio_model." + k: v.clone() for k, v in src.state_dict().items()}
    ckpt["module.audio_model.resnet.fc.1.weight"] = torch.zeros(22, 512)
    ckpt["module.audio_model.resnet.fc.1.bias"] = torch.zeros(22)
    path = os.path.join(tmp_path, "audio.pth")
    torch.save(ckpt, path)
    former = A.models.AudioFormer(backbone="resnet18_frozen")
    assert isinstance(former.audio_model, A.FrozenAudioModel) and former.audio_model.backend == "hip"
    res = A.checkpoint.load_pretrain(former, path, freeze=True)
    assert sorted(res.unexpected_keys) == ["audio_model.resnet.fc.1.bias", "audio_model.resnet.fc.1.weight"]
    assert all(k.startswith("au_head.") for k in res.missing_keys)
    got = former.audio_model.state_dict()
    assert all(torch.equal(got[k], v) for k, v in src.state_dict().items())
    assert not any(p.requires_grad for p in former.parameters())
    bare = A.FrozenAudioModel()
    res = A.checkpoint.load_pretrain(bare, path, renames=A.checkpoint.AUDIO_MODEL_RENAMES)
    assert not res.missing_keys and sorted(res.unexpected_keys) == ["resnet.fc.1.bias", "resnet.fc.1.weight"]
    assert all(torch.equal(bare.state_dict()[k], v) for k, v in src.state_dict().items())


def test_registry_accepts_the_fused_backbone_and_the_audio_backbone():
    fm = importlib.import_module(A.__name__ + ".former_models")  # (under the package's own name: one copy of its classes)
    assert fm.FROZEN_BACKBONES == ("resnet18_frozen", "resnet18_frozen_fused")
    for name, attr in (("sformer", "base_model"), ("vformer", "video_model.s_former"), ("tformer", "video_model.s_former")):
        m = A.build_model(name, modality="A;V", task="AU", backbone="resnet18_frozen_fused")
        s = m.get_submodule(attr)
        assert isinstance(s, A.FrozenResFormer) and s.backend == "hip" and s.stem_backend == "hip" and m.has_backbone
        plain = A.build_model(name, modality="A;V", task="AU", backbone="resnet18_frozen").get_submodule(attr)
        assert plain.stem_backend == "torch" and list(plain.state_dict()) == list(s.state_dict())
    assert A.build_model("sformer", modality="A;V;M", backbone="resnet18_frozen_fused").base_model.conv1.in_channels == 4
    av = A.build_model("avformer", video_backbone="resnet18_frozen_fused", audio_backbone="resnet18_frozen")
    assert av.video_model.video_model.s_former.stem_backend == "hip"
    assert isinstance(av.audio_model.audio_model, A.FrozenAudioModel) and av.audio_model.audio_model.backend == "hip"
    assert "audio_model.audio_model.resnet.layer4.1.bn2.running_var" in av.state_dict()
    with pytest.raises(ValueError, match="resnet18_frozen"):
        A.build_model("avformer", audio_backbone="resnet50")
    with pytest.raises(ValueError, match="resnet18_frozen"):
        A.build_model("avformer", video_backbone="resnet18_fused")
    plain = A.build_model("avformer")                                  # the defaults are unchanged
    assert isinstance(plain.audio_model.audio_model, torch.nn.Identity) and isinstance(plain.video_model.video_model, torch.nn.Identity)
    assert A.FrozenResFormer().stem_backend == "torch" and A.FrozenVideoModel().s_former.stem_backend == "torch"


def test_stem_hip_needs_the_hip_backend():
    with pytest.raises(ValueError, match="needs backend='hip'"):
        A.FrozenResFormer(backend="torch", stem="hip")
    with pytest.raises(ValueError, match="stem must be one of"):
        A.FrozenResFormer(backend="hip", stem="triton")
    m = A.FrozenResFormer(backend="hip", stem="hip")
    with pytest.raises(ValueError, match="needs backend='hip'"):
        m.set_backend("torch")                                          # stem=None keeps the stem: it cannot stay on hip
    assert (m.backend, m.stem_backend) == ("hip", "hip")                # a refused switch changes nothing
    m.set_backend("torch", stem="torch")
    assert (m.backend, m.stem_backend) == ("torch", "torch") and not any(b.backend != "torch" for b in m.modules() if isinstance(b, A.FrozenBasicBlock))
    m.set_backend("hip")
    assert (m.backend, m.stem_backend) == ("hip", "torch")
    with pytest.raises(ValueError, match="backend"):
        A.FrozenAudioModel(backend="triton")


def test_hip_paths_have_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.FrozenResFormer(backend="hip", stem="hip")(torch.zeros(1, 3, 112, 112))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.FrozenAudioModel(backend="hip")(torch.zeros(1, 1, 64, 130))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ops.stem_nchw(torch.zeros(1, 3, 8, 8), torch.zeros(64, 192, dtype=torch.bfloat16), torch.ones(64), torch.zeros(64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ops.stem_pack_weight(torch.zeros(64, 3, 7, 7), *[torch.ones(64) for _ in range(4)])


def test_stem_entry_points_exist_and_the_host_side_ones_answer():
    A._build.build()
    lib = A._lib.load()
    for name in ("avf_stem_packed_k", "avf_stem_pack_weight", "avf_stem_nchw", "avf_stem_plan"):
        assert hasattr(lib, name) and name in A._lib.SIGNATURES, name
    assert [A.ops.stem_packed_k(c) for c in (1, 3, 4)] == [64, 192, 224]   # Cin * 7 rows of 8, rounded up to the MFMA's 32
    with pytest.raises(RuntimeError, match="1, 3 or 4 input channels"):
        A.ops.stem_packed_k(2)
    plan = A.ops.stem_plan(2, 1, 64, 1001)
    assert plan["tile_h"] >= 1 and plan["tile_w"] >= 1
    th, tw = ctypes.c_int(), ctypes.c_int()
    assert lib.avf_stem_plan(2, 2, 64, 64, ctypes.byref(th), ctypes.byref(tw)) != 0
    assert lib.avf_stem_plan(2, 3, 0, 64, ctypes.byref(th), ctypes.byref(tw)) != 0
    assert A.ops.stem_out_hw(64, 1001) == (16, 251) and A.ops.stem_out_hw(112, 112) == (28, 28) and A.ops.stem_out_hw(1, 1) == (1, 1)
