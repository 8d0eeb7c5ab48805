"""CPU (no GPU needed): the keywords of the parity-mode backbone - ``conv_dtype`` on the frozen modules, ``backbone_dtype`` on
the registry models - validate, default to ``"bf16"``, refuse the fused stem, and leave the parameter schema alone."""
import inspect

import pytest
import torch

import avformer_amd as A
from avformer_amd import backbone as B
from avformer_amd import former_models as FM


def test_defaults_are_bf16():
    for cls in (A.FrozenBasicBlock, A.FrozenResFormer, A.FrozenAudioModel, A.FrozenVideoModel, B._FrozenResNet18):
        assert inspect.signature(cls.__init__).parameters["conv_dtype"].default == "bf16", cls.__name__
    for cls in (A.models.AudioFormer, A.models.VisualFormer, A.models.TwoStreamAuralVisualFormer, FM.SpatialFormerModel,
                FM.VisualFormerModel, FM.SpatialTemporalFormerModel):
        assert inspect.signature(cls.__init__).parameters["backbone_dtype"].default == "bf16", cls.__name__
    assert inspect.signature(B.to_nhwc).parameters["dtype"].default == torch.bfloat16
    assert B.CONV_DTYPES == ("bf16", "f32") and FM.FROZEN_BACKBONES == ("resnet18_frozen", "resnet18_frozen_fused")
    m = A.FrozenResFormer(backend="hip")
    assert m.conv_dtype == "bf16" and all(b.conv_dtype == "bf16" for b in m.modules() if isinstance(b, A.FrozenBasicBlock))
    assert A.FrozenAudioModel(backend="hip").resnet.conv_dtype == "bf16"


def test_to_nhwc_takes_a_dtype():
    x = torch.randn(2, 3, 4, 5)
    y = B.to_nhwc(x, 32, torch.float32)
    assert y.dtype == torch.float32 and y.shape == (2, 4, 5, 32) and y.is_contiguous()
    assert torch.equal(y[..., :3], x.permute(0, 2, 3, 1)) and bool((y[..., 3:] == 0).all())
    assert B.to_nhwc(x).dtype == torch.bfloat16


@pytest.mark.parametrize("bad", ["fp32", "float32", None, torch.float32, "BF16"])
def test_anything_but_the_two_strings_is_a_value_error_that_names_them(bad):
    builders = [lambda: A.FrozenBasicBlock(32, 32, conv_dtype=bad), lambda: A.FrozenResFormer(conv_dtype=bad),
                lambda: A.FrozenAudioModel(conv_dtype=bad), lambda: A.FrozenVideoModel(conv_dtype=bad),
                lambda: A.FrozenResFormer().set_conv_dtype(bad), lambda: A.FrozenAudioModel().set_conv_dtype(bad),
                lambda: A.FrozenBasicBlock(32, 32).set_conv_dtype(bad), lambda: A.FrozenVideoModel().set_conv_dtype(bad),
                lambda: A.build_model("sformer", backbone_dtype=bad),
                lambda: A.build_model("vformer", backbone="resnet18_frozen", backbone_dtype=bad),
                lambda: A.build_model("tformer", backbone_dtype=bad), lambda: A.build_model("avformer", backbone_dtype=bad),
                lambda: A.models.AudioFormer(backbone_dtype=bad), lambda: A.models.VisualFormer(backbone_dtype=bad)]
    for build in builders:
        with pytest.raises(ValueError, match=r"'bf16', 'f32'"):
            build()


def test_the_fused_stem_has_no_parity_form():
    with pytest.raises(ValueError, match=r"stem='hip' with conv_dtype='f32'"):
        A.FrozenResFormer(backend="hip", stem="hip", conv_dtype="f32")
    with pytest.raises(ValueError, match=r"stem='hip' with conv_dtype='f32'"):
        A.FrozenVideoModel(backend="hip", stem="hip", conv_dtype="f32")
    m = A.FrozenResFormer(backend="hip", stem="hip")
    with pytest.raises(ValueError, match=r"stem='hip' with conv_dtype='f32'"):
        m.set_conv_dtype("f32")
    assert m.conv_dtype == "bf16" and m.layer1[0].conv_dtype == "bf16"
    m = A.FrozenResFormer(backend="hip", conv_dtype="f32")
    with pytest.raises(ValueError, match=r"stem='hip' with conv_dtype='f32'"):
        m.set_backend("hip", stem="hip")
    assert m.stem_backend == "torch"
    for name, kw in (("sformer", "backbone"), ("vformer", "backbone"), ("tformer", "backbone"), ("avformer", "video_backbone")):
        with pytest.raises(ValueError, match=r"resnet18_frozen_fused.*backbone_dtype='f32'.*stem='hip' with conv_dtype='f32'"):
            A.build_model(name, backbone_dtype="f32", **{kw: "resnet18_frozen_fused"})


def test_set_conv_dtype_reaches_every_block_and_drops_nothing_else():
    m = A.FrozenVideoModel(backend="hip")
    assert m.set_conv_dtype("f32") is m and m.s_former.conv_dtype == "f32"
    assert all(b.conv_dtype == "f32" for b in m.modules() if isinstance(b, A.FrozenBasicBlock))
    a = A.FrozenAudioModel(backend="hip", conv_dtype="f32")
    assert a.resnet.conv_dtype == "f32" and a.set_conv_dtype("bf16").resnet.conv_dtype == "bf16"
    blk = A.FrozenBasicBlock(32, 32, conv_dtype="f32")
    assert blk._state_key("cpu")[1] == "f32" and blk.set_conv_dtype("bf16")._state_key("cpu")[1] == "bf16"  # the cache key


@pytest.mark.parametrize("name,kw", [("sformer", dict(backbone="resnet18_frozen")), ("vformer", dict(backbone="resnet18_frozen")),
                                     ("tformer", dict(backbone="resnet18_frozen")),
                                     ("avformer", dict(video_backbone="resnet18_frozen", audio_backbone="resnet18_frozen"))])
def test_registry_builds_in_parity_mode_with_the_same_schema(name, kw):
    m32 = A.build_model(name, backbone_dtype="f32", **kw)
    m16 = A.build_model(name, **kw)
    assert list(m32.state_dict().keys()) == list(m16.state_dict().keys())
    assert all(a.shape == b.shape for a, b in zip(m32.state_dict().values(), m16.state_dict().values()))
    blocks32 = [b for b in m32.modules() if isinstance(b, A.FrozenBasicBlock)]
    blocks16 = [b for b in m16.modules() if isinstance(b, A.FrozenBasicBlock)]
    assert len(blocks32) == len(blocks16) >= 8
    assert all(b.conv_dtype == "f32" for b in blocks32) and all(b.conv_dtype == "bf16" for b in blocks16)


def test_parity_mode_has_no_cpu_fallback():
    m = A.FrozenAudioModel(backend="hip", conv_dtype="f32").eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 64, 130))
