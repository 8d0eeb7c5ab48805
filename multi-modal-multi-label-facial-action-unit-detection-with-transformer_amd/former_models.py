"""The other ``*former`` entries of the reference's model registry (train.py:292-303): ``sformer`` (SpatialFormer,
sformer.py:338-382), ``vformer`` (VisualFormer, vformer.py:295-387) and ``tformer`` (SpatialTemporalFormer,
tformer.py:296-436), assembled from the token sections this package builds on the HIP path - ``ResFormerTokens``
(sformer.py:313-327), ``TFormer`` (vformer.py:270-293), ``AU_former`` / ``tformer_AU_head`` - around a caller-supplied
CNN backbone.

The ResNet stages of the reference's ``ResFormer`` are conv-bound and out of scope: ``backbone=``
takes them as two modules, ``stem`` (frames [B', C, H, W] -> stage-3 feature map [B', 256, 7, 7]) and ``tail`` (feature map
-> pooled features [B', 512]); ``ResFormerShell`` runs the token section between them exactly where ``ResFormer.forward``
does.  Without a backbone the models consume what the backbone would produce (a [B', 256, 7, 7] map, ``tail`` = global
average pool + a fixed channel tiling to 512 features), which is enough to drive the token path, the heads and the
[B, 21] output contract.  ``backbone="resnet18_frozen"`` builds the stages themselves: ``backbone.FrozenResFormer``, the reference's whole
``ResFormer`` in eval mode on the HIP conv kernels (csrc/conv.hip): forward only by default, and with ``train_tokens=True`` differentiated through the frozen ``layer4`` (csrc/conv_dgrad.hip) so that its token section trains.  Module / parameter names follow the reference so that its checkpoints load with strict=False.
The small ``fc`` heads (BatchNorm1d / Linear) are plain PyTorch modules - plumbing either side of the hot path.

``vggformer`` (VGGVisualFormer, vggformer.py:323-421) is the fifth entry: ``VGGVisualFormerModel`` owns its backbone - the frozen
VGGFace2 ResNet-50 of ``vggface2.VGGFormer`` on the HIP conv path - and, because everything trainable sits behind that backbone's
last convolution, trains there."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import nn

from .heads import AU_former, ResFormerTokens, TFormer, VA_former, tformer_AU_head
from .models import REFERENCE_TASK_LOSSES, _TaskLossMixin


class _PoolTile(nn.Module):
    """stand-in for ResNet stage 4 + avgpool when no backbone is given: [B', C, h, w] -> [B', 512]"""

    def __init__(self, out_features=512):
        super().__init__()
        self.out_features = out_features

    def forward(self, x):
        f = x.mean(dim=(2, 3))
        rep = -(-self.out_features // f.shape[1])
        return f.repeat(1, rep)[:, :self.out_features]


class ResFormerShell(ResFormerTokens):
    """``ResFormer.forward`` (sformer.py:300-337) with the conv stages supplied by the caller:
    ``x[B, T, C, H, W] -> view(-1, C, H, W) -> stem -> token section (HIP) -> tail -> [B*T, 512]``.  Subclass of the token
    section, so its parameters carry the reference's names (``base_model.pos_embedding``, ``base_model.spatial_transformer.*``)."""

    def __init__(self, backbone: Optional[Tuple[nn.Module, nn.Module]] = None, dropout=0.0, compute_dtype="bf16"):
        super().__init__(dropout=dropout, compute_dtype=compute_dtype)
        stem, tail = backbone if backbone is not None else (nn.Identity(), _PoolTile())
        self.stem, self.tail = stem, tail

    def forward(self, x):
        if x.dim() == 5:
            x = x.contiguous().view(-1, *x.shape[2:])        # sformer.py:301-302
        return self.tail(super().forward(self.stem(x)))


# "resnet18_frozen": the ResNet stages on the HIP conv kernel behind a torch stem; "resnet18_frozen_fused": the same module
# with stem="hip" - conv1 / bn1 / relu / maxpool as the one launch of csrc/stem.hip (1, 3 or 4 input channels)
FROZEN_BACKBONES = ("resnet18_frozen", "resnet18_frozen_fused")


def _check_backbone_dtype(backbone, backbone_dtype):
    """``backbone_dtype`` is ``"bf16"`` or ``"f32"``; the fused-stem backbone has no ``"f32"`` form"""
    from .backbone import _check_conv_dtype
    _check_conv_dtype(backbone_dtype)
    if backbone_dtype == "f32" and backbone == "resnet18_frozen_fused":
        raise ValueError("backbone='resnet18_frozen_fused' with backbone_dtype='f32': that is stem='hip' with conv_dtype='f32', and "
                         "the stem kernel (csrc/stem.hip) has no parity form; use backbone='resnet18_frozen'")
    return backbone_dtype


def _s_former(backbone, num_channels=3, backbone_dtype="bf16", train_tokens=False, **kw):
    """the S-Former of a ``*former`` model: ``backbone=None`` or a ``(stem, tail)`` pair -> ``ResFormerShell``;
    ``backbone="resnet18_frozen"`` -> ``backbone.FrozenResFormer`` on the HIP conv kernels (eval-mode stages; forward only unless ``train_tokens=True``, which
    trains ``pos_embedding`` and ``spatial_transformer`` behind the frozen stages), whose
    ``conv1`` takes the ``num_channels`` channels the modality selects (vformer.py:313-331); ``"resnet18_frozen_fused"`` -> the
    same with the stem on its HIP kernel too.  ``backbone_dtype``: ``"bf16"`` (default) or ``"f32"``, the frozen module's
    ``conv_dtype`` - ``"f32"`` runs its conv stages in the parity arithmetic (csrc/conv_f32.hip) and has no fused-stem form"""
    _check_backbone_dtype(backbone, backbone_dtype)
    if isinstance(backbone, str):
        if backbone not in FROZEN_BACKBONES:
            raise ValueError(f"backbone must be None, a (stem, tail) pair or one of {FROZEN_BACKBONES}, got {backbone!r}")
        from .backbone import FrozenResFormer
        return FrozenResFormer(backend="hip", in_channels=num_channels, stem="hip" if backbone.endswith("_fused") else "torch",
                               conv_dtype=backbone_dtype, train_tokens=train_tokens, **kw)
    if train_tokens:
        raise ValueError(f"train_tokens=True is the frozen backbones' switch: backbone must be one of {FROZEN_BACKBONES}, got {backbone!r}")
    return ResFormerShell(backbone, **kw)


def _fc_head(in_features):
    return nn.Sequential(nn.BatchNorm1d(in_features), nn.Linear(in_features, 256), nn.BatchNorm1d(256), nn.Linear(256, 12 + 7 + 2))


class _FormerTask(nn.Module, _TaskLossMixin):
    num_channels = 3

    def _config(self, modality, task):
        """``config_modality`` (sformer.py:384-391, same in vformer / tformer): RGB + mask -> the last 4 channels of the
        clip, mask only -> the last one, otherwise the 3 RGB channels (the caller's stem must take that many: the reference
        rebuilds ``conv1`` there, which belongs to the backbone this package does not ship).  Tasks as in the reference: AU, EX
        and VA columns come out of the fc head, with ``sformer`` overwriting the AU / VA columns by its ``AU_former`` /
        ``VA_former`` heads (sformer.py:375-380); ``vformer`` and ``tformer`` have no VA head (their VA columns are the fc head's)."""
        if 'M' in modality:
            self.num_channels = 4 if 'V' in modality else 1

    def _select(self, x):
        clip = x['clip']
        if clip.dim() == 5 and self.has_backbone:             # [B, C, T, H, W] -> [B, T, C, H, W] (sformer.py:374-377)
            clip = clip[:, -self.num_channels:].permute(0, 2, 1, 3, 4)
        return clip


class SpatialFormerModel(_FormerTask):
    """registry name ``sformer`` (sformer.py:338-382): per-frame features -> fc head, AU logits from ``AU_former``"""

    def __init__(self, modality='A;V;M', video_pretrained=True, task='EX', backbone=None, compute_dtype="bf16", task_losses="plain",
                 backbone_dtype="bf16", train_tokens=False):
        super().__init__()
        self.has_backbone = backbone is not None
        self._config(modality, task)
        self.base_model = _s_former(backbone, self.num_channels, backbone_dtype, train_tokens, dropout=0.2, compute_dtype=compute_dtype)
        self.task, self.modes = task, ["clip"]
        self.fc = _fc_head(512)
        self.au_head = AU_former(dropout=0.2, compute_dtype=compute_dtype)
        self.va_head = VA_former(dropout=0.2, compute_dtype=compute_dtype)   # sformer.py:358
        # task_losses="plain" keeps the AULoss of the path SURVEY.md section 8 scopes; "reference" builds what the reference's
        # SpatialFormer trains with: DiceAULoss, cross-entropy and CCC (sformer.py:359-363)
        self._init_task_losses(task_losses, REFERENCE_TASK_LOSSES['sformer'])

    def forward(self, x):
        features = self.base_model(self._select(x))
        out = self.fc(features)
        if self.task == 'AU':
            au_out, _ = self.au_head(features)                 # sformer.py:382-384
            out = torch.cat([au_out[:, :12].to(out.dtype), out[:, 12:]], dim=1)
        if self.task == 'VA':
            va_out, _ = self.va_head(features)                 # sformer.py:378-380: out[:, -2:] = va_out
            out = torch.cat([out[:, :-2], va_out.to(out.dtype)], dim=1)
        return out


class _VideoModel(nn.Module):
    def __init__(self, backbone, temporal_dim, au_tokens, compute_dtype, num_channels=3, backbone_dtype="bf16", train_tokens=False):
        super().__init__()
        self.s_former = _s_former(backbone, num_channels, backbone_dtype, train_tokens, compute_dtype=compute_dtype)
        self.au_head = AU_former(dropout=0.2, compute_dtype=compute_dtype) if au_tokens else None
        self.t_former = TFormer(dim=temporal_dim, compute_dtype=compute_dtype)

    def forward(self, x):
        x = self.s_former(x)                                   # [B*16, 512]
        if self.au_head is not None:                           # tformer.py:310-313: the 12 AU tokens of every frame, flattened
            _, tok = self.au_head(x)
            x = tok.reshape(tok.shape[0], -1)                  # [B*16, 12*128]
        return self.t_former(x)                                # view(-1, 16, dim) -> cls token [B, dim]


class VisualFormerModel(_FormerTask):
    """registry name ``vformer`` (vformer.py:358-387): S-Former frames -> ``TFormer`` over 16 frames -> fc head"""

    def __init__(self, modality='A;V;M', video_pretrained=True, task='EX', backbone=None, compute_dtype="bf16", task_losses="plain",
                 backbone_dtype="bf16", train_tokens=False):
        super().__init__()
        self.has_backbone = backbone is not None
        self._config(modality, task)
        self.video_model = _VideoModel(backbone, 512, False, compute_dtype, self.num_channels, backbone_dtype, train_tokens)
        self.task, self.modes = task, ["clip"]
        self.fc = _fc_head(512)
        self._init_task_losses(task_losses, REFERENCE_TASK_LOSSES['vformer'])

    def forward(self, x):
        return self.fc(self.video_model(self._select(x)))


class _VGGVideoModel(nn.Module):
    """``VideoModel`` of vggformer.py:323-342 with its fc replaced by the identity (vggformer.py:390): ``s_former`` is a
    ``VGGFormer``, ``t_former`` a ``TFormer`` over 16 frames"""

    def __init__(self, num_channels, backend, stem, backbone_dtype, compute_dtype):
        super().__init__()
        from .vggface2 import VGGFormer
        self.s_former = VGGFormer(backend=backend, stem=stem, conv_dtype=backbone_dtype, compute_dtype=compute_dtype,
                                  in_channels=num_channels)
        self.t_former = TFormer(num_patches=16, dim=512, compute_dtype=compute_dtype)

    def forward(self, x):
        return self.t_former(self.s_former(x))                 # [B, T, C, H, W] -> [B*16, 512] -> cls token [B, 512]


class VGGVisualFormerModel(_FormerTask):
    """registry name ``vggformer`` (vggformer.py:364-421): ``VGGFormer`` frames (the frozen VGGFace2 ResNet-50, a trainable 1x1
    conv and one transformer layer over its map) -> ``TFormer`` over 16 frames -> fc head ``Linear(512, 256) - BatchNorm1d -
    ReLU - Linear(256, 21)`` (vggformer.py:384-389), plain torch like the other fc heads.

    ``backend="hip"`` (default) runs the extractor on the HIP conv path and ``stem="hip"`` (default) its stem on the stem kernel;
    the model trains there, since nothing in front of the extractor's last convolution has a gradient.  ``backbone_dtype="f32"`` is
    the parity arithmetic of the extractor and needs ``stem="torch"`` (the stem kernel has no parity form).  The VGGFace2
    weights are not loaded here (the reference reads a fixed path, vggformer.py:328): call
    ``video_model.s_former.load_pretrain_vgg(path)``; ``video_pretrained`` is accepted for the signature."""
    has_backbone = True

    def __init__(self, modality='A;V;M', video_pretrained=True, task='EX', compute_dtype="bf16", task_losses="plain",
                 backbone_dtype="bf16", backend="hip", stem="hip"):
        super().__init__()
        # The reference's config_modality (vggformer.py:344-362) reads self.s_former.conv1, which VGGFormer does not have, and
        # raises for every modality with a mask.  What it means is what sformer / vformer / tformer do: the extractor's first
        # convolution, VGG_model.conv1, takes the 4 (RGB + mask) or 1 (mask only) channels the modality selects.
        self._config(modality, task)
        self.video_model = _VGGVideoModel(self.num_channels, backend, stem, backbone_dtype, compute_dtype)
        self.task, self.modes = task, ["clip"]
        self.fc = nn.Sequential(nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Linear(256, 12 + 7 + 2))
        self._init_task_losses(task_losses, REFERENCE_TASK_LOSSES['vggformer'])

    def forward(self, x):
        return self.fc(self.video_model(self._select(x)))


class SpatialTemporalFormerModel(_FormerTask):
    """registry name ``tformer`` (tformer.py:405-436): per-frame AU tokens -> ``TFormer(dim=1536)`` -> fc head, AU logits
    from ``tformer_AU_head`` on the [B, 12, 128] view of the temporal feature"""

    def __init__(self, modality='A;V;M', video_pretrained=True, task='EX', backbone=None, compute_dtype="bf16", task_losses="plain",
                 backbone_dtype="bf16", train_tokens=False):
        super().__init__()
        self.has_backbone = backbone is not None
        self._config(modality, task)
        self.video_model = _VideoModel(backbone, 128 * 12, True, compute_dtype, self.num_channels, backbone_dtype, train_tokens)
        self.task, self.modes = task, ["clip"]
        self.au_head = tformer_AU_head(dropout=0.2, compute_dtype=compute_dtype)
        self.fc = _fc_head(128 * 12)
        self._init_task_losses(task_losses, REFERENCE_TASK_LOSSES['tformer'])

    def forward(self, x):
        f = self.video_model(self._select(x))
        out = self.fc(f)
        au = self.au_head(f)                                   # tformer.py:432-433: out[:, :12] = au_out
        return torch.cat([au[:, :12].to(out.dtype), out[:, 12:]], dim=1)
