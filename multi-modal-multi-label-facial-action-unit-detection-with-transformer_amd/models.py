"""Task models and the model registry around the HIP transformer (reference train.py:292-315,
models/avformer.py:37-123).

``TwoStreamAuralVisualFormer`` keeps the reference's constructor signature, ``.modes`` / ``.task``
attributes, ``forward(dict) -> [B,21]`` layout ([0:12] AU logits, [12:19] EX, [19:21] VA) and
``get_*_loss`` methods, so the step loop of the reference's ``train.py:206-237`` runs on it
unchanged.  Its CNN feature extractors (ResNet18 on mel-spectrograms, Former-DFER video model) are
out of scope: ``AudioFormer`` / ``VisualFormer`` take a ``backbone``
module and default to the identity, i.e. they consume per-clip feature vectors [B, 512]; ``VisualFormer(backbone="resnet18_frozen")``
/ ``TwoStreamAuralVisualFormer(video_backbone="resnet18_frozen")`` put the reference's frozen ``VideoModel`` there, its ResNet
stages on the HIP conv kernels (backbone.py), and consume clips [B, C, T, H, W] (``"resnet18_frozen_fused"``: its stem on the
HIP stem kernel too); ``AudioFormer(backbone="resnet18_frozen")`` / ``TwoStreamAuralVisualFormer(audio_backbone="resnet18_frozen")``
put the reference's frozen ``AudioModel`` (ResNet18, fc = identity) there on the same kernels and consume mel maps [B, 1, 64, 1001].

``SyntheticAVFormer`` is the BASELINE.json scale-up of the same block: video tokens [B,T_v,D] and
audio tokens [B,T_a,D] fused on the SEQUENCE axis, + positional embedding -> Transformer(D, L) ->
mean-pooled -> 12 AU logits -> AULoss.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import torch
from torch import nn

from . import ops
from .heads import AU_former, TFormer, former_AU_head, tformer_AU_head  # noqa: F401
from .loss import AULoss, CCCLoss, CrossEntropyEX, DiceAULoss, FocalLoss_Ori, MultiTaskLoss
from .transformer import Transformer


def load_pretrain(model, weight_path):
    """reference avformer.py:28-35 - strips 'module.' prefixes, strict=False; a missing file is skipped
    (the reference hard-codes K:\\ paths and would crash).  See checkpoint.py for the other loaders."""
    from .checkpoint import load_pretrain as _load
    return _load(model, weight_path) is not None


class AudioFormer(nn.Module):
    def __init__(self, modality='A', audio_pretrained=False, task='EX', backbone=None, compute_dtype="bf16", backbone_dtype="bf16"):
        super().__init__()
        from .backbone import _check_conv_dtype
        _check_conv_dtype(backbone_dtype)  # "f32": the frozen backbone's conv stages in the parity arithmetic (csrc/conv_f32.hip)
        if isinstance(backbone, str):
            # "resnet18_frozen": the reference's AudioModel (audio.py:22-39, fc = identity as in avformer.py:50) on the HIP stem and
            # conv kernels - eval-mode, forward only (backbone.py); consumes mel maps [B, 1, 64, 1001]
            if backbone != "resnet18_frozen":
                raise ValueError(f"backbone must be None, a module or 'resnet18_frozen', got {backbone!r}")
            from .backbone import FrozenAudioModel
            backbone = FrozenAudioModel(backend="hip", conv_dtype=backbone_dtype)
        self.audio_model = backbone if backbone is not None else nn.Identity()
        self.task = task
        self.modes = ['audio_features']
        self.au_head = AU_former(dropout=0.2, compute_dtype=compute_dtype)

    def forward(self, x):
        return self.au_head.tokens(self.audio_model(x))  # avformer.py:96: only the tokens of this head are used


class VisualFormer(nn.Module):
    def __init__(self, modality='A;V', video_pretrained=True, task='EX', backbone=None, in_features=512,
                 compute_dtype="bf16", backbone_dtype="bf16"):
        super().__init__()
        from .former_models import _check_backbone_dtype
        _check_backbone_dtype(backbone, backbone_dtype)  # "f32": the frozen backbone's conv stages in the parity arithmetic
        if isinstance(backbone, str):
            # "resnet18_frozen": the reference's own VideoModel (vformer.py:295-311, fc = identity as in avformer.py:61-66) with
            # its ResNet stages on the HIP conv kernels - eval-mode, forward only (backbone.py); consumes clips [B, C, T, H, W]
            # "resnet18_frozen_fused": the same with the stem on its HIP kernel too (csrc/stem.hip)
            from .former_models import FROZEN_BACKBONES
            if backbone not in FROZEN_BACKBONES:
                raise ValueError(f"backbone must be None, a module or one of {FROZEN_BACKBONES}, got {backbone!r}")
            from .backbone import FrozenVideoModel
            backbone = FrozenVideoModel(backend="hip", compute_dtype=compute_dtype, stem="hip" if backbone.endswith("_fused") else "torch",
                                        conv_dtype=backbone_dtype)
        self.video_model = backbone if backbone is not None else nn.Identity()
        self.task = task
        self.modes = ["clip"]
        self.au_head = AU_former(input_dim=in_features, compute_dtype=compute_dtype)

    def forward(self, x):
        return self.au_head.tokens(self.video_model(x))  # avformer.py:99

    def forward_bank(self, feature_bank, index, assembler):
        """``forward`` on the clips of ``index``, from a bank of per-frame S-Former features (``FrozenVideoModel.forward_bank``)"""
        if not hasattr(self.video_model, "forward_bank"):
            raise RuntimeError("VisualFormer.forward_bank needs the frozen video model: backbone='resnet18_frozen' or "
                               f"'resnet18_frozen_fused' (got {type(self.video_model).__name__})")
        return self.au_head.tokens(self.video_model.forward_bank(feature_bank, index, assembler))


# the criteria each task model of the reference owns (loss_EX, loss_AU, VA weights): avformer.py:89-91 and 122, sformer.py:359-363
# and 420, vformer.py:375-379 and 404, tformer.py:423-427 and 454
REFERENCE_TASK_LOSSES = {
    'avformer': ('focal', 'bce', (2.0, 1.0)),
    'sformer': ('ce', 'dice', (1.0, 1.0)),
    'vformer': ('ce', 'bce', (2.0, 1.0)),
    'tformer': ('ce', 'bce', (2.0, 1.0)),
    'vggformer': ('ce', 'bce', (2.0, 1.0)),   # vggformer.py:391-395 and 420: cross-entropy ignoring 7, AULoss, CCC 2 v + a
}


class _TaskLossMixin:
    """``get_au_loss`` / ``get_ex_loss`` / ``get_va_loss`` / ``get_mt_loss`` on the [B, 21] row, as train.py:136-147 calls them.

    ``task_losses="plain"`` (default): AULoss on its kernel, a plain cross-entropy and a plain-torch CCC with biased variances.
    ``task_losses="reference"``: the model owns ``loss_EX`` / ``loss_AU`` / ``loss_VA`` as its reference counterpart does
    (REFERENCE_TASK_LOSSES) and the three methods run on the fused loss kernel.  ``get_mt_loss`` uses the reference's criteria
    in either setting (sformer.py:423-449; the reference defines it for ``sformer`` only)."""
    task_losses = "plain"
    _recipe = ('ce', 'bce', (2.0, 1.0))

    def _init_task_losses(self, task_losses, recipe):
        if task_losses not in ("plain", "reference"):
            raise ValueError(f"task_losses must be 'plain' or 'reference', got {task_losses!r}")
        self.task_losses, self._recipe = task_losses, recipe
        self.loss_AU = AULoss()
        if task_losses == "reference":
            ex, au, va_weights = recipe
            self.loss_EX = FocalLoss_Ori(num_class=7, gamma=2.0, ignore_index=7, reduction='mean') if ex == 'focal' \
                else CrossEntropyEX(ignore_index=7)
            if au == 'dice':
                self.loss_AU = DiceAULoss()
            self.loss_VA = CCCLoss()
            self.loss_MT = MultiTaskLoss(self.loss_EX, self.loss_AU, self.loss_VA, va_weights)

    def _mt(self):
        mt = self._modules.get('loss_MT') or self.__dict__.get('_plain_mt')
        if mt is None:  # "plain": the reference's criteria, built on first use and kept out of the module tree
            ex, au, va_weights = self._recipe
            mt = MultiTaskLoss(FocalLoss_Ori(num_class=7, gamma=2.0, ignore_index=7) if ex == 'focal' else CrossEntropyEX(ignore_index=7),
                               DiceAULoss() if au == 'dice' else AULoss(), CCCLoss(), va_weights)
            self.__dict__['_plain_mt'] = mt
        return mt

    def _au_on_own_kernel(self):
        # an AULoss wrapped by dp.DataParallel keeps its (sum, count) collective, which lives on its own kernel
        return isinstance(self.loss_AU, AULoss) and (self.task_losses == "plain" or self.loss_AU.global_mean is not None)

    def get_au_loss(self, y_pred, y_true):
        # loss on the AU slots 0..11 of the [B,21] row (train.py:136-138 / the reference models' get_au_loss)
        if self._au_on_own_kernel():
            if y_true.dim() == 2 and y_true.shape[1] == 12 and hasattr(self.loss_AU, "forward_rows"):
                return self.loss_AU.forward_rows(y_pred, y_true)
            return self.loss_AU(y_pred[:, :12], y_true)
        return self._mt()(y_pred, y_au=y_true)[1]

    def get_ex_loss(self, y_pred, y_true):
        if self.task_losses == "reference":
            return self._mt()(y_pred, y_ex=y_true)[0]
        return nn.functional.cross_entropy(y_pred[:, 12:19], y_true.view(-1), ignore_index=7)

    def get_va_loss(self, y_pred, y_true):
        if self.task_losses == "reference":
            return self._mt()(y_pred, y_va=y_true)[2]

        def ccc_loss(p, t):
            pm, tm = p.mean(), t.mean()
            cov = ((p - pm) * (t - tm)).mean()
            return 1 - 2 * cov / (p.var(unbiased=False) + t.var(unbiased=False) + (pm - tm) ** 2 + 1e-8)
        v, a = torch.tanh(y_pred[:, 19]), torch.tanh(y_pred[:, 20])
        return 2 * ccc_loss(v, y_true[:, 0]) + ccc_loss(a, y_true[:, 1])

    def get_mt_loss(self, y_pred, y_true, normalize=False):
        """``[loss_ex, loss_au, loss_va]`` for the label dict ``{'EX', 'AU', 'VA'}`` of train.py:208-213: one launch, and one more
        in backward.  ``normalize=True`` divides each by its count of valid labels on the device (0 for a count of 0); the
        reference counts through numpy on the host."""
        return self._mt()(y_pred, y_true['EX'], y_true['AU'], y_true['VA'], normalize=normalize)


class TwoStreamAuralVisualFormer(nn.Module, _TaskLossMixin):
    def __init__(self, modality='A;V;M', video_pretrained=True, audio_pretrained=True, task='EX',
                 video_weights=None, audio_weights=None, compute_dtype="bf16", task_losses="plain", video_backbone=None,
                 audio_backbone=None, backbone_dtype="bf16"):
        super().__init__()
        # backbone_dtype="f32": both frozen streams run their conv stages in the parity arithmetic (backbone.py, conv_dtype)
        # audio_backbone="resnet18_frozen": the aural stream consumes mel maps [B, 1, 64, 1001] through the frozen ResNet18 on the
        # HIP path (backbone.FrozenAudioModel)
        self.audio_model = AudioFormer(backbone=audio_backbone, compute_dtype=compute_dtype, backbone_dtype=backbone_dtype)
        # video_backbone="resnet18_frozen" / "resnet18_frozen_fused": the video stream consumes clips through the frozen S-Former on
        # the HIP path (the second with its stem on the HIP kernel too)
        self.video_model = VisualFormer(backbone=video_backbone, compute_dtype=compute_dtype, backbone_dtype=backbone_dtype)
        if video_pretrained and load_pretrain(self.video_model, video_weights):
            for p in self.video_model.parameters():
                p.requires_grad = False
        if audio_pretrained and load_pretrain(self.audio_model, audio_weights):
            for p in self.audio_model.parameters():
                p.requires_grad = False
        self.task = task
        self.au_head = former_AU_head(emb_dim=256, dropout=0.2, compute_dtype=compute_dtype)
        self.modes = ['clip', 'audio_features']
        self._init_task_losses(task_losses, REFERENCE_TASK_LOSSES['avformer'])
        self.concurrent_streams = True
        self._side_streams = {}

    def _forward_bank(self, x):
        """``x['clip_bank'] = (feature_bank, index, assembler)`` in place of ``x['clip']``: the video branch from a bank of per-frame
        S-Former features (whole-video inference, predict.py); one stream"""
        audio_tok = self.audio_model(x['audio_features'])
        video_tok = self.video_model.forward_bank(*x['clip_bank'])
        if self.task == 'AU':
            return self.au_head.forward_fused(audio_tok, video_tok, pad_to=21)
        return torch.zeros(audio_tok.shape[0], 21, device=audio_tok.device, dtype=torch.float32)

    def forward(self, x):
        if 'clip_bank' in x:
            if 'clip' in x:
                raise ValueError("x holds both 'clip' and 'clip_bank': the video branch takes one of them")
            return self._forward_bank(x)
        a_in, v_in = x['audio_features'], x['clip']
        if self.concurrent_streams and a_in.is_cuda and torch.cuda.is_current_stream_capturing():
            # the two streams of the model are independent up to the fusion: while a hipGraph is being captured the aural
            # one is recorded on a side HIP stream (autograd replays each branch's backward on its forward stream), so the
            # replayed graph runs both branches concurrently: 1.06 vs 1.18 ms per step at B=64.  Eager execution is
            # host-bound at these shapes and the extra stream bookkeeping costs 7 % there, so it stays on one stream.
            cur = torch.cuda.current_stream(a_in.device)
            side = self._side_streams.get(a_in.device)
            if side is None:
                side = self._side_streams[a_in.device] = torch.cuda.Stream(a_in.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                audio_tok = self.audio_model(a_in)
            video_tok = self.video_model(v_in)
            cur.wait_stream(side)
            audio_tok.record_stream(cur)
        else:
            audio_tok = self.audio_model(a_in)
            video_tok = self.video_model(v_in)
        if self.task == 'AU':
            # fusion on the FEATURE axis (avformer.py:100) + the head's positional add in one pass; the 12 logits land in
            # a zero-padded [B, 21] row (avformer.py:101-105)
            return self.au_head.forward_fused(audio_tok, video_tok, pad_to=21)
        return torch.zeros(audio_tok.shape[0], 21, device=audio_tok.device, dtype=torch.float32)


class _LinearPadFn(torch.autograd.Function):
    """out[:, :O] = x W^T + b, out[:, O:width] = 0 - the AU logits Linear written straight into the reference's [B,21] row"""

    @staticmethod
    def forward(ctx, x, w, b, width):
        x = x.detach().float().contiguous()
        O = w.shape[0]
        ctx.small = x.shape[1] % 4 == 0 and x.shape[1] <= 4096 and w.is_contiguous()
        if ctx.small:  # one launch (a few rows x a dozen outputs: the GEMM path is a split-K launch, a fold and a zero fill)
            out = ops.linear_pad_fwd(x, w.detach(), b.detach(), width)
        else:
            out = torch.empty((x.shape[0], width), dtype=torch.float32, device=x.device)
            ops.gemm(x, w.detach(), bias=b.detach(), out=out[:, :O])  # the fp32 kernel adds a non-null bias in every epilogue
            ops.zero_cols(out, O, width)
        ctx.save_for_backward(x, w.detach())
        ctx.O = O
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        if ctx.small and dout.stride(1) == 1 and dout.dtype == torch.float32:
            dx, dw, db = ops.linear_pad_bwd(dout, x, w, *ctx.needs_input_grad[:3])
            return dx, dw, db, None
        dl = dout[:, :ctx.O]                                        # row stride `width`: read in place
        dw = ops.gemm(dl, x, trans_a=True, trans_b=False) if ctx.needs_input_grad[1] else None
        db = ops.colsum(dl) if ctx.needs_input_grad[2] else None
        dx = ops.gemm(dl, w, trans_b=False) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None


class SyntheticAVFormer(nn.Module, _TaskLossMixin):
    """BASELINE.json configs C2-C5: one Transformer(dim, depth, heads, dim_head, mlp_dim) over the fused
    [B, T_v + T_a, dim] token sequence, mean pooling, 12 AU logits in the reference's [B,21] layout."""

    def __init__(self, dim=512, depth=6, heads=8, dim_head=64, mlp_dim=1024, t_video=196, t_audio=128, task='AU',
                 compute_dtype="bf16", residual_dtype="f32", dropout=0.0, task_losses="plain"):
        super().__init__()
        self.task = task
        self.modes = ['clip', 'audio_features']
        self.t_video, self.t_audio = t_video, t_audio
        self.pos_embedding = nn.Parameter(torch.randn(1, t_video + t_audio, dim) * 0.02)
        # dropout: 0 in BASELINE's configs; the reference's real stacks train at 0.2 (heads.py:277) - bench.py --dropout times it
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, dropout, compute_dtype=compute_dtype,
                                       residual_dtype=residual_dtype)
        self.au_fc = nn.Linear(dim, 12)
        self._init_task_losses(task_losses, REFERENCE_TASK_LOSSES['avformer'])

    def forward(self, x):
        # fusion on the SEQUENCE axis + positional embedding: cat([clip, audio], 1) + pos_embedding, then the stack and
        # y.mean(dim=1).  Widths that are a multiple of 4 take the one-pass library kernels for both ends.
        if x['clip'].shape[-1] % 4 == 0:
            # (one library pass builds the sequence in the residual stream's storage type; its backward returns d clip,
            # d audio and d pos_embedding from the fp32 gradient of the sequence)
            pooled = self.transformer(x['clip'], pool='mean', fuse=(x['audio_features'], self.pos_embedding))
        else:
            tokens = torch.cat([x['clip'], x['audio_features']], dim=1)
            pooled = self.transformer(tokens + self.pos_embedding[:, :tokens.shape[1]]).mean(dim=1)
        # the reference's [B,21] layout: AU logits in slots 0..11, the rest zero
        return _LinearPadFn.apply(pooled, self.au_fc.weight, self.au_fc.bias, 21)


# name -> class, as the if/elif chain in the reference's train.py:292-315 does for --model_name
MODEL_REGISTRY = {
    'avformer': TwoStreamAuralVisualFormer,
    'avformer_synthetic': SyntheticAVFormer,
}


def _register_former_models():
    # sformer / vformer / tformer (train.py:292-303): the token sections on the HIP path around a caller's CNN backbone;
    # vggformer (train.py:296-299): the frozen VGGFace2 ResNet-50 on the HIP conv path under a trainable token section
    from . import former_models as fm
    MODEL_REGISTRY.update({'sformer': fm.SpatialFormerModel, 'vformer': fm.VisualFormerModel,
                           'tformer': fm.SpatialTemporalFormerModel, 'vggformer': fm.VGGVisualFormerModel})


def build_model(model_name: str, modality: str = 'A;V;M', task: str = 'AU', **kw) -> nn.Module:
    if 'sformer' not in MODEL_REGISTRY:
        _register_former_models()
    if model_name not in MODEL_REGISTRY:
        raise KeyError(f"model {model_name!r} is not provided by the MI355X hot-path build; available: "
                       f"{sorted(MODEL_REGISTRY)} (the reference's models that train a CNN end to end are out of scope)")
    cls = MODEL_REGISTRY[model_name]
    if cls is SyntheticAVFormer:
        return cls(task=task, **kw)
    return cls(modality=modality, task=task, **kw)
