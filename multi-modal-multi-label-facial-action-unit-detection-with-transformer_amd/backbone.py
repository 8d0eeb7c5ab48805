"""The frozen ResNet stages of the reference's S-Former (``ResFormer``, vformer.py:128-268; copied in sformer.py, tformer.py,
dual_sformer.py): ``FrozenBasicBlock`` and ``FrozenResFormer``, and the audio stream's ResNet18 (``AudioModel``, audio.py:22-39):
``FrozenAudioModel``.  Forward only, with one exception: ``FrozenResFormer(train_tokens=True)`` differentiates through the
frozen ``layer4`` and ``avgpool`` (data gradients only, csrc/conv_dgrad.hip), so that ``pos_embedding`` and
``spatial_transformer`` train on the hip backend.

"Frozen" means eval-mode here: BatchNorm2d always uses its running statistics, whatever ``train()`` says.  That is exact for
``evaluate()`` (train.py:106-169) and whole-dataset inference (test_aff2.py); the reference itself runs the BatchNorm of its
"frozen" streams in train mode while ``model.train()`` is on (avformer.py:78-85 only clears ``requires_grad``), a quirk this
package does not reproduce.

Every module takes ``backend=``: ``"torch"`` (default) is the definition - the reference's op sequence in fp32, NCHW, runs
anywhere; ``"hip"`` runs csrc/conv.hip: NHWC activations, bf16 between launches, each conv one launch with the folded BatchNorm,
the identity add and the ReLU in its epilogue.  The stage-3 map [B', 7, 7, 256] in NHWC IS the token tensor [B', 49, 256], so the
hip backend runs no map/token permute on either side of ``spatial_transformer``.  ``stem="hip"`` (with ``backend="hip"``) runs
``conv1`` / ``bn1`` / ReLU / ``maxpool`` as the one launch of csrc/stem.hip, from NCHW planes straight to the NHWC bf16 map
``layer1`` reads: no torch compute op and no layout conversion between the front end's planes and the pooled features.

``conv_dtype=`` picks the hip backend's conv arithmetic.  ``"bf16"`` (default) is the throughput form above.  ``"f32"`` is the
parity form, csrc/conv_f32.hip (the same kernel template, csrc/conv_kernel.hpp, with two-image operands): every map between
launches is fp32 and every fp32 product runs as three bf16 MFMA products (bf16x3, the arithmetic of ``compute_dtype="f32"``; ``set_f32_arithmetic`` does not reach the conv).  The stem kernel has no
parity form: in this mode the stem is the torch definition in fp32, followed by one NCHW -> NHWC fp32 conversion, and
``stem="hip"`` is refused.

By default the hip backend computes no gradients: with grad mode on and an input or parameter that requires grad, ``forward``
raises instead of silently cutting the graph.  ``FrozenResFormer(train_tokens=True)`` is the opt-in: the stem and every stage
stay frozen, and the gradient of the pooled features reaches the token section through ``FrozenBasicBlock.backward_nhwc``."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .heads import ResFormerTokens

BACKENDS = ("torch", "hip")
STEMS = ("torch", "hip")
CONV_DTYPES = ("bf16", "f32")
_CH = 32  # the conv kernel's channel granule (Cin % 32 == 0): other widths run zero-padded to it


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
    return backend


def _check_stem(stem, backend):
    if stem not in STEMS:
        raise ValueError(f"stem must be one of {STEMS}, got {stem!r}")
    if stem == "hip" and backend != "hip":
        raise ValueError(f"stem='hip' is the first launch of the hip backend: it needs backend='hip' (got backend={backend!r})")
    return stem


def _check_conv_dtype(conv_dtype, stem="torch"):
    if conv_dtype not in CONV_DTYPES:
        raise ValueError(f"conv_dtype must be one of {CONV_DTYPES}, got {conv_dtype!r}")
    if conv_dtype == "f32" and stem == "hip":
        raise ValueError("stem='hip' with conv_dtype='f32': the stem kernel (csrc/stem.hip) has no parity form - it holds its "
                         "whole bf16 weight image in registers and a second image does not fit; use stem='torch'")
    return conv_dtype


def _map_dtype(conv_dtype):
    return torch.float32 if conv_dtype == "f32" else torch.bfloat16


def _pad_to(n: int) -> int:
    return -(-n // _CH) * _CH


def _no_grad_or_raise(module: nn.Module, x: torch.Tensor, who: str):
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())):
        raise RuntimeError(f"{who}(backend='hip') is forward-only: it computes no gradients, and its input or one of its "
                           "parameters requires grad - run it under torch.no_grad() or freeze its parameters "
                           "(requires_grad_(False)); backend='torch' differentiates")


def to_nhwc(x: torch.Tensor, channels: Optional[int] = None, dtype=torch.bfloat16) -> torch.Tensor:
    """NCHW -> NHWC ``dtype`` (bf16 by default; contiguous), zero-padded to ``channels``"""
    x = x.permute(0, 2, 3, 1)
    if channels is not None and channels != x.shape[-1]:
        x = F.pad(x, (0, channels - x.shape[-1]))
    return x.to(dtype).contiguous()


class _FrozenBlock(nn.Module):
    """What the frozen residual blocks share (``FrozenBasicBlock`` here, ``vggface2.FrozenBottleneck``): eval-mode BatchNorm, the
    packed conv images of the hip backend - one (weights, scale, shift) per (conv, bn) pair of ``_pairs()``, channels
    zero-padded to 32, in the arithmetic ``conv_dtype`` names - their cache (version counters, a ``load_state_dict`` hook,
    ``refresh_weights``), ``set_conv_dtype``, the forward-only guard and the NCHW fp32 ``forward`` around ``forward_nhwc``.  A
    subclass sets ``inplanes`` / ``planes`` / ``stride`` / ``downsample`` and defines ``_pairs``, ``_forward_torch`` and
    ``_forward_convs``.  A subclass with a backward (``FrozenBasicBlock``) also defines ``_forward_convs_saving`` and
    ``backward_nhwc``; the packed data-gradient images (``_pack_dgrad``) sit in the same cache entry as the forward images."""
    expansion = 1

    def __init__(self, backend="torch", conv_dtype="bf16"):
        super().__init__()
        self.backend = _check_backend(backend)
        self.conv_dtype = _check_conv_dtype(conv_dtype)
        self._packed = None

    @staticmethod
    def _bn(x, bn):
        return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)

    def _state_key(self, device):
        ts = [t for conv, bn in self._pairs() for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        return (str(device), self.conv_dtype) + tuple((t.data_ptr(), t._version) for t in ts)

    def refresh_weights(self):
        self._packed = None

    def _load_from_state_dict(self, *args, **kwargs):
        self._packed = None
        return super()._load_from_state_dict(*args, **kwargs)

    def set_conv_dtype(self, conv_dtype):
        self.conv_dtype = _check_conv_dtype(conv_dtype)
        return self

    def _pack(self, device):
        key = self._state_key(device)
        if self._packed is None or self._packed[0] != key:
            packs, pack = [], ops.conv_pack_weight_f32 if self.conv_dtype == "f32" else ops.conv_pack_weight
            for conv, bn in self._pairs():
                w, ts = conv.weight.detach(), [t.detach() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
                if not w.is_cuda:
                    raise RuntimeError(f"{type(self).__name__}(backend='hip'): parameters must be on the MI355X (module.to('cuda')); "
                                       "there is no CPU fallback")
                co, ci = _pad_to(w.shape[0]), _pad_to(w.shape[1])
                if (co, ci) != tuple(w.shape[:2]):  # zero weights, gamma = beta = mean = 0, var = 1: the padded channels stay 0
                    w = F.pad(w, (0, 0, 0, 0, 0, ci - w.shape[1], 0, co - w.shape[0]))
                    ts = [F.pad(t, (0, co - t.numel()), value=float(i == 3)) for i, t in enumerate(ts)]
                packs.append(pack(w.float(), *[t.float() for t in ts], eps=bn.eps))
            self._packed = (key, packs, {})  # {}: the data-gradient images of this key, packed when a backward first asks
        return self._packed[1]

    def _pack_dgrad(self, device):
        """one data-gradient image (``ops.conv_pack_weight_dgrad``; the (hi, lo) pair with ``conv_dtype="f32"``) per pair of
        ``_pairs()``, channels zero-padded like the forward images and cached with them"""
        self._pack(device)
        cache = self._packed[2]
        if "dgrad" not in cache:
            images, pack = [], ops.conv_pack_weight_dgrad_f32 if self.conv_dtype == "f32" else ops.conv_pack_weight_dgrad
            for conv, bn in self._pairs():
                w, gamma, var = conv.weight.detach(), bn.weight.detach(), bn.running_var.detach()
                co, ci = _pad_to(w.shape[0]), _pad_to(w.shape[1])
                if (co, ci) != tuple(w.shape[:2]):  # zero weights and gamma = 0: the padded channels carry no gradient
                    w = F.pad(w, (0, 0, 0, 0, 0, ci - w.shape[1], 0, co - w.shape[0]))
                    gamma, var = F.pad(gamma, (0, co - gamma.numel())), F.pad(var, (0, co - var.numel()), value=1.0)
                images.append(pack(w.float(), gamma.float(), var.float(), eps=bn.eps))
            cache["dgrad"] = images
        return cache["dgrad"]

    def forward_nhwc(self, x, out_dtype=torch.bfloat16):
        """x [N, H, W, pad32(inplanes)] bf16 or fp32 -> [N, Ho, Wo, pad32(expansion * planes)] in ``out_dtype``; with
        ``conv_dtype="f32"`` x is fp32 and so is every map, the output included (``out_dtype`` does not apply)"""
        _no_grad_or_raise(self, x, type(self).__name__)
        f32 = self.conv_dtype == "f32"
        return self._forward_convs(x, self._pack(x.device), ops.conv2d_nhwc_f32 if f32 else ops.conv2d_nhwc,
                                   {} if f32 else {"out_dtype": out_dtype})

    def forward_nhwc_saving(self, x, out_dtype=torch.bfloat16):
        """``forward_nhwc`` with the same launches -> (y, saved): ``saved`` = (h, y, (H, W)), the maps the launches wrote anyway
        (h: the block's inner ReLU output) and the input map's extent, what ``backward_nhwc`` takes"""
        _no_grad_or_raise(self, x, type(self).__name__)
        f32 = self.conv_dtype == "f32"
        return self._forward_convs_saving(x, self._pack(x.device), ops.conv2d_nhwc_f32 if f32 else ops.conv2d_nhwc,
                                          {} if f32 else {"out_dtype": out_dtype})

    def _forward_convs_saving(self, x, p, conv, last):
        raise NotImplementedError(f"{type(self).__name__} has no backward on the hip backend")

    def backward_nhwc(self, gs, saved, x_gate=None, out_dtype=None):
        raise NotImplementedError(f"{type(self).__name__} has no backward on the hip backend")

    def forward(self, x):
        if self.backend == "torch":
            return self._forward_torch(x)
        ops._need_cuda(x)
        y = self.forward_nhwc(to_nhwc(x, _pad_to(self.inplanes), _map_dtype(self.conv_dtype)), out_dtype=torch.float32)
        return y[..., :self.expansion * self.planes].permute(0, 3, 1, 2).contiguous()


class FrozenBasicBlock(_FrozenBlock):
    """``BasicBlock`` (vformer.py:128-166) in eval mode: ``conv1``, ``bn1``, ``conv2``, ``bn2``, ``downsample.0``, ``downsample.1``
    are ordinary ``nn.Conv2d`` / ``nn.BatchNorm2d`` children with the reference's state_dict keys and shapes.
    ``forward`` takes and returns NCHW fp32 with either backend; ``forward_nhwc`` is the hip backend's native form (two launches, or
    three with a downsample).  The packed bf16 weights and folded BatchNorm are rebuilt whenever a parameter or buffer changes
    (version counters, and a ``load_state_dict`` hook); writes through ``.data`` bypass the counters: call ``refresh_weights()``.

    ``conv_dtype="f32"`` (hip backend) is the parity form (csrc/conv_f32.hip): every map stays fp32 and every fp32 product runs
    as three bf16 MFMA products (bf16x3), weights packed as a hi and a lo bf16 image.  ``"bf16"`` (default) launches what it
    always launched."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, backend="torch", conv_dtype="bf16"):
        super().__init__(backend, conv_dtype)
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride, self.inplanes, self.planes = stride, inplanes, planes

    def _forward_torch(self, x):
        out = F.relu(self._bn(self.conv1(x), self.bn1))
        out = self._bn(self.conv2(out), self.bn2)
        identity = x if self.downsample is None else self._bn(self.downsample[0](x), self.downsample[1])
        return F.relu(out + identity)

    # ---- hip ------------------------------------------------------------------------------------
    def _pairs(self):
        pairs = [(self.conv1, self.bn1), (self.conv2, self.bn2)]
        if self.downsample is not None:
            pairs.append((self.downsample[0], self.downsample[1]))
        return pairs

    def _forward_convs(self, x, p, conv, last):
        return self._forward_convs_saving(x, p, conv, last)[0]

    def _forward_convs_saving(self, x, p, conv, last):
        h = conv(x, *p[0], k=3, stride=self.stride, relu=True)
        identity = x if self.downsample is None else conv(x, *p[2], k=1, stride=self.stride)
        y = conv(h, *p[1], k=3, stride=1, residual=identity, relu=True, **last)
        return y, (h, y, tuple(x.shape[1:3]))

    def backward_nhwc(self, gs, saved, x_gate=None, out_dtype=None):
        """The gradient for the block's input, [N, H, W, pad32(inplanes)], from ``gs`` [N, Ho, Wo, pad32(planes)]: the gradient
        with respect to the block's pre-ReLU sum, i.e. the caller's dy already gated by y > 0.  ``saved`` comes from
        ``forward_nhwc_saving``.  ``x_gate``: the block's input map when that map is itself a ReLU output (between blocks) - the
        result is then gated by x_gate > 0 and is the ``gs`` of the block before; ``None`` leaves it ungated.  Three launches,
        or two without a downsample (csrc/conv_dgrad.hip):
            dh  = dgrad(conv2; gy = gs, gate = h)
            add = dgrad(downsample; gy = gs) if the block has one, else gs
            dx  = dgrad(conv1; gy = dh, addend = add, gate = x_gate)
        ``out_dtype``: dx's type (default: x_gate's, else the map type of ``conv_dtype``); add and x_gate have it too, dh has
        h's.  With ``conv_dtype="f32"`` every map is fp32.  The weights are frozen: nothing else has a gradient."""
        h, _, in_hw = saved
        f32 = self.conv_dtype == "f32"
        dgrad, w = (ops.conv2d_nhwc_dgrad_f32 if f32 else ops.conv2d_nhwc_dgrad), self._pack_dgrad(gs.device)
        if out_dtype is None:
            out_dtype = x_gate.dtype if x_gate is not None else _map_dtype(self.conv_dtype)
        mid, last = ({}, {}) if f32 else ({"out_dtype": h.dtype}, {"out_dtype": out_dtype})
        dh = dgrad(gs, w[1], tuple(h.shape[1:3]), k=3, stride=1, gate=h, **mid)
        add = gs if self.downsample is None else dgrad(gs, w[2], in_hw, k=1, stride=self.stride, **last)
        return dgrad(dh, w[0], in_hw, k=3, stride=self.stride, addend=add, gate=x_gate, **last)


class _Stage(nn.Sequential):
    """one ``layerN``: its blocks in a row; NHWC in, NHWC out, the last block writing ``out_dtype``"""

    def forward_nhwc(self, x, out_dtype=torch.bfloat16):
        for i, blk in enumerate(self):
            x = blk.forward_nhwc(x, out_dtype) if i == len(self) - 1 else blk.forward_nhwc(x)
        return x


class _HipStem:
    """``conv1`` - ``bn1`` - relu - ``maxpool`` of a ResNet (children ``conv1`` 7x7 / 2 / pad 3 with 1, 3 or 4 input channels,
    ``bn1``, ``maxpool`` 3x3 / 2 / pad 1) in both forms: ``stem`` is the definition in torch ops, ``stem_nhwc`` the one launch of
    csrc/stem.hip.  The packed stem image follows ``conv1`` / ``bn1`` as ``FrozenBasicBlock._pack`` follows its pairs: version
    counters, and a ``load_state_dict`` hook; writes through ``.data`` bypass the counters: call ``refresh_weights()``.
    ``_stem_pool`` names the geometry of ``maxpool`` for the kernel (``ops.stem_nchw``'s ``pool``): ``"pad1"`` here, ``"ceil"``
    for the pad 0 / ceil_mode pool of ``vggface2.FrozenVGGFace2``."""
    _stem_packed = None
    _stem_pool = "pad1"

    def stem(self, x):
        """conv1 - bn1 - relu - maxpool (vformer.py:238-241), eval-mode BatchNorm, torch ops: NCHW fp32 in and out"""
        return self.maxpool(F.relu(FrozenBasicBlock._bn(self.conv1(x), self.bn1)))

    def refresh_weights(self):
        self._stem_packed = None
        for m in self.modules():
            if isinstance(m, _FrozenBlock):
                m.refresh_weights()

    def _load_from_state_dict(self, *args, **kwargs):
        self._stem_packed = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _stem_pack(self, device):
        ts = (self.conv1.weight, self.bn1.weight, self.bn1.bias, self.bn1.running_mean, self.bn1.running_var)
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._stem_packed is None or self._stem_packed[0] != key:
            if not ts[0].is_cuda:
                raise RuntimeError(f"{type(self).__name__}(stem='hip'): parameters must be on the MI355X (module.to('cuda')); "
                                   "there is no CPU fallback")
            self._stem_packed = (key, ops.stem_pack_weight(*[t.detach().float() for t in ts], eps=self.bn1.eps))
        return self._stem_packed[1]

    def stem_nhwc(self, x):
        """x [N, Cin, H, W] fp32 or bf16 planes -> [N, Hp, Wp, 64] NHWC bf16, what ``layer1.forward_nhwc`` reads (ops.stem_nchw)"""
        ops._need_cuda(x)
        return ops.stem_nchw(x.contiguous(), *self._stem_pack(x.device), pool=self._stem_pool)


class _Layer4Pool(torch.autograd.Function):
    """``FrozenResFormer.tokens_to_features`` with a backward: ``layer4`` with its ReLU maps kept, then the NHWC pool; backward
    = the pool's backward gated by the last ReLU map, then the blocks in reverse, the last launch writing the fp32 gradient of
    the transformer's output.  No host synchronisation; every buffer comes from torch's allocator."""

    @staticmethod
    def forward(ctx, t, stage, hw):
        x = t.detach().contiguous().view(t.shape[0], hw[0], hw[1], t.shape[2])
        saved = []
        for blk in stage:
            x, s = blk.forward_nhwc_saving(x)
            saved.append(s)
        ctx.stage, ctx.maps, ctx.t_shape = stage, saved, t.shape
        return ops.avgpool_nhwc(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        blocks, saved = list(ctx.stage), ctx.maps
        y = saved[-1][1]
        g = ops.avgpool_nhwc_bwd(dout.float().contiguous(), y.shape[1] * y.shape[2], gate=y).view(y.shape)
        for i in range(len(blocks) - 1, -1, -1):
            g = blocks[i].backward_nhwc(g, saved[i], x_gate=saved[i - 1][1] if i else None, out_dtype=None if i else torch.float32)
        return g.view(ctx.t_shape), None, None


class FrozenResFormer(_HipStem, ResFormerTokens):
    """The whole S-Former, ``ResFormer(BasicBlock, layers)`` (vformer.py:168-268), with the reference's names - ``conv1``, ``bn1``,
    ``maxpool``, ``layer1`` .. ``layer4``, ``avgpool``, ``pos_embedding``, ``spatial_transformer.*`` - so that a reference checkpoint
    loads with every key matched.  x [B, T, C, H, W] or [B', C, H, W] -> [B', 512] fp32.

    ``backend="hip"``: with ``stem="torch"`` (default) the 7x7 ``conv1`` / ``bn1`` / ReLU / ``maxpool`` are torch ops and one NCHW
    -> NHWC bf16 conversion follows; with ``stem="hip"`` they are the one launch of csrc/stem.hip, which reads x as it is and
    writes that NHWC bf16 map (``in_channels`` 1, 3 or 4).  Then ``layer1`` .. ``layer3`` on the conv kernel; the last launch of ``layer3`` writes
    the fp32 tokens, ``pos_embedding`` is added, ``spatial_transformer`` runs, and its output goes straight into ``layer4``;
    ``avgpool`` is the NHWC pool kernel.  The token section is this package's ``Transformer`` with either backend, so the
    module needs the GPU either way.

    ``conv_dtype="f32"`` (hip backend): the parity form of the conv stages (csrc/conv_f32.hip, bf16x3 products, fp32 maps
    throughout); the stem is the torch definition in fp32, followed by one NCHW -> NHWC fp32 conversion (``stem="hip"`` has no
    parity form and is refused).  With ``compute_dtype="f32"`` the whole module then runs in parity arithmetic.

    ``train_tokens=True`` trains ``pos_embedding`` and ``spatial_transformer`` on the hip backend.  The constructor freezes the
    stem and the stages (``conv1``, ``bn1``, ``layer1`` .. ``layer4``: ``requires_grad_(False)``); ``forward`` then runs the stem
    and ``layer1`` .. ``layer3`` under ``no_grad``, adds ``pos_embedding`` and runs ``spatial_transformer`` under autograd, and
    differentiates ``layer4`` + ``avgpool`` with the data-gradient kernels (csrc/conv_dgrad.hip): gradient maps in bf16 with
    ``conv_dtype="bf16"``, fp32 with ``"f32"``, the last launch writing the fp32 gradient the transformer's backward takes.
    A stage parameter that requires grad again is refused by name, and so is an input that requires grad (the stem and
    ``layer1`` .. ``layer3`` have no backward).  Under ``torch.no_grad()``, and with the default ``train_tokens=False``, every
    path is the forward-only one."""
    _STAGES = ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4")

    def __init__(self, layers=(2, 2, 2, 2), backend="torch", in_channels=3, dropout=0.0, compute_dtype="bf16", stem="torch",
                 conv_dtype="bf16", train_tokens=False):
        super().__init__(dropout=dropout, compute_dtype=compute_dtype)
        self.backend = _check_backend(backend)
        self.stem_backend = _check_stem(stem, backend)
        self.conv_dtype = _check_conv_dtype(conv_dtype, stem)
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self._modules["spatial_transformer"] = self._modules.pop("spatial_transformer")  # the reference's state_dict order
        for m in self.modules():                                                        # vformer.py:200-205
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        self.train_tokens = False
        self.set_train_tokens(train_tokens)

    def set_train_tokens(self, flag):
        """``True``: freeze the stem and the stages and let ``forward`` differentiate ``layer4`` + ``avgpool`` for the token
        section (hip backend); ``False``: the forward-only module (parameters frozen earlier stay frozen)"""
        self.train_tokens = bool(flag)
        if self.train_tokens:
            for name in self._STAGES:
                getattr(self, name).requires_grad_(False)
        return self

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(planes))
        stage = [FrozenBasicBlock(self.inplanes, planes, stride, downsample, backend=self.backend, conv_dtype=self.conv_dtype)]
        self.inplanes = planes
        stage += [FrozenBasicBlock(planes, planes, backend=self.backend, conv_dtype=self.conv_dtype) for _ in range(1, blocks)]
        return _Stage(*stage)

    def set_backend(self, backend, stem=None):
        """``stem=None`` keeps the stem where it is"""
        stem = _check_stem(self.stem_backend if stem is None else stem, _check_backend(backend))
        _check_conv_dtype(self.conv_dtype, stem)
        self.backend, self.stem_backend = backend, stem
        for m in self.modules():
            if isinstance(m, _FrozenBlock):
                m.backend = backend
        return self

    def set_conv_dtype(self, conv_dtype):
        """``"bf16"`` / ``"f32"``: the arithmetic of the hip backend's conv stages; the packed images are rebuilt on the next call"""
        self.conv_dtype = _check_conv_dtype(conv_dtype, self.stem_backend)
        for m in self.modules():
            if isinstance(m, _FrozenBlock):
                m.set_conv_dtype(conv_dtype)
        return self

    def stages_to_tokens(self, x):
        """hip: the stem's NCHW output -> layer1 .. layer3 -> ([B', h*w, 256] fp32 tokens + pos_embedding, (h, w))"""
        return self.nhwc_to_tokens(to_nhwc(x, dtype=_map_dtype(self.conv_dtype)))

    def nhwc_to_tokens(self, x):
        """hip: the stem's NHWC map (bf16; fp32 with ``conv_dtype="f32"``) -> layer1 .. layer3 -> ([B', h*w, 256] fp32 tokens +
        pos_embedding, (h, w))"""
        t, hw = self._nhwc_to_raw_tokens(x)
        return t + self.pos_embedding[:, :t.shape[1]], hw                         # vformer.py:253

    def _nhwc_to_raw_tokens(self, x):
        x = self.layer3.forward_nhwc(self.layer2.forward_nhwc(self.layer1.forward_nhwc(x)), out_dtype=torch.float32)
        return x.view(x.shape[0], x.shape[1] * x.shape[2], x.shape[3]), (x.shape[1], x.shape[2])  # NHWC IS [B', tokens, C]: no permute

    def tokens_to_features(self, t, hw):
        """hip: the transformer's [B', h*w, 256] fp32 output -> layer4 -> avgpool -> [B', 512] fp32"""
        x = self.layer4.forward_nhwc(t.view(t.shape[0], hw[0], hw[1], t.shape[2]))
        return ops.avgpool_nhwc(x)

    def forward(self, x):
        if x.dim() == 5:
            x = x.contiguous().view(-1, *x.shape[2:])                             # vformer.py:234-235
        if self.backend == "torch":
            x = self.layer3(self.layer2(self.layer1(self.stem(x))))
            x = self.layer4(ResFormerTokens.forward(self, x))                     # vformer.py:245-261
            return torch.flatten(self.avgpool(x), 1)
        ops._need_cuda(x)
        if self.train_tokens and torch.is_grad_enabled():
            return self._forward_train_tokens(x)
        _no_grad_or_raise(self, x, "FrozenResFormer")
        t, hw = self.nhwc_to_tokens(self.stem_nhwc(x)) if self.stem_backend == "hip" else self.stages_to_tokens(self.stem(x))
        return self.tokens_to_features(self.spatial_transformer(t), hw)


    def _forward_train_tokens(self, x):
        """hip, ``train_tokens=True``, grad mode on: the frozen front under ``no_grad``, the token section under autograd,
        ``layer4`` + ``avgpool`` through ``_Layer4Pool``"""
        if x.requires_grad:
            raise RuntimeError("FrozenResFormer(backend='hip') is forward-only: it computes no gradients for its input, which "
                               "requires grad (train_tokens=True differentiates layer4 and avgpool for the token section only); "
                               "backend='torch' differentiates")
        for stage in self._STAGES:
            for name, p in getattr(self, stage).named_parameters():
                if p.requires_grad:
                    raise RuntimeError(f"FrozenResFormer(train_tokens=True): parameter {stage}.{name} requires grad, but the stem and "
                                       "the stages are frozen on the hip backend (data gradients only, no weight or BatchNorm "
                                       "gradient) - requires_grad_(False) it, or use backend='torch'")
        with torch.no_grad():
            x = self.stem_nhwc(x) if self.stem_backend == "hip" else to_nhwc(self.stem(x), dtype=_map_dtype(self.conv_dtype))
            t, hw = self._nhwc_to_raw_tokens(x)
        t = t + self.pos_embedding[:, :t.shape[1]]                                # vformer.py:253, under autograd
        return _Layer4Pool.apply(self.spatial_transformer(t), self.layer4, hw)


class _FrozenResNet18(_HipStem, nn.Module):
    """torchvision's ``resnet18`` as audio.py:25-31 rebuilds it - ``conv1`` with ``in_channels`` inputs, ``bn1``, ``relu``,
    ``maxpool``, ``layer1`` .. ``layer4``, ``avgpool``, ``fc`` - with torchvision's state_dict keys, written out here because
    torchvision is not a dependency.  ``fc`` is the identity, as avformer.py:50 leaves it."""

    def __init__(self, layers=(2, 2, 2, 2), in_channels=1, backend="torch", conv_dtype="bf16"):
        super().__init__()
        self.backend = backend
        self.conv_dtype = _check_conv_dtype(conv_dtype)
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Identity()
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    _make_layer = FrozenResFormer._make_layer

    def forward(self, x):
        if self.backend == "torch":
            x = self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
            return self.fc(torch.flatten(self.avgpool(x), 1))
        # parity form: the stem as the torch definition in fp32 (the stem kernel has no parity form), fp32 maps from there on
        x = to_nhwc(self.stem(x.float()), dtype=torch.float32) if self.conv_dtype == "f32" else self.stem_nhwc(x)
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = stage.forward_nhwc(x)
        return self.fc(ops.avgpool_nhwc(x))


class FrozenAudioModel(nn.Module):
    """``AudioModel`` (audio.py:22-39) with its fc replaced by the identity, as avformer.py:40-50 uses it: the mel map
    [B, 1, 64, 1001] -> ``resnet`` (ResNet18 with a one-channel ``conv1``) -> [B, 512] fp32.  The state_dict keys are torchvision's
    ResNet18 keys under ``resnet.``; a checkpoint's ``resnet.fc.*`` keys have no counterpart and are skipped by a
    ``strict=False`` load.

    ``backend="torch"`` (default) is the definition; ``backend="hip"`` is the stem kernel (csrc/stem.hip), the four stages on
    the conv kernel and ``ops.avgpool_nhwc``: NCHW planes in, no torch compute op, forward only (``_no_grad_or_raise``).
    ``conv_dtype="f32"`` (hip backend): the stages in the parity form (csrc/conv_f32.hip, fp32 maps, bf16x3 products) behind
    the stem as the torch definition in fp32 - the stem kernel has no parity form."""

    def __init__(self, backend="torch", layers=(2, 2, 2, 2), conv_dtype="bf16"):
        super().__init__()
        self.backend = _check_backend(backend)
        self.conv_dtype = _check_conv_dtype(conv_dtype)
        self.resnet = _FrozenResNet18(layers, in_channels=1, backend=backend, conv_dtype=conv_dtype)
        self.modes = ["audio_features"]

    def set_conv_dtype(self, conv_dtype):
        self.conv_dtype = self.resnet.conv_dtype = _check_conv_dtype(conv_dtype)
        for m in self.modules():
            if isinstance(m, _FrozenBlock):
                m.set_conv_dtype(conv_dtype)
        return self

    def set_backend(self, backend):
        self.backend = self.resnet.backend = _check_backend(backend)
        for m in self.modules():
            if isinstance(m, _FrozenBlock):
                m.backend = backend
        return self

    def forward(self, x):
        if self.backend == "hip":
            ops._need_cuda(x)
            _no_grad_or_raise(self, x, "FrozenAudioModel")
        return self.resnet(x)


class FrozenVideoModel(nn.Module):
    """``VideoModel`` (vformer.py:295-311) with its fc replaced by the identity, as avformer.py:61-66 uses it: clip [B, C, T, H, W]
    -> the last ``num_channels`` channels -> ``s_former`` -> ``t_former`` -> [B, 512]"""

    def __init__(self, backend="torch", compute_dtype="bf16", stem="torch", conv_dtype="bf16", train_tokens=False):
        super().__init__()
        from .heads import TFormer
        self.s_former = FrozenResFormer(backend=backend, compute_dtype=compute_dtype, stem=stem, conv_dtype=conv_dtype,
                                        train_tokens=train_tokens)
        self.t_former = TFormer(compute_dtype=compute_dtype)
        self.num_channels = 3

    def set_conv_dtype(self, conv_dtype):
        self.s_former.set_conv_dtype(conv_dtype)
        return self

    def forward(self, x):
        x = x[:, -self.num_channels:].permute(0, 2, 1, 3, 4)
        return self.t_former(self.s_former(x))

    # ---- whole-video inference: the S-Former once per frame, the clips from its features (frames.FeatureBank) -------------------
    @torch.no_grad()
    def frame_features(self, frame_bank, front_end, chunk: int = 256):
        """``frames.FrameBank`` -> ``frames.FeatureBank``: every frame of the bank once through ``front_end`` (no mirror) and
        ``s_former``, ``chunk`` frames at a time as one-frame clips [n, 1, C, H, W], into ``features`` fp32 [F, 512].  ``s_former``
        is frozen and applied per frame (vformer.py:232-268), so these are the rows ``forward`` computes for every clip a frame
        sits in.  ``black`` is ``s_former`` of one all-zero uint8 frame through the same ``front_end``: black is a byte value and
        is normalised like any other.  ``video_db_nr`` and ``present`` are carried over; a frame with ``present == 0`` may hold
        anything, the rule never reads its row.  ``front_end``: a ``ClipFrontEnd(layout="tchw", channels=num_channels)``."""
        from .clip import ClipFrontEnd
        from .frames import FeatureBank, FrameBank
        if not isinstance(frame_bank, FrameBank):
            raise ValueError(f"frame_bank must be a FrameBank, got {type(frame_bank).__name__}")
        if not isinstance(front_end, ClipFrontEnd):
            raise ValueError(f"front_end must be a ClipFrontEnd, got {type(front_end).__name__}")
        if front_end.layout != "tchw":
            raise ValueError(f"front_end must write layout='tchw' ([n, 1, C, H, W], what s_former views as frames), got {front_end.layout!r}")
        if front_end.channels != self.num_channels:
            raise ValueError(f"front_end keeps {front_end.channels} channels, the model takes the last {self.num_channels}")
        if frame_bank.frame_shape[-1] != front_end.in_channels:
            raise ValueError(f"the bank has {frame_bank.frame_shape[-1]} channels, front_end's mean / std have {front_end.in_channels}")
        if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f"chunk must be an integer of at least 1, got {chunk!r}")
        frames, F = frame_bank.frames, len(frame_bank)
        black = self.s_former(front_end(torch.zeros((1, 1) + frame_bank.frame_shape, dtype=torch.uint8, device=frames.device)))
        features = torch.empty((F, black.shape[1]), dtype=torch.float32, device=frames.device)
        for i in range(0, F, chunk):
            features[i:i + chunk] = self.s_former(front_end(frames[i:i + chunk].unsqueeze(1)))
        return FeatureBank(features, black[0].float().contiguous(), frame_bank.video_db_nr, frame_bank.present)

    def forward_bank(self, feature_bank, index, assembler):
        """``forward`` on the clips of ``index`` int64 [B], from the features of their frames: the tokens
        ``cat(cls_token, rows) + pos_embedding`` straight from the bank (``frames.FeatureClipAssembler``), then ``t_former``'s
        stack -> [B, 512]"""
        from .frames import FeatureBank, FeatureClipAssembler
        if not isinstance(feature_bank, FeatureBank):
            raise ValueError(f"feature_bank must be a FeatureBank, got {type(feature_bank).__name__}")
        if not isinstance(assembler, FeatureClipAssembler):
            raise ValueError(f"assembler must be a FeatureClipAssembler, got {type(assembler).__name__}")
        t = self.t_former
        if assembler.clip_len != t.num_patches:
            raise ValueError(f"the assembler builds clips of {assembler.clip_len} frames, t_former takes {t.num_patches}")
        if feature_bank.dim != t.dim:
            raise ValueError(f"the bank's features are {feature_bank.dim} wide, t_former takes {t.dim}")
        if not feature_bank.features.is_cuda:
            raise RuntimeError("FrozenVideoModel.forward_bank needs its bank on the MI355X; there is no CPU fallback")
        return t.forward_tokens(assembler.tokens(feature_bank, index, t.cls_token, t.pos_embedding))
