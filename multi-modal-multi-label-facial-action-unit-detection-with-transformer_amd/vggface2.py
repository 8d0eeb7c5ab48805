"""The S-Former of the reference's ``vggformer`` model (models/vggformer.py): ``FrozenBottleneck`` (vggformer.py:25-60),
``FrozenVGGFace2`` (``VGGFace2_extractor``, vggformer.py:62-115: the VGGFace2 ResNet-50) and ``VGGFormer`` (vggformer.py:250-296).

The whole CNN of this model is frozen (vggformer.py:255-256) and everything trainable sits behind its last convolution: the
1x1 ``conv`` 2048 -> 512, ``pos_embedding`` and ``spatial_transformer``.  No data gradient has to pass through a convolution, so
unlike ``backbone.FrozenResFormer`` the module TRAINS on the hip backend: the extractor runs forward-only on the NHWC conv
kernels (csrc/conv.hip / csrc/conv_f32.hip; a Bottleneck needs only their 1x1 and 3x3 at stride 1 or 2), and the rows of its
NHWC map are the tokens' inputs.

"Frozen" means eval-mode here, as everywhere in ``backbone``: BatchNorm2d always uses its running statistics, whatever
``train()`` says.  The reference leaves the frozen extractor's BatchNorm in train mode while ``model.train()`` is on
(vggformer.py:255-256 only clears ``requires_grad``); this package does not reproduce that.

Unpinned: the full extractor is 103 MB of weights and has no reference fixture; tests hold a three-Bottleneck chain and the stem
to the reference (tests/golden/g22_*) and the full modules to their own ``backend="torch"``."""
from __future__ import annotations

import math
import pickle

import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .backbone import (_FrozenBlock, _HipStem, _Stage, _check_backend, _check_conv_dtype, _check_stem, _map_dtype, _no_grad_or_raise,
                       to_nhwc)
from .heads import _AssembleFn
from .transformer import Transformer


class FrozenBottleneck(_FrozenBlock):
    """``Bottleneck`` (vggformer.py:25-60) in eval mode: ``conv1`` 1x1 with the stride (caffe style), ``conv2`` 3x3, ``conv3`` 1x1 to
    ``4 * planes``, ``bn1`` .. ``bn3``, ``downsample.0`` / ``.1``: ordinary ``nn.Conv2d`` / ``nn.BatchNorm2d`` children with the
    reference's state_dict keys and shapes.  ``forward`` takes and returns NCHW fp32 with either backend; ``forward_nhwc`` is the
    hip backend's native form: three launches, or four with a downsample, the last one carrying the identity add and the ReLU.
    Packing, the weight cache, ``refresh_weights``, ``set_conv_dtype`` and the forward-only guard are ``backbone._FrozenBlock``'s,
    shared with ``FrozenBasicBlock``."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, backend="torch", conv_dtype="bf16"):
        super().__init__(backend, conv_dtype)
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride, self.inplanes, self.planes = stride, inplanes, planes

    def _forward_torch(self, x):
        out = F.relu(self._bn(self.conv1(x), self.bn1))
        out = F.relu(self._bn(self.conv2(out), self.bn2))
        out = self._bn(self.conv3(out), self.bn3)
        residual = x if self.downsample is None else self._bn(self.downsample[0](x), self.downsample[1])
        return F.relu(out + residual)

    def _pairs(self):
        pairs = [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]
        if self.downsample is not None:
            pairs.append((self.downsample[0], self.downsample[1]))
        return pairs

    def _forward_convs(self, x, p, conv, last):
        h = conv(x, *p[0], k=1, stride=self.stride, relu=True)
        h = conv(h, *p[1], k=3, stride=1, relu=True)
        residual = x if self.downsample is None else conv(x, *p[3], k=1, stride=self.stride)
        return conv(h, *p[2], k=1, stride=1, residual=residual, relu=True, **last)


class FrozenVGGFace2(_HipStem, nn.Module):
    """``VGGFace2_extractor`` (vggformer.py:62-115) with the reference's names - ``conv1``, ``bn1``, ``relu``, ``maxpool`` (3x3 / 2 /
    pad 0, ceil_mode), ``layer1`` .. ``layer4`` of ``FrozenBottleneck`` - and its initialisation (vggformer.py:79-85), so that the
    VGGFace2 ``resnet50_ft`` weights load with every key but ``fc.*`` matched.  x [B', C, H, W] -> [B', 2048, h, w] NCHW fp32 with
    either backend; ``forward_nhwc`` -> the NHWC map [B', h, w, 2048] of the hip backend, no permute.

    BatchNorm2d uses its running statistics whatever ``.training`` says, like every ``Frozen*`` module of this package (the
    reference leaves the frozen extractor's BatchNorm in train mode under ``model.train()``).

    ``backend="hip"``: ``stem="torch"`` runs ``conv1`` / ``bn1`` / ReLU / ``maxpool`` as torch ops and one NCHW -> NHWC conversion;
    ``stem="hip"`` runs them as the one launch of csrc/stem.hip in its ceil-mode pool geometry (``in_channels`` 1, 3 or 4).  Then
    16 Bottlenecks on the conv kernel: 52 launches.  ``conv_dtype="f32"`` is the parity form of the stages (fp32 maps, bf16x3
    products) behind the torch stem in fp32; ``stem="hip"`` has no parity form and is refused.  Forward only."""
    _stem_pool = "ceil"

    def __init__(self, layers=(3, 4, 6, 3), in_channels=3, backend="torch", stem="torch", conv_dtype="bf16"):
        super().__init__()
        self.backend = _check_backend(backend)
        self.stem_backend = _check_stem(stem, backend)
        self.conv_dtype = _check_conv_dtype(conv_dtype, stem)
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=0, ceil_mode=True)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.out_channels = 512 * FrozenBottleneck.expansion
        for m in self.modules():                                                        # vggformer.py:79-85
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_layer(self, planes, blocks, stride=1):
        downsample, e = None, FrozenBottleneck.expansion
        if stride != 1 or self.inplanes != planes * e:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * e, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * e))
        stage = [FrozenBottleneck(self.inplanes, planes, stride, downsample, backend=self.backend, conv_dtype=self.conv_dtype)]
        self.inplanes = planes * e
        stage += [FrozenBottleneck(self.inplanes, planes, backend=self.backend, conv_dtype=self.conv_dtype) for _ in range(1, blocks)]
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
        self.conv_dtype = _check_conv_dtype(conv_dtype, self.stem_backend)
        for m in self.modules():
            if isinstance(m, _FrozenBlock):
                m.set_conv_dtype(conv_dtype)
        return self

    def forward_nhwc(self, x, out_dtype=torch.bfloat16):
        """hip: x [B', C, H, W] planes -> [B', h, w, 2048] NHWC in ``out_dtype`` (fp32 with ``conv_dtype="f32"``, whatever
        ``out_dtype`` says)"""
        ops._need_cuda(x)
        _no_grad_or_raise(self, x, "FrozenVGGFace2")
        if self.stem_backend == "hip":
            h = self.stem_nhwc(x)
        else:  # (the parity form: the stem as the torch definition in fp32 - the stem kernel has no parity form)
            h = to_nhwc(self.stem(x.float()), dtype=_map_dtype(self.conv_dtype))
        h = self.layer3.forward_nhwc(self.layer2.forward_nhwc(self.layer1.forward_nhwc(h)))
        return self.layer4.forward_nhwc(h, out_dtype)

    def forward(self, x):
        if self.backend == "torch":
            return self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
        return self.forward_nhwc(x, out_dtype=torch.float32).permute(0, 3, 1, 2).contiguous()


class _Conv1x1Fn(torch.autograd.Function):
    """tokens' inputs = rows W^T: the trainable 1x1 ``conv`` 2048 -> dim of ``VGGFormer`` (vggformer.py:257, 274) on the rows
    [B' h w, 2048] of the frozen extractor's NHWC map, on the library's GEMMs: forward NT, weight gradient TN, no gradient for the
    map (nothing behind it trains).  Operands are bf16 under ``conv_dtype="bf16"`` (the map already is; the weight and the
    incoming gradient are cast) and fp32 under ``"f32"`` (the parity GEMM); the output and the weight gradient are fp32."""

    @staticmethod
    def forward(ctx, rows, weight, bf16):
        w = weight.detach().reshape(weight.shape[0], -1)
        if bf16:
            rows = rows if rows.dtype == torch.bfloat16 else ops.cast_bf16(rows)
            w = ops.cast_bf16(w)
        else:
            rows, w = rows.float(), w.float()
        ctx.save_for_backward(rows)
        ctx.bf16, ctx.wshape = bf16, weight.shape
        return ops.gemm(rows, w, out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, dout):
        (rows,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None
        dout = dout.contiguous()
        if ctx.bf16:
            dout = ops.cast_bf16(dout.float())
        dw = ops.gemm(dout, rows, trans_a=True, trans_b=False, out_dtype=torch.float32)
        return None, dw.view(ctx.wshape), None


class VGGFormer(nn.Module):
    """``VGGFormer`` (vggformer.py:250-296): the frozen VGGFace2 ResNet-50, a trainable 1x1 ``conv`` 2048 -> ``dim``, the learned
    positional embedding, ``spatial_transformer`` = ``Transformer(dim, depth, heads, dim_head, mlp_dim)`` and the mean over the
    tokens.  state_dict names and order are the reference's: ``pos_embedding``, ``VGG_model.*``, ``conv.weight``,
    ``spatial_transformer.*``; ``VGG_model``'s parameters have ``requires_grad=False``.  x [B, T, C, H, W] or [B', C, H, W] ->
    [B', dim] fp32.

    ``backend="hip"``: the extractor on the HIP conv path (``FrozenVGGFace2``; ``stem="hip"``: its stem too), producing the NHWC
    map [B', h, w, 2048] whose rows ARE the tokens' inputs: ``tokens = rows @ conv.weight^T + pos_embedding[:, :h*w]`` on the
    library's GEMM, then ``spatial_transformer(tokens, pool='mean')``, which stands for the reference's permute / reshape /
    avgpool.  The module is trainable on this path: ``conv``, ``pos_embedding`` and the transformer get their gradients; the
    forward-only guard of the conv path applies to the input x only (x may not require grad).  ``backend="torch"`` is the
    definition: the reference's op sequence in torch ops on the same parameters (the token section is this package's
    ``Transformer`` with either backend, so the module needs the GPU either way).

    ``conv_dtype="f32"`` runs the extractor and the 1x1 ``conv`` in the parity arithmetic; with ``compute_dtype="f32"`` the whole
    module then does.  BatchNorm2d of the extractor is eval-mode whatever ``.training`` says (see ``FrozenVGGFace2``)."""

    def __init__(self, num_patches=7 * 7, dim=512, depth=1, heads=8, mlp_dim=512, dim_head=32, dropout=0.0, backend="torch",
                 stem="torch", conv_dtype="bf16", compute_dtype="bf16", in_channels=3):
        super().__init__()
        self.backend = _check_backend(backend)
        self.stem_backend = _check_stem(stem, backend)
        self.conv_dtype = _check_conv_dtype(conv_dtype, stem)
        self.num_patches, self.dim = num_patches, dim
        self.VGG_model = FrozenVGGFace2(in_channels=in_channels, backend=backend, stem=stem, conv_dtype=conv_dtype)
        for param in self.VGG_model.parameters():                                      # vggformer.py:255-256
            param.requires_grad = False
        self.conv = nn.Conv2d(self.VGG_model.out_channels, dim, kernel_size=1, stride=1, bias=False)
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches, dim))
        self.spatial_transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, dropout, compute_dtype=compute_dtype)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))

    def load_pretrain_vgg(self, path):
        """vggformer.py:262-266: a latin1 pickle of name -> numpy array (the VGGFace2 ``resnet50_ft`` weights), loaded
        ``strict=False`` into ``VGG_model``; -> what ``load_state_dict`` returns (its ``fc.*`` keys are the unexpected ones)"""
        with open(path, 'rb') as f:
            obj = f.read()
        weights = {key: torch.from_numpy(arr) for key, arr in pickle.loads(obj, encoding='latin1').items()}
        return self.VGG_model.load_state_dict(weights, strict=False)

    def set_backend(self, backend, stem=None):
        self.VGG_model.set_backend(backend, stem)
        self.backend, self.stem_backend = self.VGG_model.backend, self.VGG_model.stem_backend
        return self

    def set_conv_dtype(self, conv_dtype):
        self.VGG_model.set_conv_dtype(conv_dtype)
        self.conv_dtype = conv_dtype
        return self

    def _check_tokens(self, n):
        if n > self.num_patches:
            raise ValueError(f"VGGFormer: the extractor's map has {n} positions but pos_embedding holds num_patches = "
                             f"{self.num_patches} (a 112 x 112 frame gives 4 x 4, a 224 x 224 frame 7 x 7)")

    def forward(self, x):
        if x.dim() == 5:
            x = x.contiguous().view(-1, *x.shape[2:])                                  # vggformer.py:270-271
        ops._need_cuda(x)
        if self.backend == "torch":
            x = self.conv(self.VGG_model(x))                                           # vggformer.py:273-274
            b_l, c, h, w = x.shape
            self._check_tokens(h * w)
            x = x.reshape((b_l, c, h * w)).permute(0, 2, 1)
            x = x + self.pos_embedding[:, :h * w]
            x = self.spatial_transformer(x.contiguous())
            x = x.permute(0, 2, 1).reshape((b_l, c, h, w))
            return torch.flatten(self.avgpool(x), 1)                                   # vggformer.py:287-293
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("VGGFormer(backend='hip'): the frozen extractor is forward-only and its input requires grad - "
                               "detach it; backend='torch' differentiates")
        m = self.VGG_model.forward_nhwc(x, out_dtype=_map_dtype(self.conv_dtype))      # [B', h, w, 2048]: its rows are the tokens
        b_l, n = m.shape[0], m.shape[1] * m.shape[2]
        self._check_tokens(n)
        t = _Conv1x1Fn.apply(m.view(b_l * n, m.shape[3]), self.conv.weight, self.conv_dtype == "bf16")
        t = _AssembleFn.apply(t.view(b_l, n, self.dim), None, self.pos_embedding)      # + pos_embedding[:, :n]
        return self.spatial_transformer(t, pool='mean')
