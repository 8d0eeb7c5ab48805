"""Shared by tests/test_vggformer_cpu.py and tests/test_gpu_vggformer.py: the G22 fixtures (tests/golden/make_golden_vggformer.py,
made from the reference's own ``Bottleneck`` / ``VGGFace2_extractor``) and the modules built for them."""
import os

import numpy as np
import torch
from torch import nn

import avformer_amd as A
from conftest import GOLDEN


def g22_chain_fixture():
    """-> (state dict of the chain, x [2, 48, 7, 5], y [2, 128, 4, 3])"""
    z = np.load(os.path.join(GOLDEN, "g22_bottleneck.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}
    return sd, torch.from_numpy(z["x"]), torch.from_numpy(z["y"])


def g22_chain(backend, conv_dtype="bf16"):
    """the chain of the fixture: Bottleneck(48, 16, 1, down 48 -> 64), Bottleneck(64, 16), Bottleneck(64, 32, 2, down 64 -> 128)"""
    def down(cin, cout, stride):
        return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(cout))

    kw = dict(backend=backend, conv_dtype=conv_dtype)
    return nn.Sequential(A.FrozenBottleneck(48, 16, 1, down(48, 64, 1), **kw), A.FrozenBottleneck(64, 16, **kw),
                         A.FrozenBottleneck(64, 32, 2, down(64, 128, 2), **kw))


def g22_stem_fixture():
    """-> (state dict with conv1.* / bn1.* keys, [(x, y), (x, y)]): [2, 3, 30, 45] -> [2, 64, 7, 11], [2, 3, 28, 20] -> [2, 64, 7, 5]"""
    z = np.load(os.path.join(GOLDEN, "g22_stem.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}
    return sd, [(torch.from_numpy(z["xa"]), torch.from_numpy(z["ya"])), (torch.from_numpy(z["xb"]), torch.from_numpy(z["yb"]))]


def randomise_batchnorm(module, generator):
    """non-trivial eval-mode statistics, drawn as tests/golden/make_golden_backbone.py draws them (a fresh BatchNorm2d is the
    identity); the last BatchNorm of a Bottleneck and its downsample get gammas of a third of that, which keeps the activations
    of a 16-block residual chain of order 1"""
    for name, m in module.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            damp = 1.0 / 3.0 if name.endswith("bn3") or name.endswith("downsample.1") else 1.0
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(n, generator=generator) * 0.3)
                m.running_var.copy_(torch.rand(n, generator=generator) * 1.5 + 0.5)
                m.weight.copy_((torch.rand(n, generator=generator) + 0.5) * damp)
                m.bias.copy_(torch.randn(n, generator=generator) * 0.3)


def extractor(backend="torch", seed=5, **kw):
    """``FrozenVGGFace2`` with its reference initialisation and randomised BatchNorm statistics"""
    torch.manual_seed(seed)
    m = A.FrozenVGGFace2(backend=backend, **kw)
    randomise_batchnorm(m, torch.Generator().manual_seed(seed + 1))
    return m


def vggformer(backend="torch", seed=5, **kw):
    torch.manual_seed(seed)
    m = A.VGGFormer(backend=backend, **kw)
    randomise_batchnorm(m.VGG_model, torch.Generator().manual_seed(seed + 1))
    return m


def frames(n=2, c=3, size=112, seed=3):
    return torch.randn(n, c, size, size, generator=torch.Generator().manual_seed(seed))


def rel_fro(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())
