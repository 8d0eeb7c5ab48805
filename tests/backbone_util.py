"""Shared by tests/test_backbone_cpu.py and tests/test_gpu_backbone.py: the G20 fixture (tests/golden/make_golden_backbone.py) and
random but well-conditioned weights for a whole FrozenResFormer."""
import torch
from torch import nn

import avformer_amd as A
from conftest import load_golden, split_golden


def g20():
    """-> (state dict of the chain, input [2, 32, 7, 5], the reference's output [2, 48, 4, 3])"""
    p, _, r = split_golden(load_golden("g20_basicblock"))
    sd = {k: (torch.as_tensor(v, dtype=torch.long) if k.endswith("num_batches_tracked") else v) for k, v in p.items()}
    return sd, r["x"], r["y"]


def g20_chain(backend="torch"):
    """Sequential(BasicBlock(32, 48, stride=2, downsample=conv1x1 + BN), BasicBlock(48, 48)) as the generator builds it"""
    down = nn.Sequential(nn.Conv2d(32, 48, kernel_size=1, stride=2, bias=False), nn.BatchNorm2d(48))
    return nn.Sequential(A.FrozenBasicBlock(32, 48, stride=2, downsample=down, backend=backend),
                         A.FrozenBasicBlock(48, 48, backend=backend))


def randomize_batchnorm(module, seed):
    """Non-trivial BatchNorm2d statistics that keep the activations of order 1 through 17 convolutions: a kaiming-initialised
    conv doubles the variance of a ReLU'd input's half, so gammas 0.6 .. 1.0 over running variances 0.8 .. 1.6 hold the scale of
    each residual branch near 0.7 and the sum of branch and identity near 1 (checked on the CPU per stage: see
    tests/test_backbone_cpu.py::test_resformer_activations_neither_die_nor_blow_up)."""
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=g) * 0.8 + 0.8)
                m.weight.copy_(torch.rand(n, generator=g) * 0.4 + 0.6)
                m.bias.copy_(torch.randn(n, generator=g) * 0.2)
    return module


def resformer(backend, seed=2020):
    torch.manual_seed(seed)
    m = A.FrozenResFormer(backend=backend)
    return randomize_batchnorm(m, seed + 1).eval()
