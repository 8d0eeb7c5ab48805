#!/usr/bin/env python3
"""Generate the backbone fixtures from the REFERENCE's own ``vformer.BasicBlock`` / ``vformer.ResFormer`` (models/vformer.py:128-268),
imported unmodified through make_golden.load_reference:

    python tests/golden/make_golden_backbone.py

g20_basicblock.npz       Sequential(BasicBlock(32, 48, stride=2, downsample=conv1x1 + BatchNorm2d), BasicBlock(48, 48)) in eval():
                         the input [2, 32, 7, 5], every state_dict entry ("p." + key) and the output, fp32.  Running means,
                         variances, gammas and betas are set to non-trivial values first (a fresh BatchNorm2d is the identity).
g20_resformer_keys.json  [[key, shape], ...] of ResFormer(BasicBlock, [2, 2, 2, 2]).state_dict()

Data only: no program text of the reference is stored."""
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def main():
    _, _, _, vformer = mg.load_reference()
    torch.manual_seed(1020)
    down = nn.Sequential(vformer.conv1x1(32, 48, 2), nn.BatchNorm2d(48))
    chain = nn.Sequential(vformer.BasicBlock(32, 48, stride=2, downsample=down), vformer.BasicBlock(48, 48))
    for m in chain.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(torch.randn(n) * 0.3)
            m.running_var.copy_(torch.rand(n) * 1.5 + 0.5)
            m.weight.data.copy_(torch.rand(n) + 0.5)
            m.bias.data.copy_(torch.randn(n) * 0.3)
    chain.eval()
    x = torch.randn(2, 32, 7, 5)
    with torch.no_grad():
        y = chain(x)
    arrays = {"p." + k: v.float() for k, v in chain.state_dict().items()}
    mg.save("g20_basicblock", x=x, y=y, **arrays)
    print("output", tuple(y.shape), "abs mean %.3f max %.3f, zeros %.2f" % (y.abs().mean(), y.abs().max(), (y == 0).float().mean()))

    sd = vformer.ResFormer(vformer.BasicBlock, [2, 2, 2, 2]).state_dict()
    path = os.path.join(mg.OUT, "g20_resformer_keys.json")
    with open(path, "w") as f:
        json.dump([[k, list(v.shape)] for k, v in sd.items()], f, indent=0)
    print(f"wrote {path} ({len(sd)} keys)")


if __name__ == "__main__":
    main()
