#!/usr/bin/env python3
"""Generate the stem fixture from the REFERENCE's own ``vformer.ResFormer`` (models/vformer.py:168-268), imported unmodified
through make_golden.load_reference:

    python tests/golden/make_golden_stem.py

g21_stem.npz  conv1 - bn1 - relu - maxpool of ResFormer(BasicBlock, [2, 2, 2, 2]) in eval(), called in the order of
              ResFormer.forward (vformer.py:238-241): the input [2, 3, 37, 29] (odd conv map 19 x 15, pooled 10 x 8), conv1.weight
              and every bn1 entry ("p." + key), and the output [2, 64, 10, 8], fp32.  The running mean and variance, gamma and
              beta are set to non-trivial values first (a fresh BatchNorm2d is the identity).

Data only: no program text of the reference is stored."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def main():
    _, _, _, vformer = mg.load_reference()
    torch.manual_seed(1021)
    net = vformer.ResFormer(vformer.BasicBlock, [2, 2, 2, 2])
    m = net.bn1
    m.running_mean.copy_(torch.randn(64) * 0.3)
    m.running_var.copy_(torch.rand(64) * 1.5 + 0.5)
    m.weight.data.copy_(torch.rand(64) + 0.5)
    m.bias.data.copy_(torch.randn(64) * 0.3)
    net.eval()
    x = torch.randn(2, 3, 37, 29)
    with torch.no_grad():
        y = net.maxpool(net.relu(net.bn1(net.conv1(x))))
    arrays = {"p." + k: v.float() for k, v in net.state_dict().items() if k.split(".")[0] in ("conv1", "bn1")}
    mg.save("g21_stem", x=x, y=y, **arrays)
    print("output", tuple(y.shape), "abs mean %.3f max %.3f, zeros %.2f" % (y.abs().mean(), y.abs().max(), (y == 0).float().mean()))


if __name__ == "__main__":
    main()
