#!/usr/bin/env python3
"""Generate the vggformer fixtures (G22) from the REFERENCE's own ``vggformer.Bottleneck`` / ``vggformer.VGGFace2_extractor`` /
``vggformer.VGGFormer`` (models/vggformer.py:25-115, 250-296), imported unmodified (make_golden.load_reference for the
torchvision stub and the package the relative imports resolve in, then make_golden._load_standalone):

    python tests/golden/make_golden_vggformer.py

g22_bottleneck.npz        Sequential(Bottleneck(48, 16, 1, downsample 48 -> 64), Bottleneck(64, 16), Bottleneck(64, 32, 2, downsample
                          64 -> 128)) in eval(): the input x [2, 48, 7, 5], every state_dict entry ("p." + key) and the output y
                          [2, 128, 4, 3], fp32.  Running means, variances, gammas and betas are set to non-trivial values first, as
                          make_golden_backbone.py does; at least a quarter of the outputs are non-zero (asserted).
g22_stem.npz              the extractor's own conv1 / bn1 / relu / maxpool (3x3 / 2 / pad 0, ceil_mode) with such statistics, eval():
                          "p." + key of conv1 and bn1, the inputs xa [2, 3, 30, 45] (odd conv map 15 x 23) and xb [2, 3, 28, 20]
                          (even conv map 14 x 10: the last window in each direction is partial) and the outputs ya, yb.
g22_vggformer_keys.json   [[key, shape], ...] of VGGFormer().state_dict()

The whole extractor is 103 MB of weights and is not a fixture.  Data only: no program text of the reference is stored."""
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def randomise_batchnorm(module):
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(torch.randn(n) * 0.3)
            m.running_var.copy_(torch.rand(n) * 1.5 + 0.5)
            m.weight.data.copy_(torch.rand(n) + 0.5)
            m.bias.data.copy_(torch.randn(n) * 0.3)


def main():
    mg.load_reference()
    vgg = mg._load_standalone("refmodels.vggformer", os.path.join(mg.REF, "models", "vggformer.py"))
    torch.manual_seed(1022)

    def down(cin, cout, stride):
        return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(cout))

    chain = nn.Sequential(vgg.Bottleneck(48, 16, 1, down(48, 64, 1)), vgg.Bottleneck(64, 16), vgg.Bottleneck(64, 32, 2, down(64, 128, 2)))
    randomise_batchnorm(chain)
    chain.eval()
    x = torch.randn(2, 48, 7, 5)
    with torch.no_grad():
        y = chain(x)
    assert tuple(y.shape) == (2, 128, 4, 3) and float((y != 0).float().mean()) >= 0.25, (y.shape, float((y != 0).float().mean()))
    mg.save("g22_bottleneck", x=x, y=y, **{"p." + k: v.float() for k, v in chain.state_dict().items()})
    print("chain output", tuple(y.shape), "abs mean %.3f max %.3f, zeros %.2f" % (y.abs().mean(), y.abs().max(), (y == 0).float().mean()))

    ext = vgg.VGGFace2_extractor()
    stem = nn.Sequential(ext.conv1, ext.bn1, ext.relu, ext.maxpool)
    randomise_batchnorm(stem)
    stem.eval()
    xa, xb = torch.randn(2, 3, 30, 45), torch.randn(2, 3, 28, 20)
    with torch.no_grad():
        ya, yb = stem(xa), stem(xb)
    assert tuple(ya.shape) == (2, 64, 7, 11) and tuple(yb.shape) == (2, 64, 7, 5), (ya.shape, yb.shape)
    arrays = {"p.conv1." + k: v.float() for k, v in ext.conv1.state_dict().items()}
    arrays.update({"p.bn1." + k: v.float() for k, v in ext.bn1.state_dict().items()})
    mg.save("g22_stem", xa=xa, ya=ya, xb=xb, yb=yb, **arrays)

    sd = vgg.VGGFormer().state_dict()
    path = os.path.join(mg.OUT, "g22_vggformer_keys.json")
    with open(path, "w") as f:
        json.dump([[k, list(v.shape)] for k, v in sd.items()], f, indent=0)
    print(f"wrote {path} ({len(sd)} keys)")


if __name__ == "__main__":
    main()
