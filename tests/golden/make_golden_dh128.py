#!/usr/bin/env python3
"""Generate tests/golden/g16_transformer_dh128.npz from the REFERENCE implementation (see make_golden.py for how the
reference's modules are imported unmodified; this script reuses its loader and writer and is run the same way, in the
build container only):

    python tests/golden/make_golden_dh128.py

G16: the reference's Transformer at dim_head 128 (dim 64, depth 2, 2 heads x 128, mlp 128; inner width 256 > dim),
B 2, N 20, loss y.pow(2).mean().  Data only: inputs, parameters, outputs and gradients as fp32.  The parameter gradients
go to a second file, g16_transformer_dh128_grads.npz, so that each file stays under the 1 MiB limit for a committed file
(random fp32 data does not compress); a reader merges the two.
"""
import os
import sys

import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import load_reference, module_io, save  # noqa: E402


def main():
    heads, _, _, _ = load_reference()
    torch.manual_seed(1600)
    tr = heads.Transformer(64, 2, 2, 128, 128)
    io = module_io(tr, torch.randn(2, 20, 64), lambda y: y.pow(2).mean())
    save("g16_transformer_dh128", dim=64, depth=2, heads=2, dim_head=128, mlp_dim=128,
         **{k: v for k, v in io.items() if not k.startswith("g.")})
    save("g16_transformer_dh128_grads", **{k: v for k, v in io.items() if k.startswith("g.")})


if __name__ == "__main__":
    main()
