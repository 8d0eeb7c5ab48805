#!/usr/bin/env python3
"""Generate tests/golden/g17_task_losses.npz from the REFERENCE implementation (see make_golden.py for how the reference's
modules are imported unmodified; this script reuses its loader and writer and is run the same way, in the build container
only):

    python tests/golden/make_golden_task_losses.py

G17: the expression / action-unit / valence-arousal criteria of the reference's task models (models/loss.py) on random
[B, 21] output rows (AU logits 0..11, EX logits 12..18, valence / arousal 19..20), fp32.  Data only: per case the rows and
the three label arrays, per criterion the loss and d loss / d out restricted to the criterion's own column block (the rest of
the row has no gradient).  Cases:

    b16, b64   nothing ignored
    mix        B = 64 with ignored EX rows (7), dropped AU rows (first label -1), -1 among the other AU labels of kept rows,
               and -5 in either VA column
    exign      every EX row ignored
    va1        exactly one valid row in each VA column

Criteria (key = "<case>.<criterion>.loss" / ".dout"):

    ce      nn.CrossEntropyLoss(ignore_index=7)                       sformer.py:359
    cew     ... with the class weights of sformer.py:360 (b16 only)
    focal   FocalLoss_Ori(7, gamma=2.0, ignore_index=7)               avformer.py:89
    focal0  FocalLoss_Ori(7, alpha=0.25, gamma=2) (b16 only: without an ignore index every label must be a class)
    aubce   AULoss()                                                  avformer.py:90
    dice    DiceAULoss()                                              sformer.py:362
    va21    2 CCC(tanh v) + CCC(tanh a)                               avformer.py:119-123
    va11    CCC(tanh v) + CCC(tanh a)                                 sformer.py:415-421
    ccc     CCCLoss() on the raw column 19 against the valence labels (the criterion on its own; dout [B, 1])

"b64.mt" / "mix.mt": SpatialFormer.get_mt_loss (sformer.py:423-449, its own methods on its own three criteria) for normalize
False ("mt.loss" [3]) and True ("mtn.loss" [3]), and d (3 ex + au + va) / d out [B, 21] for both ("mt.dout", "mtn.dout";
the weights of train.py:147).
"""
import os
import sys
import types

import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _load_standalone, load_reference, save  # noqa: E402

EX_WEIGHT = [2.62, 26.5, 45, 40, 4.0, 5.87, 1.0]


def make_case(B, seed, mix=False, ex_all_ignored=False, va_one=False):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(B, 21, generator=g)
    y_ex = torch.randint(0, 7, (B,), generator=g)
    y_au = (torch.rand(B, 12, generator=g) > 0.6).float()
    y_va = torch.rand(B, 2, generator=g) * 2 - 1
    if mix:
        y_ex[::5] = 7
        y_au[3::9] = -1                      # whole rows unlabelled: dropped
        y_au[1::7, 4] = -1                   # a kept row with an unlabelled unit: the reference trains on the -1
        y_au[2::11, 0] = -1                  # first label only: dropped
        y_va[::7] = -5.0
        y_va[2::9, 1] = -5.0
    if ex_all_ignored:
        y_ex[:] = 7
    if va_one:
        y_va[:] = -5.0
        y_va[5, 0] = 0.3
        y_va[9, 1] = -0.7
    return out, y_ex, y_au, y_va


def run(fn, out, cols):
    o = out.clone().requires_grad_(True)
    loss = fn(o)
    (g,) = torch.autograd.grad(loss, o, allow_unused=True)
    g = torch.zeros_like(out) if g is None else g
    rest = torch.ones(out.shape[1], dtype=torch.bool)
    rest[cols] = False
    assert float(g[:, rest].abs().nan_to_num(1.0).max()) == 0.0
    return loss.detach(), g[:, cols].clone()


def main():
    _, L, _, _ = load_reference()
    torch.cuda.current_device = lambda: "cpu"  # the AULoss / DiceAULoss constructors ask for it
    sformer = _load_standalone("refmodels.sformer", os.path.join(REF, "models", "sformer.py"))
    ce, cew = torch.nn.CrossEntropyLoss(ignore_index=7), torch.nn.CrossEntropyLoss(weight=torch.tensor(EX_WEIGHT), ignore_index=7)
    focal = L.FocalLoss_Ori(num_class=7, gamma=2.0, ignore_index=7, reduction='mean')
    focal0 = L.FocalLoss_Ori(num_class=7, alpha=0.25, gamma=2)
    aubce, dice, ccc = L.AULoss(), L.DiceAULoss(), L.CCCLoss()
    EX, AU, VA = slice(12, 19), slice(0, 12), slice(19, 21)
    arrays = {}
    cases = {"b16": make_case(16, 1701), "b64": make_case(64, 1702), "mix": make_case(64, 1703, mix=True),
             "exign": make_case(16, 1704, ex_all_ignored=True), "va1": make_case(16, 1705, va_one=True)}
    for name, (out, y_ex, y_au, y_va) in cases.items():
        arrays.update({f"{name}.out": out, f"{name}.y_ex": y_ex, f"{name}.y_au": y_au, f"{name}.y_va": y_va})

        def va(w):
            return lambda o: w * ccc(torch.tanh(o[:, 19]), y_va[:, 0]) + ccc(torch.tanh(o[:, 20]), y_va[:, 1])
        crits = {"ce": (lambda o: ce(o[:, EX], y_ex), EX), "focal": (lambda o: focal(o[:, EX], y_ex), EX),
                 "aubce": (lambda o: aubce(o[:, AU], y_au), AU), "dice": (lambda o: dice(o[:, AU], y_au), AU),
                 "va21": (va(2), VA), "va11": (va(1), VA), "ccc": (lambda o: ccc(o[:, 19], y_va[:, 0]), slice(19, 20))}
        if name == "b16":
            crits.update({"cew": (lambda o: cew(o[:, EX], y_ex), EX), "focal0": (lambda o: focal0(o[:, EX], y_ex), EX)})
        for cname, (fn, cols) in crits.items():
            arrays[f"{name}.{cname}.loss"], arrays[f"{name}.{cname}.dout"] = run(fn, out, cols)
        if name in ("b64", "mix"):
            # the recipe of SpatialFormer (sformer.py:359-363) driven through its own get_*_loss / get_mt_loss
            m = types.SimpleNamespace(loss_EX=torch.nn.CrossEntropyLoss(ignore_index=7), loss_AU=L.DiceAULoss(), loss_VA=L.CCCLoss())
            for meth in ("get_ex_loss", "get_au_loss", "get_va_loss", "get_mt_loss"):
                setattr(m, meth, types.MethodType(getattr(sformer.SpatialFormer, meth), m))
            labels = {"EX": y_ex, "AU": y_au, "VA": y_va}
            for key, normalize in (("mt", False), ("mtn", True)):
                o = out.clone().requires_grad_(True)
                ls = m.get_mt_loss(o, labels, normalize=normalize)
                (3 * ls[0] + ls[1] + ls[2]).backward()
                arrays[f"{name}.{key}.loss"] = torch.stack([l.detach().float() for l in ls])
                arrays[f"{name}.{key}.dout"] = o.grad.clone()
    save("g17_task_losses", **arrays)


if __name__ == "__main__":
    main()
