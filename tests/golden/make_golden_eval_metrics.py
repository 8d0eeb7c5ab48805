#!/usr/bin/env python3
"""Generate tests/golden/g18_eval_metrics.npz from the REFERENCE implementation (see make_golden.py for how the reference's
modules are imported unmodified; this script reuses its loader and writer and is run the same way, in the build container
only):

    python tests/golden/make_golden_eval_metrics.py

G18: the three metric classes that the reference's evaluate() builds (train.py:111-113: AccF1Metric(ignore_index=7),
CCCMetric(ignore_index=-5.0), MultiLabelAccF1(ignore_index=-1); metrics/accf1.py and metrics/cccmetric.py, numpy + sklearn)
fed batch by batch exactly as train.py:150-155 feeds them - argmax of columns 12..18, tanh of columns 19..20,
np.round(sigmoid) of columns 0..11, all on CPU fp32 - and scored as train.py:160-164.  Data only.  Per case:

    <case>.out [batches, B, 21] fp32   <case>.y_ex [batches, B] int64   <case>.y_au [batches, B, 12] fp32   <case>.y_va [batches, B, 2] fp32
    <case>.ex_acc .ex_f1 .ex_score  .au_acc .au_f1 .au_score  .ccc_v .ccc_a .va_score     fp64 scalars (NaN where the reference
                                                                                          returns NaN)
    <case>.ccc_v64 .ccc_a64            CCCMetric on the SAME prediction / label arrays cast to fp64 (the reference's own fp32
                                       rounding is the difference to .ccc_v / .ccc_a)

Cases:

    eq       4 x 32, nothing ignored
    mix      3 x 48 with ignored EX rows (7), -1 among the AU labels, AU unit 7 wholly unlabelled, -5 in either VA column
    exabs    EX classes absent from the labels (4, 6), from the predictions (3) and from both (5)
    exign    every EX row ignored
    va1      exactly one valid row in each VA column
    va02     no valid row in the valence column, two in the arousal column
    vaconst  valence: logits 0 and labels 0 (the denominator is the 1e-8 alone); arousal: constant labels 0.5
    ties     EX logits on a coarse grid, rows with all seven equal among them: argmax ties
    auedge   AU logits drawn from +0, -0, -2^-22, +2^-22, +-60, +-inf

No AU logit of any case lies inside (0, 2^-22), where fp32 sigmoid implementations round differently.
"""
import os
import sys
import warnings

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _load_standalone, save  # noqa: E402


def make_case(name, nb, B, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(nb, B, 21, generator=g)
    y_ex = torch.randint(0, 7, (nb, B), generator=g)
    y_au = (torch.rand(nb, B, 12, generator=g) > 0.6).float()
    y_va = torch.rand(nb, B, 2, generator=g) * 2 - 1
    if name == "mix":
        y_ex[:, ::5] = 7
        y_au[torch.rand(nb, B, 12, generator=g) < 0.15] = -1
        y_au[:, :, 7] = -1
        y_au[:, 3::9] = -1
        y_va[:, ::7] = -5.0
        y_va[:, 2::9, 1] = -5.0
    elif name == "exabs":
        y_ex = torch.randint(0, 4, (nb, B), generator=g)
        out[:, :, 12 + 3] = -10.0
        out[:, :, 12 + 5] = -10.0
    elif name == "exign":
        y_ex[:] = 7
    elif name == "va1":
        y_va[:] = -5.0
        y_va[0, 5, 0] = 0.3
        y_va[1, 9, 1] = -0.7
    elif name == "va02":
        y_va[:] = -5.0
        y_va[0, 3, 1] = 0.25
        y_va[1, 11, 1] = -0.5
    elif name == "vaconst":
        out[:, :, 19] = 0.0
        y_va[:, :, 0] = 0.0
        y_va[:, :, 1] = 0.5
    elif name == "ties":
        out[:, :, 12:19] = torch.round(out[:, :, 12:19])
        out[:, ::6, 12:19] = 1.0
    elif name == "auedge":
        vals = torch.tensor([0.0, -0.0, -2.0 ** -22, 2.0 ** -22, 60.0, -60.0, float("inf"), float("-inf")])
        out[:, :, :12] = vals[torch.randint(0, len(vals), (nb, B, 12), generator=g)]
    au = out[:, :, :12]
    assert not bool(((au > 0) & (au < 2.0 ** -22)).any())
    return out, y_ex, y_au, y_va


CASES = {"eq": (4, 32), "mix": (3, 48), "exabs": (2, 40), "exign": (2, 16), "va1": (2, 16), "va02": (2, 16), "vaconst": (2, 24),
         "ties": (2, 36), "auedge": (2, 32)}


def main():
    accf1 = _load_standalone("ref_accf1", os.path.join(REF, "metrics", "accf1.py"))
    cccm = _load_standalone("ref_cccmetric", os.path.join(REF, "metrics", "cccmetric.py"))
    arrays = {}
    for i, (name, (nb, B)) in enumerate(CASES.items()):
        out, y_ex, y_au, y_va = make_case(name, nb, B, 1801 + i)
        arrays.update({f"{name}.out": out, f"{name}.y_ex": y_ex, f"{name}.y_au": y_au, f"{name}.y_va": y_va})
        m_ex, m_va, m_au = accf1.AccF1Metric(ignore_index=7), cccm.CCCMetric(ignore_index=-5.0), accf1.MultiLabelAccF1(ignore_index=-1)
        m_va64 = cccm.CCCMetric(ignore_index=-5.0)
        for b in range(nb):
            result = out[b]
            logits_ex, logits_au, logits_va = result[:, 12:19], result[:, :12], result[:, 19:21]
            # train.py:150-155
            pred = torch.argmax(logits_ex, dim=1).detach().cpu().numpy().reshape(-1)
            label = y_ex[b].detach().cpu().numpy().reshape(-1)
            m_ex.update(pred, label)
            va_pred, va_true = torch.tanh(logits_va).detach().cpu().numpy(), y_va[b].detach().cpu().numpy()
            m_va.update(y_pred=va_pred, y_true=va_true)
            m_va64.update(y_pred=va_pred.astype(np.float64), y_true=va_true.astype(np.float64))
            m_au.update(y_pred=np.round(torch.sigmoid(logits_au).detach().cpu().numpy()), y_true=y_au[b].detach().cpu().numpy())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            acc_ex, f1_ex = m_ex.get()
            acc_au, f1_au = m_au.get()
            ccc = m_va.get()
            ccc64 = m_va64.get()
        res = {"ex_acc": acc_ex, "ex_f1": f1_ex, "ex_score": 0.67 * f1_ex + 0.33 * acc_ex,     # train.py:162
               "au_acc": acc_au, "au_f1": f1_au, "au_score": 0.5 * f1_au + 0.5 * acc_au,       # train.py:163
               "ccc_v": ccc[0], "ccc_a": ccc[1], "va_score": ccc[2],                           # train.py:164
               "ccc_v64": ccc64[0], "ccc_a64": ccc64[1]}
        for k, v in res.items():
            arrays[f"{name}.{k}"] = np.float64(v)
        print(name, {k: float(v) for k, v in res.items()})
    save("g18_eval_metrics", **arrays)


if __name__ == "__main__":
    main()
