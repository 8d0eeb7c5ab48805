"""Shared by test_eval_metrics_cpu.py and test_gpu_eval_metrics.py: the cases of fixture G18 (tests/golden/
make_golden_eval_metrics.py), random case builders, and an fp64 two-pass checker of the evaluation scores written from the
formulas of the reference (metrics/accf1.py, metrics/cccmetric.py, train.py:150-164) - on the samples themselves, with no
statistics in between, so it shares nothing with EvalMetrics.update_torch.

Bounds.  Counts-derived scores (accuracy, F1 and their weighted sums) are a handful of fp64 operations on integers: 1e-12
absolute.  CCC from fp64 moments against the reference run on fp64 arrays: 1e-10.  Against the reference's own fp32 run: max(1e-6,
4 x |ref_fp32 - ref_fp64|), the gap taken per case from the fixture.  Moment slots of two accumulations that differ only in the
order of their fp64 additions: 1e-12 relative to the slot's sum of magnitudes (16 384 terms x 2^-53 = 1.8e-12 is the worst case of
any order; the orders compared here are blocked and stay well inside it).  Moment slots computed from a tanh that differs from
the checker's by at most u fp32 ulps: every x moves by at most u 2^-23 |x|, so sum x and sum x y move by at most u 2^-23 times
their sums of magnitudes and sum x^2 by twice that (to first order; the second-order term is 2^-23 of the first); n, sum y and
sum y^2 do not depend on x."""
import numpy as np
import torch

CASES = ("eq", "mix", "exabs", "exign", "va1", "va02", "vaconst", "ties", "auedge")
COUNT_TOL = 1e-12
CCC_TOL_FP64 = 1e-10
ORDER_TOL = 1e-12
AU_LO, AU_HI = 0.0, 2.0 ** -22   # the band of AU logits that is unspecified; no test puts a logit inside it
MUTANTS = ("f1_all7", "unbiased_var", "au_rowwise", "au_ge0")


def fixture_batches(G, case):
    """[(out [B, 21], {'EX', 'AU', 'VA'})] of a G18 case"""
    return [(G[f"{case}.out"][b], {"EX": G[f"{case}.y_ex"][b], "AU": G[f"{case}.y_au"][b], "VA": G[f"{case}.y_va"][b]})
            for b in range(G[f"{case}.out"].shape[0])]


def random_batch(rows, seed, width=21):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(rows, width, generator=g)
    y_ex = torch.randint(0, 8, (rows,), generator=g)                 # 7 = ignored
    y_au = (torch.rand(rows, 12, generator=g) > 0.6).float()
    y_au[torch.rand(rows, 12, generator=g) < 0.15] = -1
    y_va = torch.rand(rows, 2, generator=g) * 2 - 1
    y_va[torch.rand(rows, 2, generator=g) < 0.15] = -5.0
    au = out[:, :12]
    au[(au > AU_LO) & (au < AU_HI)] = AU_HI
    return out, {"EX": y_ex, "AU": y_au, "VA": y_va}


def au_prediction(x):
    """round(sigmoid(x)) in fp32 outside the unspecified band: 0 for x <= 0 (both zeros), 1 for x >= 2^-22"""
    assert not bool(((x > AU_LO) & (x < AU_HI)).any()), "an AU logit inside the unspecified band"
    return (x >= AU_HI).to(torch.float64)


def ccc_two_pass(x, y, ignore=-5.0, unbiased=False):
    """cccmetric.py:4-34 in fp64: mean first, then centred sums"""
    x, y = x.to(torch.float64).reshape(-1), y.to(torch.float64).reshape(-1)
    k = y != ignore
    x, y = x[k], y[k]
    n = x.numel()
    if n <= 1:
        return 0.0
    mx, my = x.sum() / n, y.sum() / n
    dx, dy = x - mx, y - my
    d = n - 1 if unbiased else n
    return float(2 * (dx * dy).sum() / n / ((dx * dx).sum() / d + (dy * dy).sum() / d + (mx - my) ** 2 + 1e-8))


def check_scores(batches, mutant=None, ex_ignore=7, au_ignore=-1.0, va_ignore=-5.0):
    """the scores of train.py:160-164 from the samples, fp64; `mutant` swaps in one of the wrong forms of MUTANTS"""
    out = torch.cat([b[0] for b in batches]).float()
    y_ex = torch.cat([b[1]["EX"] for b in batches]).long()
    y_au = torch.cat([b[1]["AU"] for b in batches]).to(torch.float64)
    y_va = torch.cat([b[1]["VA"] for b in batches]).float()
    nan = float("nan")
    # EX: accuracy and macro F1 over the classes among the kept rows' labels or predictions
    pred = torch.argmax(out[:, 12:19], dim=1)
    keep = (y_ex != ex_ignore) & (y_ex >= 0) & (y_ex < 7)
    p, t = pred[keep], y_ex[keep]
    ex_acc = float((p == t).double().mean()) if p.numel() else nan
    f1s = []
    for c in range(7):
        tp, fp, fn = int(((p == c) & (t == c)).sum()), int(((p == c) & (t != c)).sum()), int(((p != c) & (t == c)).sum())
        if tp + fp + fn > 0:
            f1s.append(2.0 * tp / (2 * tp + fp + fn))
        elif mutant == "f1_all7":
            f1s.append(0.0)
    ex_f1 = float(np.mean(f1s)) if f1s else nan
    # AU: entry by entry
    x_au = out[:, :12]
    pa = (x_au >= 0).to(torch.float64) if mutant == "au_ge0" else au_prediction(x_au)
    lab = y_au != au_ignore
    if mutant == "au_rowwise":
        lab = lab & (y_au[:, :1] != au_ignore)
    correct = int(((pa == y_au) & lab).sum())
    au_acc = correct / int(lab.sum()) if int(lab.sum()) else nan
    f1u = []
    for u in range(12):
        pu, tu = pa[:, u][lab[:, u]], y_au[:, u][lab[:, u]]
        tp, fp, fn = int(((pu == 1) & (tu == 1)).sum()), int(((pu == 1) & (tu != 1)).sum()), int(((pu != 1) & (tu == 1)).sum())
        f1u.append(2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else 0.0)
    au_f1 = float(np.mean(f1u))
    # VA on tanh in fp32
    xv = torch.tanh(out[:, 19:21])
    ccc = [ccc_two_pass(xv[:, j], y_va[:, j], va_ignore, unbiased=(mutant == "unbiased_var")) for j in range(2)]
    return {"ex_acc": ex_acc, "ex_f1": ex_f1, "ex_score": 0.67 * ex_f1 + 0.33 * ex_acc, "au_acc": au_acc, "au_f1": au_f1,
            "au_score": 0.5 * au_f1 + 0.5 * au_acc, "ccc_v": ccc[0], "ccc_a": ccc[1], "va_score": (ccc[0] + ccc[1]) / 2}


def same(a, b, tol):
    """NaN matches NaN only; else |a - b| <= tol"""
    a, b = float(a), float(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return abs(a - b) <= tol


def assert_scores_match_fixture(got, G, case, extra_ccc=0.0):
    """`got`: dict with the nine score names.  Counts-derived scores to COUNT_TOL; CCC to CCC_TOL_FP64 of the reference's fp64
    result and to max(1e-6, 4 x the reference's own fp32 gap) of its fp32 result; `extra_ccc` widens both CCC bounds (the device
    tanh term of the GPU tests)."""
    for k in ("ex_acc", "ex_f1", "ex_score", "au_acc", "au_f1", "au_score"):
        assert same(got[k], G[f"{case}.{k}"], COUNT_TOL), (case, k, got[k], G[f"{case}.{k}"])
    for k in ("ccc_v", "ccc_a"):
        r32, r64 = float(G[f"{case}.{k}"]), float(G[f"{case}.{k}64"])
        assert same(got[k], r64, CCC_TOL_FP64 + extra_ccc), (case, k, got[k], r64)
        assert same(got[k], r32, max(1e-6, 4 * abs(r32 - r64)) + extra_ccc), (case, k, got[k], r32, r64)
    r64 = (float(G[f"{case}.ccc_v64"]) + float(G[f"{case}.ccc_a64"])) / 2
    assert same(got["va_score"], r64, CCC_TOL_FP64 + extra_ccc), (case, "va_score", got["va_score"], r64)
    assert same(got["va_score"], G[f"{case}.va_score"], max(1e-6, 4 * abs(float(G[f"{case}.va_score"]) - r64)) + extra_ccc)


def flat_scores(scores):
    """EvalMetrics.scores() -> the nine names used here"""
    return {"ex_acc": scores["EX"]["EX:acc"], "ex_f1": scores["EX"]["f1"], "ex_score": scores["EX"]["score"],
            "au_acc": scores["AU"]["AU:acc"], "au_f1": scores["AU"]["f1"], "au_score": scores["AU"]["score"],
            "ccc_v": scores["VA"]["VA:ccc_v"], "ccc_a": scores["VA"]["ccc_a"], "score_va": scores["VA"]["score"],
            "va_score": scores["VA"]["score"]}


def moment_magnitudes(batches, va_ignore=-5.0):
    """[2, 6] fp64: per VA column the sums of |term| of n, sum x, sum y, sum x^2, sum y^2, sum x y (x = tanh in fp32)"""
    out = torch.cat([b[0] for b in batches]).float()
    y = torch.cat([b[1]["VA"] for b in batches]).to(torch.float64)
    x = torch.tanh(out[:, 19:21]).to(torch.float64)
    k = (y != va_ignore).to(torch.float64)
    return torch.stack([k.sum(0), (k * x.abs()).sum(0), (k * y.abs()).sum(0), (k * x * x).sum(0), (k * y * y).sum(0),
                        (k * (x * y).abs()).sum(0)], 1)


def moment_bounds(batches, tanh_ulps):
    """[2, 6] fp64: the bound of each moment slot for a tanh within `tanh_ulps` fp32 ulps of the checker's (module docstring)"""
    mag = moment_magnitudes(batches)
    w = torch.tensor([0.0, 1.0, 0.0, 2.0 * (1 + 2.0 ** -20), 0.0, 1.0], dtype=torch.float64) * tanh_ulps * 2.0 ** -23
    return mag * (w + ORDER_TOL)


def ccc_tanh_term(state, bounds):
    """first-order bound of the change of the two CCC values when the moment slots of `state` (fp64 [128]) move by at most
    `bounds` [2, 6]: sum over the slots of |d ccc / d slot| x bound, the derivative taken by autograd on the formula of the issue"""
    mom = state.detach().cpu().double()[109:121].reshape(2, 6).clone().requires_grad_(True)
    n, sx, sy, sxx, syy, sxy = mom.unbind(-1)
    nn = n.clamp(min=1)
    mx, my = sx / nn, sy / nn
    c = 2 * (sxy / nn - mx * my) / ((sxx / nn - mx * mx) + (syy / nn - my * my) + (mx - my) ** 2 + 1e-8)
    c = torch.where(n > 1, c, torch.zeros_like(c))
    (g,) = torch.autograd.grad(c.sum(), mom)
    return float((g.abs() * bounds).sum(1).max())


def ulps_between(a, b):
    """max |a - b| in units of the fp32 ulp of b (both fp32 tensors)"""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    ulp = torch.maximum(torch.abs(torch.nextafter(b, torch.full_like(b, float("inf"))) - b),
                        torch.full_like(b, 2.0 ** -149)).double()
    return float(((a.double() - b.double()).abs() / ulp).max())
