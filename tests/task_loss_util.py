"""Shared by test_task_losses_cpu.py and test_gpu_task_losses.py: the criteria of fixture G17 (tests/golden/
make_golden_task_losses.py) as this package builds them, and the project's bounds for a loss kernel."""
import torch

import avformer_amd as A

# test_gpu_ops.py::test_au_loss_golden
LOSS_TOL = dict(atol=1e-6, rtol=1e-5)
GRAD_TOL = dict(atol=1e-7, rtol=1e-5)

EX_WEIGHT = [2.62, 26.5, 45, 40, 4.0, 5.87, 1.0]
EX, AU, VA = slice(12, 19), slice(0, 12), slice(19, 21)
CASES = ("b16", "b64", "mix", "exign", "va1")


def _va(w):
    return dict(make=lambda: A.CCCLoss(), label="y_va", cols=VA,
                torch=lambda c, o, y: c.forward_rows_torch(o, y.to(o.dtype), (w, 1.0)),
                rows=lambda c, o, y: c.forward_rows(o, y, (w, 1.0)))


def _ex(make):
    return dict(make=make, label="y_ex", cols=EX, torch=lambda c, o, y: c.forward_torch(o[:, EX], y),
                rows=lambda c, o, y: c.forward_rows(o, y), alone=lambda c, o, y: c(o[:, EX], y))


def _au(make):
    return dict(make=make, label="y_au", cols=AU, torch=lambda c, o, y: c.forward_torch(o[:, AU], y),
                rows=lambda c, o, y: c.forward_rows(o, y), alone=lambda c, o, y: c(o[:, AU], y))


# name -> how to build the criterion, which labels it takes, its column block, its plain-torch form on the [B, 21] rows, its
# kernel form on the rows and (where the reference's own signature differs) on the sliced input
CRITERIA = {
    "ce": _ex(lambda: A.CrossEntropyEX(ignore_index=7)),
    "cew": _ex(lambda: A.CrossEntropyEX(weight=EX_WEIGHT, ignore_index=7)),
    "focal": _ex(lambda: A.FocalLoss_Ori(num_class=7, gamma=2.0, ignore_index=7, reduction='mean')),
    "focal0": _ex(lambda: A.FocalLoss_Ori(num_class=7, alpha=0.25, gamma=2)),
    "aubce": _au(lambda: A.AULoss()),
    "dice": _au(lambda: A.DiceAULoss()),
    "va21": _va(2.0),
    "va11": _va(1.0),
    "ccc": dict(make=lambda: A.CCCLoss(), label="y_va", cols=slice(19, 20),
                torch=lambda c, o, y: c.forward_torch(o[:, 19], y[:, 0].to(o.dtype)),
                alone=lambda c, o, y: c(o[:, 19], y[:, 0])),
}


def fixture_pairs(g):
    """every (case, criterion) the fixture holds"""
    return [(case, name) for case in CASES for name in CRITERIA if f"{case}.{name}.loss" in g]


def assert_same_kind_close(got, ref, what, **tol):
    """NaN where the reference has NaN, exact zeros where it has exact zeros - compared by kind -, the rest within tol"""
    got, ref = torch.as_tensor(got).detach().cpu().to(torch.float64), torch.as_tensor(ref).detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern differs"
    if bool(torch.isnan(ref).all()):
        return
    if float(ref.nan_to_num(0.0).abs().max()) == 0.0:
        assert float(got.nan_to_num(0.0).abs().max()) == 0.0, f"{what}: expected exact zeros"
        return
    torch.testing.assert_close(got, ref, equal_nan=True, msg=lambda m: f"{what}: {m}", **tol)


def loss_and_grad(fn, out):
    o = out.clone().requires_grad_(True)
    loss = fn(o)
    if loss.requires_grad:
        (g,) = torch.autograd.grad(loss, o, allow_unused=True)
    else:
        g = None
    return loss.detach(), (torch.zeros_like(out) if g is None else g)
