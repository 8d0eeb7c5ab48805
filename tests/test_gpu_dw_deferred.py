"""The deferred weight gradients of the bf16 stack: the dW GEMMs of several layers in one launch (avf_layer_bwd_dx +
avf_layers_dw, planned by transformer.plan_dw_groups), which at four layers of 64 tiles fills one round of the chip
without a split of the token reduction - no partial slabs, no slab fold.

Tolerances
  ops level:   the one tests/test_gpu_ops.py::test_gemm_tn_group uses for the same K (atol 2e-5 K, rtol 1e-5 against the fp64
               product of the bf16 operands).
  stack level: the caps tests/test_gpu_transformer.py::test_transformer_vs_oracle applies to the per-layer bf16 path
               (relative Frobenius error 1.5e-2 on y, 3e-2 on dx, 4e-2 on each parameter gradient, against the fp64-free CPU
               oracle the existing stack tests use).  Between the deferred and the per-layer path the dX chain is the same
               code on the same inputs: loss and dx are bit-equal.  The weight gradients sum the same bf16 products, in one fp32
               chain instead of (up to) eight chains plus a fold: each element differs by at most ~K * 2^-24 of the sum of the
               magnitudes of its products (K = 320 token rows here: 2e-5), so the relative Frobenius distance of a tensor is
               held to 1e-4; the column folds (biases, LayerNorm affine) are the same kernels on the same partial rows and
               are bit-equal.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import oracle
from gpu_util import DEV, check_rel, oracle_transformer_run, rel_fro

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQ = lambda y: y.pow(2).mean()
L, N, D, H, DH, M = 6, 40, 128, 4, 32, 256
# B = 2 is the issue's case: 80 token rows are no multiple of the 64-row K-step, the layers keep their own launches whatever
# the switches say.  B = 8 (320 rows) is the smallest batch of this shape at which the grouped launch, and with it the
# deferral, engages.
BATCHES = (2, 8)


def test_plan_groups_fill_one_round_exactly_or_less():
    """CPU: the plan from the top layer down.  C2 / C3: 64 tiles per layer on the 256 slots of the 256 x 128 kernel -> 4 + 2;
    C4: 144 tiles per layer -> every layer on its own; no group of more than one layer exceeds one round"""
    from avformer_amd.transformer import plan_dw_groups
    assert plan_dw_groups(6, 64, 256) == [4, 2]
    assert plan_dw_groups(12, 144, 256) == [1] * 12
    assert plan_dw_groups(12, 64, 256) == [4, 4, 4]
    assert plan_dw_groups(5, 64, 256) == [4, 1]
    assert plan_dw_groups(3, 100, 256) == [2, 1]
    assert plan_dw_groups(2, 300, 256) == [1, 1]
    assert plan_dw_groups(6, 8, 512) == [4, 2]          # the argument block holds four layers
    assert plan_dw_groups(6, 64, 256, force=2) == [2, 2, 2]
    assert plan_dw_groups(6, 64, 256, force=6) == [4, 2]
    assert plan_dw_groups(6, 64, 256, force=1) == [1] * 6
    assert plan_dw_groups(0, 64, 256) == []
    for n in range(1, 14):
        for tiles in (1, 8, 63, 64, 65, 128, 129, 144, 256, 257):
            for slots in (256, 512):
                plan = plan_dw_groups(n, tiles, slots)
                assert sum(plan) == n and all(1 <= g <= 4 for g in plan)
                assert all(g == 1 or g * tiles <= slots for g in plan), (n, tiles, slots, plan)


_OPS_CHILD = r'''
import os, sys, torch
sys.path.insert(0, %r)
import avformer_amd as A
SHAPES = [(136, 72), (256, 128), (264, 136), (512, 64)]
for splits in ("1", "2"):
    os.environ["AVF_TN_SPLITS"] = splits   # 1: every tile stores straight to C; 2: two slabs and the slab fold
    for count in (8, 16):
        for K in (64, 192, 2624):
            g = torch.Generator().manual_seed(K + count)
            shapes = [SHAPES[(i + i // 4) %% 4] for i in range(count)]
            pairs = [(torch.randn(K, m, generator=g).bfloat16(), torch.randn(K, n, generator=g).bfloat16()) for m, n in shapes]
            outs = A.ops.gemm_tn_group([(a.cuda(), b.cuda()) for a, b in pairs])
            for i, ((a, b), c) in enumerate(zip(pairs, outs)):
                ref = (a.double().t() @ b.double()).float()
                err = (c.cpu() - ref).abs().max().item()
                print("ops", splits, count, K, i, tuple(ref.shape), "max abs err %%.3e" %% err, flush=True)
                torch.testing.assert_close(c.cpu(), ref, atol=2e-5 * K, rtol=1e-5)
del os.environ["AVF_TN_SPLITS"]
print("TN_GROUP16_OK")
'''


@pytest.mark.gpu
def test_gemm_tn_group_8_and_16_problems():
    """ops.gemm_tn_group with 8 and 16 problems against fp64 products, edges of both tile shapes, K of one K-step, three, and
    41 (a multiple of 64 but not of 256); AVF_TN_SPLITS = 1 (direct store) and 2 (slabs) - a tuning switch, honoured under
    AVF_TUNING=1 only, which a process reads at its first library call: a child process"""
    r = subprocess.run([sys.executable, "-c", _OPS_CHILD % REPO], capture_output=True, text=True,
                       env=dict(os.environ, AVF_TUNING="1"), timeout=600)
    assert r.returncode == 0 and "TN_GROUP16_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@functools.lru_cache(maxsize=None)
def _case(B):
    """state, input and the oracle's results for the stack at batch B (computed once, shared, never modified)"""
    g = torch.Generator().manual_seed(321 + B)
    sd = oracle.init_transformer_state(D, L, H, DH, M, generator=g)
    for k in sd:  # non-trivial LayerNorm affine so the dgamma / dbeta folds are exercised
        if k.endswith("norm.weight"):
            sd[k] = 1 + 0.1 * torch.randn(D, generator=g)
        if k.endswith("norm.bias"):
            sd[k] = 0.1 * torch.randn(D, generator=g)
    x = torch.randn(B, N, D, generator=g)
    return sd, x, oracle_transformer_run(x, sd, L, H, SQ)


def _stack(sd):
    import avformer_amd as A
    t = A.Transformer(D, L, H, DH, M, 0.0, compute_dtype="bf16", residual_dtype="bf16")
    t.load_state_dict(sd, strict=True)
    return t.to(DEV)


def _run(t, x):
    """-> loss, dx, {name: grad} (clones: a later run must not alias them), and the plan backward used"""
    x = x.detach().to(DEV).clone().requires_grad_(True)
    for p in t.parameters():
        p.grad = None
    loss = SQ(t(x))
    loss.backward()
    torch.cuda.synchronize()
    plan = t.__dict__.get("_dw_plan_cache", (None, None, [1] * L))[2]
    return loss.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in t.named_parameters()}, list(plan)


@functools.lru_cache(maxsize=None)
def _per_layer(B):
    """the per-layer path (AVF_DW_DEFER=0) on the case of batch B, run once"""
    sd, x, _ = _case(B)
    old = os.environ.get("AVF_DW_DEFER")
    os.environ["AVF_DW_DEFER"] = "0"
    try:
        out = _run(_stack(sd), x)
    finally:
        if old is None:
            del os.environ["AVF_DW_DEFER"]
        else:
            os.environ["AVF_DW_DEFER"] = old
    assert out[3] == [1] * L
    return out


EXPECTED_PLAN = {"1": [1] * 6, "2": [2, 2, 2], "4": [4, 2], "6": [4, 2]}


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("group", ["off", "1", "2", "4", "6"])
def test_stack_gradients_vs_oracle(monkeypatch, B, group):
    sd, x, (y_ref, dx_ref, g_ref) = _case(B)
    loss0, dx0, g0, _ = _per_layer(B)
    if group == "off":
        monkeypatch.setenv("AVF_DW_DEFER", "0")
    else:
        monkeypatch.delenv("AVF_DW_DEFER", raising=False)
        monkeypatch.setenv("AVF_DW_GROUP", group)
    loss, dx, grads, plan = _run(_stack(sd), x)
    assert plan == (EXPECTED_PLAN[group] if (group != "off" and B % 8 == 0) else [1] * L), plan
    tag = f"dw_deferred[B{B},g{group}]"
    print(f"{tag}: plan {plan} loss {loss.item():.6e} dx rel {rel_fro(dx, dx_ref):.3e}")
    for k, v in g_ref.items():
        print(f"{tag}: g.{k} vs oracle {rel_fro(grads[k], v):.3e} vs per-layer {rel_fro(grads[k], g0[k]):.3e}")
    check_rel(f"{tag}:dx", dx, dx_ref, 3e-2)
    for k, v in g_ref.items():
        check_rel(f"{tag}:g.{k}", grads[k], v, 4e-2)
    # the dX chain is untouched
    assert torch.equal(loss, loss0) and torch.equal(dx, dx0)
    for k in g0:
        if grads[k].dim() == 1:
            assert torch.equal(grads[k], g0[k]), k          # column folds: same kernels, same partial rows
        else:
            assert rel_fro(grads[k], g0[k]) <= 1e-4, (k, rel_fro(grads[k], g0[k]))
    if plan == [1] * L:
        for k in g0:
            assert torch.equal(grads[k], g0[k]), k


@pytest.mark.gpu
def test_deferred_gradients_repeat_bit_for_bit(monkeypatch):
    sd, x, _ = _case(8)
    monkeypatch.delenv("AVF_DW_DEFER", raising=False)
    monkeypatch.setenv("AVF_DW_GROUP", "4")
    t = _stack(sd)
    l1, dx1, g1, plan = _run(t, x)
    l2, dx2, g2, _ = _run(t, x)            # same module: the cached operand blocks are reused
    l3, dx3, g3, _ = _run(_stack(sd), x)   # a fresh module: fresh blocks
    assert plan == [4, 2]
    for l, dx, g in ((l2, dx2, g2), (l3, dx3, g3)):
        assert torch.equal(l, l1) and torch.equal(dx, dx1)
        for k in g1:
            assert torch.equal(g[k], g1[k]), k


@pytest.mark.gpu
def test_captured_step_equals_eager_deferred_step(monkeypatch):
    """graphs.GraphedTrainStep records the deferred backward (operand blocks, descriptors and the per-layer gradient images are
    fixed addresses of the capture); Adam at lr 0 keeps the weights, so every replay must give the eager step's gradients"""
    import avformer_amd as A
    sd, x, _ = _case(8)
    monkeypatch.delenv("AVF_DW_DEFER", raising=False)
    monkeypatch.setenv("AVF_DW_GROUP", "4")
    _, _, g_eager, plan = _run(_stack(sd), x)
    assert plan == [4, 2]
    t = _stack(sd)
    opt = torch.optim.Adam(t.parameters(), lr=0.0, fused=True, capturable=True)
    batch = {"x": x.to(DEV)}
    step = A.graphs.GraphedTrainStep(t, opt, lambda m, b: SQ(m(b["x"])), batch, warmup=2)
    for _ in range(2):
        step(batch)
        torch.cuda.synchronize()
        for k, p in t.named_parameters():
            assert torch.equal(p.grad, g_eager[k]), k


@pytest.mark.gpu
def test_gradient_hook_switches_deferral_off(monkeypatch):
    sd, x, _ = _case(8)
    _, dx0, g0, _ = _per_layer(8)
    monkeypatch.delenv("AVF_DW_DEFER", raising=False)
    monkeypatch.setenv("AVF_DW_GROUP", "4")
    t = _stack(sd)
    seen = []
    t.set_grad_hook(lambda l, flat: seen.append((l, flat.numel())) and None)
    t.__dict__.pop("_dw_plan_cache", None)
    _, dx, grads, _ = _run(t, x)
    assert [l for l, _ in seen] == list(reversed(range(L)))            # each layer handed over as soon as it is done, top down
    assert len({n for _, n in seen}) == 1
    assert "_dw_plan_cache" not in t.__dict__                            # no plan was made: every layer ran its own launch
    assert torch.equal(dx, dx0)
    for k in g0:
        assert torch.equal(grads[k], g0[k]), k


_SPLIT_CHILD = r'''
import os, sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import test_gpu_dw_deferred as T
sd, x, _ = T._case(8)
_, dx0, g0, _ = T._per_layer(8)
os.environ["AVF_TN_SPLITS"] = "2"     # the groups of four and of two layers on two slabs: slab fold + 12 / 6 column folds, one launch
os.environ["AVF_DW_GROUP"] = "4"
_, dx, g, plan = T._run(T._stack(sd), x)
assert plan == [4, 2], plan
assert torch.equal(dx, dx0)
for k in g0:
    d = T.rel_fro(g[k], g0[k])
    print("split2", k, "%%.3e" %% d, flush=True)
    assert (torch.equal(g[k], g0[k]) if g[k].dim() == 1 else d <= 1e-4), (k, d)
print("DW_SPLIT2_OK")
'''


@pytest.mark.gpu
def test_deferred_group_on_two_slabs():
    """the deferred groups forced onto two K-ranges (AVF_TN_SPLITS=2 under AVF_TUNING=1: a child process), as the two-layer
    group of the full-size stack runs: the slab fold of 16 / 8 problems with the layers' column folds in the same launch"""
    r = subprocess.run([sys.executable, "-c", _SPLIT_CHILD % (REPO, REPO)], capture_output=True, text=True,
                       env=dict(os.environ, AVF_TUNING="1"), timeout=600)
    assert r.returncode == 0 and "DW_SPLIT2_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
