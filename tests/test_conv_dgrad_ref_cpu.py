"""CPU (no GPU needed): the references of tests/conv_dgrad_util.py are what they claim - the index formula equals
torch.autograd of fp64 F.conv2d on every shape (the anchor that does not share the formula), and the FrozenBasicBlock backward
chain restated with it equals fp64 autograd of the torch block; its cases are not vacuous and reach their tiles; its bounds
bite: fp32 simulations of the correct kernel pass, every mutant is refused on every case it applies to."""
import pytest
import torch
from torch.nn import functional as F

import conv_dgrad_util as du
import conv_util as cu

ALL_SHAPES = du.SMALL_SHAPES + du.BIG_SHAPES + [du.SQUARE_SHAPE]


def _by_id(cases):
    return dict(argvalues=cases, ids=[c["id"] for c in cases])


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_reference_is_autograd_of_conv2d(shape):
    N, H, W, Cin, Cout, k, s = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Cin, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, dtype=torch.float64, generator=g)
    y = F.conv2d(x, w, stride=s, padding=1 if k == 3 else 0)
    assert tuple(y.shape[2:]) == cu.out_hw(H, W, k, s)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    want, = torch.autograd.grad(y, x, gy)
    got = du.dgrad(gy.permute(0, 2, 3, 1).contiguous(), du.wt_of(w), H, W, k, s)[0].reshape(N, H, W, Cin)
    assert float((got - want.permute(0, 2, 3, 1)).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


def _bn(c, g):
    return dict(weight=torch.rand(c, dtype=torch.float64, generator=g) + 0.5, bias=torch.randn(c, dtype=torch.float64, generator=g),
                mean=torch.randn(c, dtype=torch.float64, generator=g), var=torch.rand(c, dtype=torch.float64, generator=g) + 0.5)


@pytest.mark.parametrize("hw", [(7, 7), (8, 5), (4, 4), (1, 1), (2, 3)], ids=str)
@pytest.mark.parametrize("stride,down", [(1, False), (1, True), (2, True)])
def test_block_chain_is_autograd_of_the_torch_block(hw, stride, down):
    """FrozenBasicBlock.backward_nhwc's three launches, restated with the util, against fp64 autograd of BasicBlock.forward in
    eval mode; the block's input is a ReLU output and the result is gated by it"""
    g = torch.Generator().manual_seed(5)
    N, cin, planes, eps = 2, 6 if down else 5, 5, 1e-5
    H, W = hw
    ws = [torch.randn(planes, cin, 3, 3, dtype=torch.float64, generator=g) * 0.3,
          torch.randn(planes, planes, 3, 3, dtype=torch.float64, generator=g) * 0.3,
          torch.randn(planes, cin, 1, 1, dtype=torch.float64, generator=g) if down else None]
    bns = [_bn(planes, g), _bn(planes, g), _bn(planes, g) if down else None]
    pre = torch.randn(N, cin, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    x = F.relu(pre)

    def bn(t, b):
        return F.batch_norm(t, b["mean"], b["var"], b["weight"], b["bias"], False, 0.0, eps)

    h = F.relu(bn(F.conv2d(x, ws[0], stride=stride, padding=1), bns[0]))
    identity = bn(F.conv2d(x, ws[2], stride=stride), bns[2]) if down else x
    y = F.relu(bn(F.conv2d(h, ws[1], padding=1), bns[1]) + identity)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    want, = torch.autograd.grad(y, pre, dy)

    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    scales = [None if b is None else b["weight"] / torch.sqrt(b["var"] + eps) for b in bns]
    gs = nhwc(dy) * (nhwc(y) > 0)
    got = du.block_backward(gs, nhwc(h), ws, scales, (H, W), stride, x_gate=nhwc(x))
    assert float((got - nhwc(want)).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
    assert float(want.abs().max()) > 0 or H * W == 1


@pytest.mark.parametrize("case", **_by_id(du.CASES + [du.SQUARE_CASE]))
def test_case_is_not_vacuous_and_reaches_its_tile(case):
    du.guard(case)


def test_the_cases_cover_every_instantiation_and_shape():
    assert len({(c["tile"], c["gy"], c["out"], c["add"], c["gate"]) for c in du.CASES}) == 32
    assert len({(c["tile"], c["add"], c["gate"]) for c in du.F32_CASES}) == 8
    for cases in (du.CASES, du.F32_CASES):
        assert {c["shape_id"] for c in cases} == set(du.SMALL_SHAPES) | set(du.BIG_SHAPES)
    o = du.operands(du.CASES[0])
    for t in (o["gy"], o["wt_f32"]):  # not bf16-exact: the kernel's rounding (and both splits) are part of the test
        assert float((t.bfloat16().float() != t).float().mean()) > 0.9
    # stride-2 cases with all four parity classes, and even maps with a dropped edge tap, exist
    figs = [du.guard(c) for c in du.CASES if c["s"] == 2]
    assert any(f["parity_classes"] == 4 for f in figs) and any(f["dropped_edge_taps"] > 0 for f in figs)


@pytest.mark.parametrize("case", **_by_id(du.CASES + [du.SQUARE_CASE]))
def test_bound_passes_the_fp32_simulation_and_refuses_every_mutant(case):
    ref, rows = du.reference(case), du.mutant_rows(case)
    assert du.ratio(du.simulate_fp32(case), ref) <= 1.0
    assert du.ratio(du.simulate(case, None, rows), ref, rows) <= 1.0
    for name, applies in du.MUTANTS.items():
        if applies(case):
            assert du.ratio(du.simulate(case, name, rows), ref, rows) > 1.0, name


@pytest.mark.parametrize("case", **_by_id(du.F32_CASES))
def test_parity_checks_pass_the_fp32_simulation_and_the_bound_refuses_every_mutant(case):
    du.guard(case)
    (exact, emulated), rows = du.f32_reference(case), du.mutant_rows(case)
    sim = du.simulate_fp32(case, f32=True)
    assert du.ratio(sim, exact) <= 1.0 and du.rel_fro(sim, emulated) <= du.CAP
    assert du.rel_fro(emulated, exact["C"]) > 1e-7  # the emulation is not the exact product
    # an operand rounded to bf16 (the bf16 form's arithmetic) is what the cap refuses
    assert du.rel_fro(du.simulate_fp32(dict(case, out="f32")), emulated) > 10 * du.CAP
    for name, applies in du.MUTANTS.items():
        if applies(case):
            assert du.ratio(du.simulate(case, name, rows, f32=True), exact, rows) > 1.0, name


def test_every_mutant_applies_somewhere():
    for name, applies in du.MUTANTS.items():
        n = sum(applies(c) for c in du.CASES + [du.SQUARE_CASE])
        assert n >= (1 if name == "weight_not_transposed" else 2), name


@pytest.mark.parametrize("HW,Cn,od,gate", du.POOL_CASES)
def test_pool_backward_bound_passes_and_refuses_a_wrong_count(HW, Cn, od, gate):
    dout, gt = du.pool_inputs(HW, Cn, od, gate)
    if gate:
        assert float((gt == 0).double().mean()) >= 0.25 and float((gt > 0).double().mean()) >= 0.25
    du.pool_check("pool", du.pool_simulate(dout, HW, gt, od), dout, HW, gt)
    with pytest.raises(AssertionError):
        du.pool_check("pool", du.pool_simulate(dout, HW, gt, od, "avgpool_bwd_wrong_count"), dout, HW, gt)
