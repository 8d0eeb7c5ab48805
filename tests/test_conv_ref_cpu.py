"""CPU (no GPU needed): the fp64 reference of tests/conv_util.py is the reference's convolution + eval-mode BatchNorm, its cases
are not vacuous, and its element-wise bounds refuse every mutant - what tests/test_gpu_conv.py asserts of the device bites."""
import pytest
import torch

import conv_util as cu


def _by_id(cases):
    return dict(argvalues=cases, ids=[c["id"] for c in cases])


@pytest.mark.parametrize("case", **_by_id(cu.CASES))
def test_case_is_not_vacuous_and_reaches_its_tile(case):
    cu.guard(case)
    assert cu.expected_tile(case) == case["tile"]


def test_the_cases_cover_every_instantiation():
    seen = {(c["tile"], c["x"], c["out"], c["res"], c["relu"]) for c in cu.CASES}
    assert len(seen) == 2 * len(cu.COMBOS) == 48
    shapes = {c["shape_id"] for c in cu.CASES}
    assert shapes == set(cu.SMALL_SHAPES) | set(cu.BIG_SHAPES)


@pytest.mark.parametrize("shape", cu.SMALL_SHAPES + cu.BIG_SHAPES, ids=str)
def test_reference_is_conv2d_plus_eval_batchnorm(shape):
    N, H, W, Cin, Cout, k, s = shape
    case = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, relu=False, res=None, shape_id=shape)
    o = cu.operands(case)
    g = torch.Generator().manual_seed(5)
    gamma, beta = torch.rand(Cout, generator=g).double() + 0.5, torch.randn(Cout, generator=g).double()
    mean, var, eps = torch.randn(Cout, generator=g).double(), torch.rand(Cout, generator=g).double() + 0.5, 1e-5
    x = o["x"].bfloat16().double().permute(0, 3, 1, 2)
    w = o["w"].double().permute(0, 3, 1, 2)
    want = torch.nn.functional.conv2d(x, w, stride=s, padding=1 if k == 3 else 0)
    want = torch.nn.functional.batch_norm(want, mean, var, gamma, beta, False, 0.0, eps).permute(0, 2, 3, 1)
    scale = gamma / torch.sqrt(var + eps)
    P, magP, _ = cu.products(case)
    got = cu.epilogue(case, P, magP, scale, beta - mean * scale, None)["C"]
    assert tuple(want.shape[1:3]) == cu.out_hw(H, W, k, s)
    assert float((got - want.reshape(got.shape)).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("case", **_by_id(cu.CASES))
def test_bounds_pass_the_reference_and_refuse_every_mutant(case):
    ref, rows = cu.reference(case), cu.mutant_rows(case)
    assert cu.check("unmutated", ref, cu.simulate(case, None, rows), rows) <= 1.0
    for name, applies in cu.MUTANTS.items():
        if not applies(case):
            continue
        with pytest.raises(AssertionError):
            cu.check(name, ref, cu.simulate(case, name, rows), rows)


def test_every_mutant_applies_somewhere():
    for name, applies in cu.MUTANTS.items():
        assert sum(applies(c) for c in cu.CASES) >= 8, name


@pytest.mark.parametrize("HW,Cn,xd", cu.POOL_CASES)
def test_avgpool_bound(HW, Cn, xd):
    x = cu.pool_inputs(HW, Cn, xd)
    mean, b = cu.pool_reference(x)
    assert float(((cu.pool_simulate(x).double() - mean).abs() / b).max()) <= 1.0
    assert float(((cu.pool_simulate(x, "avgpool_wrong_count").double() - mean).abs() / b).max()) > 1.0
