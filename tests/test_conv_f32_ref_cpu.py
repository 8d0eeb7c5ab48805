"""CPU (no GPU needed): the references of tests/conv_f32_util.py are what they claim, its cases are not vacuous and reach their
tiles, and its two checks bite - the derived element-wise bound refuses every indexing mutant of conv_util, the 1e-6 cap
against the emulated bf16x3 product refuses every arithmetic mutant (which the bound alone does not: see that module's docstring),
while fp32 simulations of the correct arithmetic pass both with margin."""
import pytest
import torch

import conv_f32_util as fu
import conv_util as cu

# the shapes the arithmetic figures in conv_f32_util's docstring were measured on: the eight small ones and the first big one
ARITH_CASES = [c for c in fu.CASES if c["tile"] == 1] + [c for c in fu.CASES if c["tile"] == 0][:1]


def _by_id(cases):
    return dict(argvalues=cases, ids=[c["id"] for c in cases])


@pytest.mark.parametrize("case", **_by_id(fu.CASES))
def test_case_is_not_vacuous_and_reaches_its_tile(case):
    fu.guard(case)
    assert cu.expected_tile(case) == case["tile"]


def test_the_cases_cover_every_instantiation_and_shape():
    assert len({(c["tile"], c["res"], c["relu"]) for c in fu.CASES}) == 8
    assert {c["shape_id"] for c in fu.CASES} == set(cu.SMALL_SHAPES) | set(cu.BIG_SHAPES)
    o = fu.operands(fu.CASES[0])
    for t in (o["x"], o["w"]):  # neither operand is bf16-exact: both splits are part of the test
        assert float((t.bfloat16().float() != t).float().mean()) > 0.9


@pytest.mark.parametrize("shape", cu.SMALL_SHAPES + cu.BIG_SHAPES[:1], ids=str)
def test_exact_reference_is_conv2d_and_emulated_is_within_the_per_product_bound(shape):
    N, H, W, Cin, Cout, k, s = shape
    case = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, relu=False, res=None, shape_id=shape)
    o = fu.operands(case)
    want = torch.nn.functional.conv2d(o["x"].double().permute(0, 3, 1, 2), o["w"].double().permute(0, 3, 1, 2), stride=s,
                                      padding=1 if k == 3 else 0).permute(0, 2, 3, 1)
    P, magP, E, _ = fu.products(case)
    assert tuple(want.shape[1:3]) == cu.out_hw(H, W, k, s)
    assert float((P - want.reshape(P.shape)).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool(((E - P).abs() <= fu.PER_PRODUCT_BOUND * magP).all())
    assert fu.rel_fro(E, P) > 1e-7  # ... and E is not P: the cap below is measured against the arithmetic, not the exact product


@pytest.mark.parametrize("case", **_by_id(fu.CASES))
def test_bound_passes_the_arithmetic_and_refuses_every_indexing_mutant(case):
    (exact, _), rows = fu.reference(case), cu.mutant_rows(case)
    assert fu.ratio(fu.simulate_index(case, None, rows), exact, rows) <= 1.0
    for name, applies in cu.MUTANTS.items():
        if applies(case):
            assert fu.ratio(fu.simulate_index(case, name, rows), exact, rows) > 1.0, name


def test_every_indexing_mutant_applies_somewhere():
    for name, applies in cu.MUTANTS.items():
        assert sum(applies(c) for c in fu.CASES) >= 2, name


@pytest.mark.parametrize("case", **_by_id(ARITH_CASES))
def test_cap_sits_between_the_correct_arithmetic_and_every_arithmetic_mutant(case):
    exact, emulated = fu.reference(case)
    for order in ("chunks", "torch"):
        got = fu.simulate_arith(case, None, order)
        err = fu.rel_fro(got, emulated)
        print(f"CONVF32SIM {case['id']} {order} rel_fro {err:.3e} ratio {fu.ratio(got, exact):.3f}")
        assert err <= fu.CAP / 2 and fu.ratio(got, exact) <= 1.0
    for name in fu.ARITH_MUTANTS:
        err = fu.rel_fro(fu.simulate_arith(case, name), emulated)
        print(f"CONVF32SIM {case['id']} {name} rel_fro {err:.3e}")
        assert err >= 10 * fu.CAP, name


def test_the_element_wise_bound_alone_does_not_refuse_a_wrong_arithmetic():
    """why the cap exists: a split by truncation stays well inside the derived bound on the exact product on every shape, and a
    dropped cross term passes it by a margin that shrinks like 1 / sqrt(K) (1.3 x at K = 864, the deepest reduction here)"""
    for c in ARITH_CASES:
        assert fu.ratio(fu.simulate_arith(c, "split_by_truncation"), fu.reference(c)[0]) <= 0.5, c["id"]
    deep = next(c for c in ARITH_CASES if c["k"] ** 2 * c["Cin"] == 864)
    assert fu.ratio(fu.simulate_arith(deep, "lo_x_hi_w_dropped"), fu.reference(deep)[0]) <= 2.0
