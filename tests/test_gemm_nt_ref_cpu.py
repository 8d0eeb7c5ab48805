"""No device: the fp64 reference and the element-wise bounds of tests/gemm_nt_util.py pass a correctly rounded result for every
data family, epilogue and C type, and refuse every mutant a subtly wrong NT GEMM kernel would produce (the list in that
module).  The role tests/test_layernorm_ref_cpu.py has for LayerNorm.  And the launcher's own plan query (avf_gemm_nt_plan: host
code) confirms that every tile of the table is some shape's unforced pick."""
import pytest
import torch

import gemm_nt_util as G

BF, F32 = torch.bfloat16, torch.float32
# two 128-row tiles and a ragged third, two 128-column tiles and a ragged third, two K-steps; ldc = N + 8
M, N, K = 300, 264, 128
LDC = N + 8
P_DROP = 0.2
EPIS = (G.EPI_NONE, G.EPI_BIAS_RES, G.EPI_BIAS_GELU, G.EPI_DGELU)


def _inputs(family, epi, cdt):
    return G.make_inputs(M, N, K, 1000 + 10 * G.FAMILIES.index(family) + epi, family, cdt, epi)


def _factors(epi):
    return G.make_factors(M, N, LDC, P_DROP, 7 + epi)


@pytest.mark.parametrize("cdt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("epi", EPIS, ids=[G.EPI_NAMES[e] for e in EPIS])
@pytest.mark.parametrize("family", G.FAMILIES)
def test_reference_passes_its_own_bounds(family, epi, cdt):
    inp = _inputs(family, epi, cdt)
    for drop in ((False, True) if epi != G.EPI_NONE else (False,)):
        f, f_ldc = _factors(epi) if drop else (None, None)
        ref = G.reference(inp, f)
        if drop:
            G.mask_not_vacuous(ref)
        c, aux, cs = G.simulate(inp, f, f_ldc)
        stats = G.check_outputs(f"{family}/{G.EPI_NAMES[epi]}", ref, c, aux, cs)
        # rounding alone stays well inside: the bounds are not tuned to the rounding of this very reference
        assert stats["C"] <= 1.0 and stats["colsum"] <= 0.5, stats
        assert torch.isfinite(c.float()).all()


def test_bf16_bound_is_half_an_ulp():
    """the bf16 term of the bound is met with equality by a tie and is below 2^-8 |x| everywhere; 2^-9 |x| is not a bound"""
    x = torch.tensor([1.0 + 2.0 ** -8, 1.5 + 2.0 ** -8, 2.0 - 2.0 ** -8, 3.0, 1e-3, 100.0], dtype=torch.float64)
    zero = torch.zeros_like(x)
    bound = G.bf16_bound(x, zero)
    err = (x.float().bfloat16().double() - x).abs()
    assert bool((err <= bound).all()) and float(err[0]) == float(bound[0]) == 2.0 ** -8
    assert bool((bound <= 2.0 ** -8 * x).all()) and bool((bound > 2.0 ** -9 * x * (1 - 1e-12)).all())
    assert float(err[0]) > 2.0 ** -9 * float(x[0])


def test_dgelu_reference_at_the_saturated_ends():
    """gelu' is 0 at -8, -20, -1e4 and at 1 at 8, 20, 1e4 to fp32 accuracy, 0.5 at +-0: the special aux values are present and
    the reference is finite there"""
    inp = _inputs("normal", G.EPI_DGELU, F32)
    x = inp["aux_in"]
    for v in G.SPECIAL_AUX:
        assert int((x == v).sum()) >= 8, v
    d = G.dgelu_tanh(torch.tensor(G.SPECIAL_AUX, dtype=torch.float64))
    assert torch.isfinite(d).all()
    assert torch.allclose(d, torch.tensor([0.5, 0.5, 1, 0, 1, 0, 1, 0], dtype=torch.float64), atol=1e-9)
    # and the derivative matches a central difference of the forward form
    u = torch.linspace(-6, 6, 97, dtype=torch.float64)
    num = (G.gelu_tanh(u + 1e-6) - G.gelu_tanh(u - 1e-6)) / 2e-6
    assert float((num - G.dgelu_tanh(u)).abs().max()) < 1e-8
    assert float(G.dgelu_tanh(torch.linspace(-12, 12, 100001, dtype=torch.float64)).abs().max()) <= G.DGELU_MAX


def _applicable(name):
    epi, need_drop, _, bf_only = G.MUTANTS[name]
    epis = [epi] if epi is not None else ([e for e in EPIS if e != G.EPI_NONE] if need_drop else list(EPIS))
    return [(e, cdt) for e in epis for cdt in ((BF,) if bf_only else (BF, F32))]


# A duplicated row in the column sums is one term too many among M: where the product nearly cancels, the accumulation term
# of the bound (2 K U magP per element, summed over M rows) is larger than any single |C[M-1, n]|, so that family cannot see
# it; the other two must.
BLIND = {("colsum_dup_row", "cancel")}


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("name", sorted(G.MUTANTS))
def test_every_mutant_fails(name, family):
    _, need_drop, _, _ = G.MUTANTS[name]
    for epi, cdt in _applicable(name):
        inp = _inputs(family, epi, cdt)
        f, f_ldc = _factors(epi) if need_drop else (None, None)
        ref = G.reference(inp, f)
        what = f"{name}/{family}/{G.EPI_NAMES[epi]}/{cdt}"
        G.check_outputs(what, ref, *G.simulate(inp, f, f_ldc))  # the same case unmutated passes
        if (name, family) in BLIND:
            continue
        with pytest.raises(AssertionError, match="error / bound above 1"):
            G.check_outputs(what, ref, *G.simulate(inp, f, f_ldc, mutant=name))


def test_every_tile_of_the_table_is_some_shapes_own_plan():
    """host code only: the tile ids the table holds (asked with each id forced) are exactly the ones tests/test_gpu_gemm_nt.py
    lists, and each is what avf_gemm_nt_plan picks UNFORCED for some shape - a tile no input selects cannot sit in the table"""
    import os
    import avformer_amd as A
    A._build.build()
    held = G.tile_ids_held(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))["bf16"]
    assert held == {1, 2, 5, 6}, held
    picked = set()
    for (m, n), tile in G.PLAN_SHAPES.items():
        for k in (128, 512, 1536):
            plan = A.ops.gemm_nt_plan(m, n, k)
            assert plan["kind"] == 1 and plan["tile"] == (6 if tile is None else tile), (m, n, k, plan)
            picked.add(plan["tile"])
    assert picked == held, (picked, held)
