"""No device: the reference, bounds and bit-for-bit checks of tests/gemm_mx8_util.py pass a correctly computed result in every
data family, epilogue and C type, refuse every mutant a subtly wrong MX-FP8 GEMM kernel would produce, and the exact families
have the properties their exactness rests on.  The role tests/test_gemm_nt_ref_cpu.py has for the bf16 NT GEMM."""
import pytest
import torch

import gemm_mx8_util as X
import gemm_nt_util as G

BF, F32 = torch.bfloat16, torch.float32
# tile 5 (96 x 128): three row tiles and a ragged fourth, two column tiles and a ragged third, three K-steps; ldc = N + 8
M, N, K = 300, 264, 384
TILE = (96, 128)
LDC = N + 8
P_DROP = 0.2
NI = N // 32 * 32  # the columns an MX-FP8 image of C covers in whole blocks
EPIS = (X.EPI_NONE, X.EPI_BIAS_RES, X.EPI_BIAS_GELU, X.EPI_DGELU)

_images = {}


def _img(family):
    if family not in _images:
        img = X.make_images(M, N, K, 500 + X.FAMILIES.index(family), family)
        _images[family] = (img, X.products(img))
    return _images[family]


def _inputs(family, epi, cdt):
    return X.make_inputs(M, N, K, 1000 + 10 * X.FAMILIES.index(family) + epi, family, cdt, epi, _img(family)[0])


def _factors(epi):
    return X.make_factors(M, N, LDC, P_DROP, 7 + epi)


@pytest.mark.parametrize("cdt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("epi", EPIS, ids=[X.EPI_NAMES[e] for e in EPIS])
@pytest.mark.parametrize("family", X.FAMILIES)
def test_reference_passes_its_own_checks(family, epi, cdt):
    inp = _inputs(family, epi, cdt)
    prod = _img(family)[1]
    for drop in ((False, True) if epi != X.EPI_NONE else (False,)):
        f, f_ldc = _factors(epi) if drop else (None, None)
        ref = X.reference(inp, f, prod)
        if drop and family == "dense-int":
            X.mask_not_vacuous(ref)
        c, aux, cs, _ = X.simulate(inp, f, f_ldc, tile=TILE)
        stats = X.check_outputs(f"{family}/{X.EPI_NAMES[epi]}", ref, c, aux, cs)
        assert stats["C"] <= 1.0 and stats["colsum"] <= 0.5, stats
        assert torch.isfinite(c.float()).all()
        if family in X.EXACT_FAMILIES:
            n = X.check_exact(f"{family}/{X.EPI_NAMES[epi]}", inp, prod, c, aux, dropout=drop)
            assert n >= 1 or epi != X.EPI_NONE


def test_dense_int_accumulates_exactly_in_fp32():
    """every partial sum is an integer times 2^-9 below 2^24, so an fp32 accumulator holds P in any order: an fp32 matmul of
    the dequantised operands equals the fp64 one bit for bit, also with K reversed; u = P + bias is in the GELU's live range"""
    import oracle
    img, (P, magP) = _img("dense-int")
    assert torch.equal((P * 512).round(), P * 512) and float(magP.max()) * 512 < 2.0 ** 24
    a, b = oracle.mx8_dequant(img["aq"], img["as_"]), oracle.mx8_dequant(img["bq"], img["bs"])
    assert torch.equal((a @ b.t()).double(), P) and torch.equal((a.flip(1) @ b.flip(1).t()).double(), P)
    # the terms of one instruction (four 32-blocks of a row pair) span at most 2^8
    assert int(img["as_"].max()) - int(img["as_"].min()) <= 3 and int(img["bs"].max()) - int(img["bs"].min()) <= 3
    assert float(a.abs().max() / a.abs()[a != 0].min()) <= 16 and float(b.abs().max() / b.abs()[b != 0].min()) <= 16
    assert 1.0 < float(P.std()) < 3.0
    assert set(img["as_"].unique().tolist()) == {127, 128, 129, 130} and set(img["bs"].unique().tolist()) == {118, 119, 120, 121}


@pytest.mark.parametrize("family", ["sparse-a", "sparse-b"])
def test_one_block_wide_products_are_exact_fp32_normals(family):
    img, (P, magP) = _img(family)
    sparse, dense = (img["as_"], img["bs"]) if family == "sparse-a" else (img["bs"], img["as_"])
    assert bool(((sparse != 0).sum(1) == 1).all()) and bool((dense != 0).all())
    q = img["aq"] if family == "sparse-a" else img["bq"]
    assert bool((q.view(-1, K // 32, 32)[sparse == 0] == 0).all())  # zero blocks: zero bytes under scale byte 0
    live = torch.cat([sparse[sparse != 0], dense.flatten()])
    assert 87 <= int(live.min()) and int(live.max()) <= 167 and int(live.max()) - int(live.min()) > 70
    nz = P[P != 0].abs()
    assert float(nz.min()) >= 2.0 ** -126 and float(nz.max()) < 2.0 ** 127  # fp32 normals
    assert float(nz.min()) < 1e-20 and float(nz.max()) > 1e20              # ... over the E8M0 range the family spans
    assert float((P != 0).double().mean()) >= 0.9
    assert torch.equal(P.float().double(), P)  # an fp32 value: 2^(sa + sb - 254) times a small integer


def test_unit_family_makes_the_quantised_value_the_stored_one():
    """u = P + 64 in [8, 256] and P in [-256, 256] are integers: bf16 values, where the fast GELU forms return u and 1"""
    _, (P, _) = _img("unit")
    assert torch.equal(P.round(), P) and float(P.abs().max()) <= 56
    u = P + X.UNIT_BIAS
    assert torch.equal(u.float().bfloat16().double(), u) and torch.equal(P.float().bfloat16().double(), P)
    assert float(P.abs().max()) >= 4  # block maxima differ: more than one scale byte in the image
    assert len(X.expected_image(P[:, :256])[1].unique()) >= 2


def _applicable(name):
    side, epi, need_drop, _ = X.MUTANTS[name]
    epis = [epi] if epi is not None else ([e for e in EPIS if e != X.EPI_NONE] if need_drop else list(EPIS))
    # "unit" has one scale byte everywhere (it exists for the image of a bf16 C): a misplaced scale cannot show there
    fams = X.FAMILIES if side == "operand" else ("dense-int",)
    if "scale" in name:
        fams = tuple(f for f in fams if f != "unit")
    return fams, [(e, cdt) for e in epis for cdt in (BF, F32)]


@pytest.mark.parametrize("name", sorted(X.MUTANTS))
def test_every_mutant_fails(name):
    side, _, need_drop, _ = X.MUTANTS[name]
    fams, cases = _applicable(name)
    for family in fams:
        prod = _img(family)[1]
        for epi, cdt in cases:
            if side == "operand" and family != "dense-int" and epi != X.EPI_NONE:
                continue  # the other families run EPI_NONE on the device
            inp = _inputs(family, epi, cdt)
            f, f_ldc = _factors(epi) if need_drop else (None, None)
            ref = X.reference(inp, f, prod)
            what = f"{name}/{family}/{X.EPI_NAMES[epi]}/{cdt}"
            c, aux, cs, _ = X.simulate(inp, f, f_ldc, tile=TILE)
            X.check_outputs(what, ref, c, aux, cs)  # the same case unmutated passes
            c, aux, cs, _ = X.simulate(inp, f, f_ldc, mutant=name, tile=TILE)
            with pytest.raises(AssertionError, match="error / bound above 1"):
                X.check_outputs(what, ref, c, aux, cs)
            if side == "operand" and family in X.EXACT_FAMILIES and epi == X.EPI_NONE:
                with pytest.raises(AssertionError, match="bit for bit"):
                    X.check_exact(what, inp, prod, c, aux)


@pytest.mark.parametrize("epi", [X.EPI_BIAS_GELU, X.EPI_DGELU], ids=["bias_gelu", "dgelu"])
def test_image_checks_tell_the_two_sources_apart(epi):
    """the contract (the fp32 value is quantised) against an image of the rounded bf16 value, both ways, on "dense-int";
    on "unit" the two coincide, which is what lets a bf16-C run be checked at all"""
    inp = _inputs("dense-int", epi, BF)
    prod = _img("dense-int")[1]
    c, _, _, good = X.simulate(inp, tile=TILE, image="fp32")
    _, _, _, bad = X.simulate(inp, tile=TILE, image="bf16")
    v = X.reference(inp, None, prod)["C"].float()[:, :NI]
    c = c[:, :NI]
    assert X.image_contracts_differ(v)
    X.check_image("fp32 contract", v, *good)
    with pytest.raises(AssertionError, match="MX-FP8 image"):
        X.check_image("fp32 contract", v, *bad)
    X.check_image("bf16 contract", c.float(), *bad)
    with pytest.raises(AssertionError, match="MX-FP8 image"):
        X.check_image("bf16 contract", c.float(), *good)
    inp = _inputs("unit", epi, BF)
    c, _, _, img = X.simulate(inp, tile=TILE, image="fp32")
    assert not X.image_contracts_differ(X.reference(inp, None, _img("unit")[1])["C"].float()[:, :NI])
    X.check_image("unit", c.float()[:, :NI], *img)
    X.check_exact("unit", inp, _img("unit")[1], c, X.simulate(inp, tile=TILE)[1])


def test_the_plan_names_every_variant_the_gpu_test_lists():
    """host code only: avf_gemm_mx8_nt_plan (the launcher's own decision) sends the shapes of tests/test_gpu_gemm_mx8.py to
    the tile and LEAN code that file names"""
    import avformer_amd as A
    A._build.build()
    plan = A.ops.gemm_mx8_plan
    for name, (tile, lean_tile, shapes) in X.VARIANTS.items():
        for (m, n, k) in shapes:
            for cdt in (BF, F32):
                for epi in EPIS:
                    got = plan(m, n, k, cdt, epi, bias=epi != X.EPI_DGELU, ldc=n + 8, ldres=n + 8, ldaux=n + 8)
                    assert got == dict(tile=tile, lean=1 if lean_tile else 0), (name, m, n, k, epi, got)
                if lean_tile:
                    assert plan(m, n, k, cdt, X.EPI_DGELU, bias=False, want_colsum=True)["lean"] == 3
                    assert plan(m, n, k, cdt, X.EPI_DGELU, bias=False, want_colsum=True, want_image=True)["lean"] == 7
                    assert plan(m, n, k, cdt, X.EPI_BIAS_GELU, want_image=True)["lean"] == 5
                    assert plan(m, n, k, cdt, X.EPI_BIAS_GELU, p=0.2)["lean"] == 0
                    assert plan(m, n, k, cdt, X.EPI_NONE, want_colsum=True)["lean"] == 0


def test_every_tile_of_the_table_is_some_shapes_own_plan():
    """host code only: the tile ids this kernel has (asked with each id forced; the three-stage tile 6 is the bf16 kernel's)
    are exactly the ones tests/test_gpu_gemm_mx8.py lists, and each is what avf_gemm_mx8_nt_plan picks UNFORCED for some shape"""
    import os
    import avformer_amd as A
    A._build.build()
    held = G.tile_ids_held(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))["mx8"]
    assert held == {1, 2, 5}, held
    picked = set()
    for (m, n), tile in G.PLAN_SHAPES.items():
        for k in (384, 1536):
            plan = A.ops.gemm_mx8_plan(m, n, k)
            assert plan["tile"] == (5 if tile is None else tile), (m, n, k, plan)
            picked.add(plan["tile"])
    assert picked == held, (picked, held)
