"""No device: the fp64 reference and the element-wise bounds of tests/gemm_f32_util.py pass a correctly rounded result of
either arithmetic for every data family and epilogue; the "exact" family is what it claims to be; every mutant a subtly wrong
fp32 GEMM kernel would produce is refused somewhere in the GPU case table (the blind pairs are listed by name); and the plan
queries (host code only) name the kernel, split and access width every case of that table expects."""
import pytest
import torch

import avformer_amd as A
import gemm_f32_util as G
import gemm_nt_util as NT
from oracle import bf16x3 as X3

LDC_PAD = 8


def _find(name, orient=None):
    for i, c in enumerate(G.CASES):
        if c["name"] == name and (orient is None or c["orient"] == orient):
            return i, c
    raise KeyError(name)


def _setup(i, case, family, epi, drop):
    M, N, K = case["M"], case["N"], case["K"]
    a, w = G.make_operands(M, N, K, 100 + i, family, w_lo=case["kernel"] == "x3")
    inp = G.make_inputs(M, N, K, 200 + i, family, epi, (a, w), case["S"], case["kchunk"], res_row=case["res"] == "row")
    p = G.P_DROP_EXACT if family == "exact" else G.P_DROP
    f, f_ldc = NT.make_factors(M, N, N + LDC_PAD, p, 7 + epi) if drop else (None, None)
    return inp, G.products(a, w), f, f_ldc


# one case per kernel form: x3 unsplit (five K-steps), x3 ragged K, x3 split in three, T = 1, T = 1 split, T = 2 split
REPRESENTATIVE = [_find("x3", "TT")[0] + 4, _find("x3_ktail")[0], _find("x3_split3_ragged")[0], _find("t1", "NN")[0] + 2,
                  _find("t1_split")[0], _find("t2_split")[0]]


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("i", REPRESENTATIVE, ids=[G.case_id(G.CASES[i]) for i in REPRESENTATIVE])
def test_reference_passes_its_own_bounds(i, family):
    case = G.CASES[i]
    for epi in case["epis"]:
        if family == "exact" and epi not in (G.EPI_NONE, G.EPI_BIAS_RES):
            continue
        for drop in ((False, True) if epi != G.EPI_NONE else (False,)):
            inp, prod, f, f_ldc = _setup(i, case, family, epi, drop)
            c, aux = G.simulate(inp, case["kernel"], f, f_ldc)
            stats = G.check_case(f"{G.case_id(case)}/{family}/{G.EPI_NAMES[epi]}", inp, G.kernel_of(case), f, prod, c, aux)
            # rounding alone (and, against the exact product, the dropped terms of typical data) stays well inside
            assert all(v <= 0.5 for v in stats.values()), stats
            if drop:
                NT.mask_not_vacuous(G.reference(inp, "f32", f, prod))


@pytest.mark.parametrize("K", [32, 160, 520, 4096])
def test_exact_family_is_exact(K):
    """hi + lo == x with hi = h and lo = m 2^-12; the emulation is representable in fp32, differs from the exact product by
    lo_a lo_b, and equals an fp32 sum of the 3 K terms in a scrambled order and in chunks folded afterwards; with m = 0 in W the
    fp64 product itself is representable and equals the fp32 fmaf chain"""
    M, N = 12, 8
    a, w = G.exact_operands(M, N, K, K)
    for x in (a, w):
        hi, lo = X3.split(x)
        assert torch.equal(hi + lo, x) and torch.equal(hi, torch.round(x)) and bool((hi.abs() >= 1).all())
        assert torch.equal(lo * 4096, torch.round(lo * 4096)) and float(lo.abs().max()) <= 7 * 2.0 ** -12
    emu = X3.matmul(a, w.t())
    assert torch.equal(emu.float().double(), emu)
    exact = a.double() @ w.double().t()
    la, lw = X3.split(a)[1].double(), X3.split(w)[1].double()
    assert torch.equal(exact - emu, la @ lw.t()) and bool((exact != emu).any())
    (ah, al), (bh, bl) = X3.split(a), X3.split(w)
    terms = torch.cat([ah[:, None, :] * bh[None], ah[:, None, :] * bl[None], al[:, None, :] * bh[None]], 2)  # [M, N, 3 K] fp32
    g = torch.Generator().manual_seed(K)
    acc = torch.zeros(M, N)
    for k in torch.randperm(3 * K, generator=g).tolist():
        acc = acc + terms[:, :, k]
    assert torch.equal(acc, emu.float())
    chunks = [c.sum(2) for c in terms.flip(2).split(97, 2)]  # fp32 partial sums of 97 terms, then a fold
    fold = chunks[0]
    for c in chunks[1:]:
        fold = fold + c
    assert torch.equal(fold, emu.float())
    a0, w0 = G.exact_operands(M, N, K, K, w_lo=False)
    exact0 = a0.double() @ w0.double().t()
    assert torch.equal(exact0.float().double(), exact0) and torch.equal(X3.matmul(a0, w0.t()), exact0)
    chain = torch.zeros(M, N)
    for k in range(K):  # every product and every partial sum is exact: fmaf or not makes no difference
        chain = chain + a0[:, None, k] * w0[None, :, k]
    assert torch.equal(chain, exact0.float())


@pytest.mark.parametrize("name", ["t1", "t1_split", "t2_split"])
def test_fmaf_chain_emulation(name):
    """the chain the GPU test holds gemm_f32_kernel to bit for bit: on "exact" data (m = 0 in W) it is the fp64 product,
    split or not; on every other family it stays within the (K + S) U magP it is the worst case of - and is not the correctly
    rounded product, so the comparison says something"""
    i, case = _find(name)
    rows = G.chain_rows(case["M"])
    epi = case["epis"][-1] if name != "t1" else G.EPI_BIAS_RES
    for family in G.FAMILIES:
        inp, prod, _, _ = _setup(i, case, family, epi, False)
        got = G.fmaf_chain(inp, rows)
        ref = G.reference(inp, "f32", None, prod)
        if family == "exact":
            assert torch.equal(got.double(), ref["C"][rows])
            continue
        assert float(((got.double() - ref["C"][rows]).abs() / ref["bC"][rows]).max()) <= 1.0
        if case["K"] >= 100:
            assert not torch.equal(got, ref["C"][rows].float())


def test_tanhf_sits_well_inside_the_activation_term():
    """ACT = 16 was set for the exp2 / rcp forms of the bf16x3 kernel; gemm_f32_kernel's tanhf forms, evaluated in fp32 step by
    step as the device code does, use a small part of it"""
    u = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    uf = u.float()
    c, a = torch.tensor(NT._C, dtype=torch.float32), torch.tensor(NT._A, dtype=torch.float32)
    t = torch.tanh(c * (uf + a * uf * uf * uf))
    gelu = 0.5 * uf * (1.0 + t)
    dgelu = 0.5 * (1.0 + t) + 0.5 * uf * (1.0 - t * t) * c * (1.0 + 3.0 * a * uf * uf)
    bound = G.ACT * G.U * (1.0 + uf.double().abs())
    for got, ref in ((gelu, G.gelu_tanh(uf.double())), (dgelu, G.dgelu_tanh(uf.double()))):
        assert float(((got.double() - ref).abs() / bound).max()) < 0.5


def _applicable(name):
    """-> [(i, case, epi, drop)]: the first two cases of the GPU table per kernel the mutant applies to"""
    kernels, epi, need_drop, need_split, need_ragged = G.MUTANTS[name]
    out = []
    for kern in kernels:
        n = 0
        for i, case in enumerate(G.CASES):
            if G.kernel_of(case) != kern or (need_split and case["S"] == 1) or n == 2:
                continue
            if need_ragged and case["K"] % G.k_step(case["kernel"]) == 0:
                continue
            if name == "tiles_swapped" and case["M"] <= 128:
                continue
            if name == "residual_row_plus1" and case["res"] == "row":
                continue
            epis = [e for e in case["epis"] if (epi is None or e == epi) and not (need_drop and e == G.EPI_NONE)]
            if name == "residual_row_plus1":
                epis = [e for e in epis if e == G.EPI_BIAS_RES]
            if not epis:
                continue
            out.append((i, case, epis[0], need_drop))  # (NONE, or BIAS_RES with dropout: the epilogues every family runs)
            n += 1
    assert out, name
    return out


# (mutant, family) pairs NO applicable case refuses: the GELU epilogues do not run on "exact" data, so the two mutants of
# BIAS_GELU cannot be seen there.  Everything else is refused by every family, the arithmetic mutants at the K = 32 and K = 64
# cases (at K = 160 a truncating split is inside the emulation bound; a lost cross term is still 14 x outside).
BLIND = {("bias_shifted", "exact"), ("aux_masked", "exact")}


@pytest.mark.parametrize("name", sorted(G.MUTANTS))
def test_every_mutant_fails(name):
    refused = set()
    for i, case, epi, drop in _applicable(name):
        for family in G.FAMILIES:
            if family == "exact" and epi not in (G.EPI_NONE, G.EPI_BIAS_RES):
                continue
            inp, prod, f, f_ldc = _setup(i, case, family, epi, drop)
            what = f"{name}/{G.case_id(case)}/{family}/{G.EPI_NAMES[epi]}"
            kern = G.kernel_of(case)
            G.check_case(what, inp, kern, f, prod, *G.simulate(inp, case["kernel"], f, f_ldc))  # the same case unmutated passes
            try:
                G.check_case(what, inp, kern, f, prod, *G.simulate(inp, case["kernel"], f, f_ldc, mutant=name))
            except AssertionError as e:
                assert "error / bound above 1" in str(e) or isinstance(e, G.BitsDiffer), e
                refused.add(family)
    blind = {fam for fam in G.FAMILIES if (name, fam) in BLIND}
    assert refused == set(G.FAMILIES) - blind, (name, sorted(refused), sorted(blind))


@pytest.mark.parametrize("name", G.GROUP_MUTANTS)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_every_group_mutant_fails(name, family):
    shapes, K, _, S, _ = G.GROUP_CASES[0]
    pairs = []
    for j, (M, N) in enumerate(shapes):
        a, w = G.make_operands(M, N, K, 31 + j, family)
        pairs.append((a.t().contiguous(), w.t().contiguous()))
    prods = G.group_products(pairs)
    G.check_group(f"{name}/{family}", family, K, prods, G.simulate_group(pairs, S))
    with pytest.raises(AssertionError, match="error / bound above 1|differ from the exact result"):
        G.check_group(f"{name}/{family}", family, K, prods, G.simulate_group(pairs, S, mutant=name))


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    A._build.build()
    return A.ops


def _with_arith(mode):
    return A._lib.set_f32_arithmetic(mode)


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=[G.case_id(c) for c in G.CASES])
def test_plan_of_every_case(ops, i):
    """avf_gemm_f32_plan - the function the launcher acts on - for the layout the GPU test builds of every case"""
    case = G.CASES[i]
    M, N, K = case["M"], case["N"], case["K"]
    lda, ldb, ldc, ldres, ldaux = G.case_leading_dims(case)
    prev = _with_arith(case["arith"])
    try:
        for epi in case["epis"]:
            kw = dict(trans_a=case["ta"], trans_b=case["tb"], epilogue=epi, bias=epi != G.EPI_DGELU, lda=lda, ldb=ldb, ldc=ldc,
                      ldres=ldres, ldaux=ldaux, misaligned=G.case_misaligned(case, epi))
            plan = ops.gemm_f32_plan(M, N, K, workspace=True, **kw)
            want = dict(kernel=case["kernel"], akf=not case["ta"], bkf=case["tb"], S=case["S"], kchunk=case["kchunk"])
            assert {k: plan[k] for k in want} == want, (G.case_id(case), epi, plan)
            if case["kernel"] == "x3":
                assert plan["vec"] == G.case_vec(case, epi), (G.case_id(case), epi, plan)
            if case["S"] > 1:  # no workspace: unsplit (the shapes that split on 64 x 64 tiles have too few of them to run unsplit there)
                plan = ops.gemm_f32_plan(M, N, K, workspace=False, **kw)
                unsplit = "mfma_t1" if case["kernel"] == "mfma_t2" else case["kernel"]
                assert plan["kernel"] == unsplit and plan["S"] == 1 and plan["kchunk"] == 0, plan
                assert ops.gemm_f32_workspace_bytes(M, N, K, case["ta"], case["tb"]) >= case["S"] * M * N * 4
                for gelu in (G.EPI_BIAS_GELU, G.EPI_DGELU):  # the fold has no GELU: those epilogues never split
                    assert ops.gemm_f32_plan(M, N, K, **dict(kw, epilogue=gelu))["S"] == 1
    finally:
        _with_arith(prev)


def test_plan_follows_the_arithmetic_switch(ops):
    """the same eligible call is the bf16x3 kernel under "bf16x3" and gemm_f32_kernel under "f32" """
    prev = _with_arith("bf16x3")
    try:
        assert ops.gemm_f32_plan(128, 128, 64)["kernel"] == "x3"
        _with_arith("f32")
        assert ops.gemm_f32_plan(128, 128, 64)["kernel"] == "mfma_t1"
        for mis in ("a", "b"):  # an unaligned k-fast operand
            _with_arith("bf16x3")
            assert ops.gemm_f32_plan(128, 128, 64, misaligned=(mis,))["kernel"] == "mfma_t1"
    finally:
        _with_arith(prev)


def test_group_plans(ops):
    prev = _with_arith("bf16x3")
    try:
        for shapes, K, _, S, kchunk in G.GROUP_CASES:
            plan = ops.gemm_f32_tn_group_plan(shapes, K)
            tiles = sum(-(-m // 128) * -(-n // 128) for m, n in shapes)
            assert plan["ok"] and plan["tiles"] == tiles and plan["S"] == S and plan["kchunk"] == kchunk, (shapes, K, plan)
            assert plan["workspace_bytes"] == 4 * S * sum(m * n for m, n in shapes), plan
        for shapes, K, why in G.GROUP_INELIGIBLE:
            plan = ops.gemm_f32_tn_group_plan(shapes, K)
            assert not plan["ok"] and plan["tiles"] == plan["S"] == plan["workspace_bytes"] == 0, (why, plan)
        _with_arith("f32")  # the grouped launch is the bf16x3 arithmetic's
        assert not ops.gemm_f32_tn_group_plan(G.GROUP_CASES[0][0], 512)["ok"]
    finally:
        _with_arith(prev)


def test_a_layer_configuration_carries_its_own_arithmetic(ops):
    """avf_layer_cfg ends in f32_arith and the binding agrees on its size; what a layer call is told about its arithmetic comes
    from that field alone, so the host-side queries answer the same under both settings of the process-wide default - which
    stays the default of the operator-level plan queries, as before.  The buffers of a layer serve either arithmetic."""
    import ctypes as C
    L = A._lib
    lib = L.load()
    assert C.sizeof(L.LayerCfg) == lib.avf_sizeof_layer_cfg()
    assert L.LayerCfg._fields_[-1][0] == "f32_arith"
    mk = lambda dt, arith, N=64, D=128, H=2, dh=64, M=256: L.LayerCfg(8, N, D, H, dh, M, dt, 1, 1e-5, 0.0, 0, 0, 0, None, 0, 0, 0, 0, 0,
                                                                      None, arith)
    sizes = lambda cfg: tuple(f(C.byref(cfg)) for f in (lib.avf_layer_saved_bytes, lib.avf_layer_workspace_bytes, lib.avf_layer_lowp_bytes))
    small = dict(N=16, D=256, H=8, dh=32)  # the short-sequence layer: fused kernels on bf16 (7), none on fp32 (0)
    prev = L.get_f32_arithmetic()
    try:
        answers = set()
        for setting in ("bf16x3", "f32"):
            _with_arith(setting)
            for arith in (0, 1):
                assert A.ops.layer_small_path(mk(L.BF16, arith, **small)) == 7
                assert A.ops.layer_small_path(mk(L.F32, arith, **small)) == 0
                assert A.ops.layer_small_path(mk(L.F32, arith)) == 0
                answers.add((sizes(mk(L.F32, arith)), sizes(mk(L.BF16, arith))))
            assert sizes(mk(L.F32, 2)) == (0, 0, 0) and sizes(mk(L.F32, -1)) == (0, 0, 0)  # neither 0 nor 1: refused
            assert A.ops.layer_small_path(mk(L.BF16, 2, **small)) == 0
            assert "f32_arith" in lib.avf_last_error().decode()
            # the operator-level queries read the default
            x3 = setting == "bf16x3"
            assert ops.gemm_f32_plan(128, 128, 64)["kernel"] == ("x3" if x3 else "mfma_t1")
            assert bool(ops.gemm_f32_tn_group_plan(G.GROUP_CASES[0][0], 512)["ok"]) == x3
            assert lib.avf_attn_parity_plan(L.F32, 64, 0, 0, 1, 2) == (2 if x3 else 1)
            assert L.get_f32_arithmetic() == setting  # (no query moves it)
        assert len(answers) == 1, answers  # one set of sizes, whatever the field and the default say
        f32_sizes, bf16_sizes = answers.pop()
        assert min(f32_sizes[:2]) > 0 and min(bf16_sizes) > 0, (f32_sizes, bf16_sizes)  # (and they are sizes, not refusals)
        with pytest.raises(ValueError, match="bf16x3"):
            L.set_f32_arithmetic("fp32")
    finally:
        _with_arith(prev)
