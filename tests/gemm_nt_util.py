"""fp64 reference, element-wise bounds and mutants for the tiled bf16 NT GEMM family (csrc/gemm_bf16.hip: gemm_bf16_nt_kernel,
gemm_bf16_nt_glds_kernel; csrc/gemm_nt.hpp: nt_epilogue, nt_epilogue_lean_body).  CPU only: tests/test_gpu_gemm_nt.py
feeds it what the device returned, tests/test_gemm_nt_ref_cpu.py shows without a device that the bounds bite.

The operation (f = the dropout factors keep / (1 - p) of the site, element index m * N + n; f = 1 without dropout):
    P = A W^T, magP = |A| |W|^T, u = P + bias                    (bf16 operands are exact in fp64)
    NONE       C = u
    BIAS_RES   C = u * f + res
    BIAS_GELU  aux = u (unmasked), C = gelu_tanh(u) * f
    DGELU      C = P * f * gelu_tanh'(aux)                        (aux given, no bias)
    column sums = sum over the rows m < M of C, from the values before their rounding to C's type

Bounds, with U = 2^-24 (half an fp32 ulp, relative).  Every one is a bound on |device - reference| per ELEMENT.
  accumulation   eP = 2 * K * U * magP.  A product of two bf16 values is exact in fp32 (8 + 8 significand bits); K * U * magP is
                 the worst case of an fp32 summation of K terms in any order; the factor 2 covers the rounding inside the
                 MFMA's 32-term sum, which is not documented.
  epilogue       every fp32 add or multiply: U * (|its exact result| + the bound carried into it), and the carried bound
                 itself scaled by the other factor.  (An fma the compiler forms rounds once where this counts twice.)
  activation     ACT * U * (1 + |u|) absolute, for gelu_tanh_fast(u) and for dgelu_tanh_fast(u), ACT = 16: v_exp_f32 and
                 v_rcp_f32 are about 1 ulp each and the argument error of exp2 is damped by s (1 - s), roughly
                 5 * U * |u|; 16 leaves a margin of 3.  In DGELU it is scaled by |P * f|.  The error u itself carries into
                 the activation is bounded with |gelu'| <= 1.13.
                 Measured on an MI355X (tests/test_gpu_gemm_nt.py, GEMMSTAT lines, fp32 C): BIAS_GELU uses at most 0.12
                 and DGELU at most 0.30 of their whole bound, so ACT = 16 stands as stated.
  bf16 C / aux   b + 2^-9 * pow2ceil(|ref| + b) for one round-to-nearest-even of a value within b of ref, pow2ceil(x) = the
                 power of two above x: exactly half a bf16 ulp of the largest value that can be rounded.  (2^-9 * (|ref| + b)
                 itself is not a bound a correct rounding meets: bf16 keeps 8 significand bits, so 1 + 2^-8 rounds to 1 with a
                 relative error of 2^-8 (1 - 2^-8); test_gemm_nt_ref_cpu.py::test_bf16_bound_is_half_an_ulp shows both.  Half
                 an ulp lies between 2^-9 and 2^-8 of the value and is the tightest bound that holds.)
  column sums    sum_m of the per-element fp32 bound + M * U * sum_m |C| (an fp32 sum of M terms in any order).

Data families (make_inputs): "normal" randn; "wide" magnitudes spread over six decades inside every row of A; "cancel" rows
whose product nearly cancels (|P| << magP).  W is scaled so that u covers about [-10, 10].  The aux given to DGELU also
holds +-0, +-8, +-20 and +-1e4: the saturated ends of exp2, where the result must be 0 or 1 times the product, never NaN."""
import math

import torch

EPI_NONE, EPI_BIAS_RES, EPI_BIAS_GELU, EPI_DGELU = 0, 1, 2, 3
EPI_NAMES = {EPI_NONE: "none", EPI_BIAS_RES: "bias_res", EPI_BIAS_GELU: "bias_gelu", EPI_DGELU: "dgelu"}
FAMILIES = ("normal", "wide", "cancel")
U = 2.0 ** -24
U_BF16 = 2.0 ** -9
ACT = 16.0
DGELU_MAX = 1.13  # max |gelu_tanh'| (1.129 at u = 1.41 ...)
SPECIAL_AUX = (0.0, -0.0, 8.0, -8.0, 20.0, -20.0, 1e4, -1e4)
_C = math.sqrt(2.0 / math.pi)
_A = 0.044715


def gelu_tanh(u):
    return 0.5 * u * (1.0 + torch.tanh(_C * (u + _A * u ** 3)))


def dgelu_tanh(u):
    t = torch.tanh(_C * (u + _A * u ** 3))
    return 0.5 * (1.0 + t) + 0.5 * u * (1.0 - t * t) * _C * (1.0 + 3.0 * _A * u * u)


def make_operands(M, N, K, seed, family):
    """bf16 A [M, K] and W [N, K] of a data family: the same for every epilogue of a (shape, family, seed)"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    if family == "wide":
        a = a * torch.pow(10.0, torch.rand(M, K, generator=g) * 6 - 3)
    elif family == "cancel":  # the second half of K undoes the first up to 2^-6: |P| ~ 2^-6 magP / sqrt(K)
        h = K // 2
        a[:, h:2 * h] = -a[:, :h]
        w[:, h:2 * h] = w[:, :h] * (1.0 + 2.0 ** -6 * torch.randn(N, h, generator=g))
    a = a.bfloat16()
    p = a.double() @ w.bfloat16().double().t()
    w = (w * (3.3 / float(p.std()))).bfloat16()  # u = P + bias: P within about +-10 at three sigma
    return a, w


def make_inputs(M, N, K, seed, family, c_dtype, epilogue, operands=None):
    """bf16 A [M, K], W [N, K] (make_operands, or the given pair); fp32 bias [N] (None for DGELU); res (BIAS_RES) /
    aux_in (DGELU) [M, N] in c_dtype."""
    a, w = operands if operands is not None else make_operands(M, N, K, seed, family)
    g = torch.Generator().manual_seed(seed * 8 + epilogue + 1)
    bias = None if epilogue == EPI_DGELU else (torch.rand(N, generator=g) * 6 - 3)
    inp = dict(M=M, N=N, K=K, family=family, epilogue=epilogue, c_dtype=c_dtype, a=a, w=w, bias=bias, res=None, aux_in=None)
    if epilogue == EPI_BIAS_RES:
        inp["res"] = (torch.randn(M, N, generator=g) * 3).to(c_dtype)
    if epilogue == EPI_DGELU:
        x = torch.rand(M, N, generator=g) * 20 - 10
        flat = x.view(-1)
        for i, v in enumerate(SPECIAL_AUX):  # 488 elements apart, so that every lane position and row block meets them
            flat[i * 7::61 * len(SPECIAL_AUX)] = v
        inp["aux_in"] = x.to(c_dtype)
    return inp


def products(inp):
    """P and magP in fp64: computed once per (shape, data) and shared by every epilogue"""
    a, w = inp["a"].double(), inp["w"].double()
    return a @ w.t(), a.abs() @ w.abs().t()


def reference(inp, f=None, prod=None, bias=None, res=None, aux_in=None, eP=None):
    """fp64 reference and per-element fp32 bounds.  f: dropout factors [M, N] or None.  bias / res / aux_in override
    the ones of inp (one (shape, data) serves every epilogue).  eP: the accumulation bound (a number or [M, N]) in place of
    2 K U magP, for a kernel family with another accumulator (tests/gemm_mx8_util.py).
    -> dict(C, bC, aux, baux, cs, bcs, premask)."""
    epi, M, K = inp["epilogue"], inp["M"], inp["K"]
    P, magP = prod if prod is not None else products(inp)
    bias = inp["bias"] if bias is None else bias
    res = inp["res"] if res is None else res
    aux_in = inp["aux_in"] if aux_in is None else aux_in
    f = torch.ones_like(P) if f is None else f.double()
    eP = 2.0 * K * U * magP if eP is None else torch.zeros_like(P) + eP
    b = torch.zeros(P.shape[1], dtype=torch.float64) if bias is None else bias.double()
    u = P + b
    eu = eP + U * (u.abs() + eP)
    out = dict(aux=None, baux=None)
    if epi == EPI_NONE:
        C, bC, pre = u, eu, u
    elif epi == EPI_BIAS_RES:
        t = u * f
        et = eu * f.abs() + U * (t.abs() + eu * f.abs())
        C = t + res.double()
        bC = et + U * (C.abs() + et)
        pre = u
    elif epi == EPI_BIAS_GELU:
        out["aux"], out["baux"] = u, eu
        pre = gelu_tanh(u)
        eg = DGELU_MAX * eu + ACT * U * (1.0 + u.abs())
        C = pre * f
        bC = eg * f.abs() + U * (C.abs() + eg * f.abs())
    else:
        x = aux_in.double()
        d = dgelu_tanh(x)
        ed = ACT * U * (1.0 + x.abs())
        m = f * d
        em = f.abs() * ed + U * (m.abs() + f.abs() * ed)
        pre = u * d
        C = u * m
        bC = eu * (m.abs() + em) + u.abs() * em + U * C.abs()
    out.update(C=C, bC=bC, premask=pre, f=f)
    out["cs"] = C.sum(0)
    out["bcs"] = bC.sum(0) + M * U * C.abs().sum(0)
    return out


def bf16_bound(ref, b):
    """b + half a bf16 ulp of |ref| + b (= 2^-9 times the power of two above it)"""
    _, e = torch.frexp(ref.abs() + b)  # x = m 2^e, 0.5 <= m < 1
    return b + U_BF16 * torch.pow(2.0, e.double())


def round_to(x, dtype, truncate=False):
    """fp64 -> the storage type, as a correct kernel would store it (fp32 first, then round-to-nearest-even to bf16)"""
    x = x.float()
    if dtype == torch.float32:
        return x
    if truncate:
        return (x.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    return x.bfloat16()


def _ratio(got, ref, bound):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max())


def mask_not_vacuous(ref):
    """with dropout: at least 10 % of the masked and 10 % of the kept elements are non-zero before the mask"""
    f, pre = ref["f"], ref["premask"]
    masked, kept = f == 0, f != 0
    assert int(masked.sum()) > 0 and int(kept.sum()) > 0, "the mask drops nothing or everything"
    nz_m = float((pre[masked] != 0).double().mean())
    nz_k = float((pre[kept] != 0).double().mean())
    assert nz_m >= 0.1 and nz_k >= 0.1, (nz_m, nz_k)
    return dict(masked_nonzero=round(nz_m, 3), kept_nonzero=round(nz_k, 3), dropped=round(float(masked.double().mean()), 3))


def check_outputs(what, ref, c, aux=None, cs=None):
    """assert every given output element-wise within its bound; -> the worst error / bound ratio per output"""
    stats = {}
    bC = ref["bC"] if c.dtype == torch.float32 else bf16_bound(ref["C"], ref["bC"])
    stats["C"] = _ratio(c, ref["C"], bC)
    if ref["aux"] is not None:
        assert aux is not None, what + ": BIAS_GELU must write aux"
        ba = ref["baux"] if aux.dtype == torch.float32 else bf16_bound(ref["aux"], ref["baux"])
        stats["aux"] = _ratio(aux, ref["aux"], ba)
    if cs is not None:
        stats["colsum"] = _ratio(cs, ref["cs"], ref["bcs"])
    bad = {k: v for k, v in stats.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1: {bad} (all: {stats})"
    return {k: round(v, 4) for k, v in stats.items()}


# ------------------------------------------------------------------------------------------------
# Mutants: what a subtly wrong kernel would return.  simulate() computes the reference's own arithmetic with one of them
# applied and rounds to C's type; check_outputs must pass the unmutated result and refuse every mutant.
# name -> (epilogue it applies to or None for all, needs dropout, needs column sums, bf16 C only)
MUTANTS = {
    "k_tail_dropped": (None, False, False, False),      # the last 64 of K dropped for one 128-row tile
    "ragged_tile_copied": (None, False, False, False),  # the last ragged row tile copied from the previous tile
    "bias_shifted": (EPI_BIAS_GELU, False, False, False),  # bias shifted by 4 columns
    "lane_pair_swapped": (None, False, False, False),   # columns 4..7 and 16..19 of one 32-column block pair swapped
    "bf16_truncated": (None, False, False, True),       # bf16 by truncation instead of round-to-nearest
    "residual_masked": (EPI_BIAS_RES, True, False, False),  # the residual masked along with the product
    "aux_masked": (EPI_BIAS_GELU, True, False, False),  # GELU's saved aux masked
    "mask_index_ldc": (None, True, False, False),       # the mask indexed with m * ldc + n instead of m * N + n
    "colsum_dup_row": (None, False, True, False),       # column sums that include a duplicated clamped row M - 1
    "colsum_unmasked": (None, True, True, False),       # column sums of unmasked values
    "colsum_partial_lost": (None, False, True, False),  # one partial row of a wave row left out of the column sums
}


def make_factors(M, N, ldc, p, seed):
    """CPU stand-in for ops.dropout_factors: factors over a flat index space, as (f indexed m * N + n, f indexed m * ldc + n)"""
    g = torch.Generator().manual_seed(seed)
    flat = (torch.rand(M * ldc, generator=g) >= p).double() / (1.0 - p)
    return flat[:M * N].view(M, N).clone(), flat.view(M, ldc)[:, :N].clone()


def simulate(inp, f=None, f_ldc=None, mutant=None):
    """-> (C, aux or None, column sums) as the (mutated) kernel would return them, in inp's C type"""
    epi, M, N, K, cdt = inp["epilogue"], inp["M"], inp["N"], inp["K"], inp["c_dtype"]
    P, magP = products(inp)
    bias = inp["bias"]
    if mutant == "k_tail_dropped":
        r0 = 128 if M > 128 else 0
        a, w = inp["a"].double(), inp["w"].double()
        P = P.clone()
        P[r0:r0 + 128] = a[r0:r0 + 128, :K - 64] @ w[:, :K - 64].t()
    if mutant == "bias_shifted":
        bias = torch.roll(bias, 4)
    fm = f_ldc if mutant == "mask_index_ldc" else f
    ref = reference(inp, fm, (P, magP), bias=bias)
    C, aux = ref["C"].clone(), (None if ref["aux"] is None else ref["aux"].clone())
    fd = torch.ones_like(C) if fm is None else fm.double()
    if mutant == "residual_masked":
        C = (ref["premask"] + inp["res"].double()) * fd
    if mutant == "aux_masked":
        aux = aux * fd
    cs_src = C
    if mutant == "colsum_unmasked":
        cs_src = reference(inp, None, (P, magP), bias=bias)["C"]
    cs = cs_src.sum(0)
    if mutant == "colsum_dup_row":
        cs = cs + cs_src[M - 1]
    if mutant == "colsum_partial_lost":
        cs = cs - cs_src[48:96].sum(0)
    if mutant == "ragged_tile_copied":
        r0 = (M - 1) // 128 * 128
        assert r0 >= 128 and M % 128 != 0
        C[r0:M] = C[r0 - 128:M - 128]
    if mutant == "lane_pair_swapped":
        c0 = 32 if N >= 64 else 0
        blk = C[16:32, c0:c0 + 32].clone()
        C[16:32, c0 + 4:c0 + 8], C[16:32, c0 + 16:c0 + 20] = blk[:, 16:20], blk[:, 4:8]
    trunc = mutant == "bf16_truncated"
    return round_to(C, cdt, trunc), (None if aux is None else round_to(aux, cdt, trunc)), cs.float()


# ------------------------------------------------------------------------------------------------
# The tile table (kNtTiles of csrc/gemm_nt.hpp) and the shapes whose UNFORCED plan is each of its entries: every entry must
# be some shape's own pick, or it is a kernel family no input reaches (tests/test_gemm_nt_ref_cpu.py, test_gemm_mx8_ref_cpu.py).
# (M, N) -> the tile pick_nt_tile plans at any K; the first row is the bf16 kernel's small-M tile 6 at K = 128 and tile 5 of
# the MX-FP8 kernel at K = 384 (which has no tile 6: two LDS stages).
PLAN_SHAPES = {(300, 264): None, (4096, 512): 5, (8192, 1024): 2, (10368, 768): 1}
_TABLE_CHILD = r"""
import avformer_amd as A
M, N = 8192, 1024
print("HELD", A.ops.gemm_nt_plan(M, N, 512)["tile"], A.ops.gemm_mx8_plan(M, N, 512)["tile"])
"""
_held = {}


def tile_ids_held(repo, ids=range(8)):
    """-> {"bf16": ids, "mx8": ids}: the tile ids the two kernels' tables hold, asked of the launcher's own plan with the id
    forced (AVF_TUNING=1 AVF_NT_TILE=id, read once per process: one child per id, side by side; host code, no device).  An id a
    table does not hold plans as tile 2."""
    import os
    import subprocess
    import sys
    if not _held:
        procs = {}
        for i in ids:
            env = dict(os.environ, AVF_TUNING="1", AVF_NT_TILE=str(i))
            procs[i] = subprocess.Popen([sys.executable, "-c", _TABLE_CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                        text=True, env=env, cwd=repo)
        held = {"bf16": set(), "mx8": set()}
        for i, pr in procs.items():
            out, err = pr.communicate(timeout=300)
            assert pr.returncode == 0, err[-2000:]
            bf, mx = [int(x) for x in [l for l in out.splitlines() if l.startswith("HELD ")][-1].split()[1:]]
            assert bf in (i, 2) and mx in (i, 2), (i, bf, mx)
            if bf == i:
                held["bf16"].add(i)
            if mx == i:
                held["mx8"].add(i)
        _held.update(held)
    return _held
