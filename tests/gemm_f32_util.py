"""fp64 reference, element-wise bounds, data families, case table and mutants for the parity-mode fp32 GEMM family
(csrc/gemm_f32.hip: gemm_f32_kernel<T = 1 | 2> and its split form, gemm_f32_fold_kernel, gemm_f32x3_kernel in four
orientations, gemm_f32x3_group_kernel + gemm_f32x3_group_fold_kernel).  CPU only: tests/test_gpu_gemm_f32.py feeds it what the
device returned, tests/test_gemm_f32_ref_cpu.py shows without a device that the bounds bite and that the plan query names the
kernel each case expects.

The operation is the one stated at the top of tests/gemm_nt_util.py, with fp32 operands, fp32 C / residual / aux and any of
the four orientations (here always written on the logical A [M, K] and W [N, K]: P = A W^T); the epilogue reference, its error
propagation, ACT, DGELU_MAX, SPECIAL_AUX, gelu_tanh and dgelu_tanh are imported from that module, not copied.  The bias, where
one is given, is added by every epilogue but DGELU.

Bounds, per ELEMENT, U = 2^-24.  All derived, none tuned; only the accumulation term differs from gemm_nt_util:
  f32 arithmetic (gemm_f32_kernel)     |dev - P| <= (K + S) U magP, magP = |A| |W|^T in fp64: the worst case of the k-ordered
                                       fmaf chain the kernel's header claims (one rounding per product) plus the S - 1 additions
                                       of the fold.  Measured on an MI355X: at most 0.88 of the whole bound (1000 x 1030 x 20,
                                       "wide"), so (K + S) stands as stated; and the claim holds to the letter - fmaf_chain()
                                       restates it and the device returns its bits (NONE / BIAS_RES, split or not).
  bf16x3 against the exact product    (oracle.bf16x3.PER_PRODUCT_BOUND + 2 K U) magP: the contract of the arithmetic (3 * 2^-16
                                       per product) plus an fp32 sum in any order, doubled for the undocumented rounding inside
                                       an MFMA as in gemm_nt_util.
  bf16x3 against its own emulation     6 K U mag3 against oracle.bf16x3.matmul (fp64 sum of the three kept products), mag3 =
                                       |hi_a||hi_b| + |hi_a||lo_b| + |lo_a||hi_b|: an fp32 sum of 3 K exact terms in any
                                       order, doubled.  The bound that catches a lost cross term; loose by construction (it
                                       grows with K while the cross terms do not), so it is asserted where K <= EMU_K_MAX = 160.
  epilogue, activation                 gemm_nt_util's, for gelu_tanh_fast (bf16x3 kernel) and tanhf (gemm_f32_kernel) alike.

Data families: "normal", "wide" (magnitudes over eight decades inside every row of A) and "cancel" as in gemm_nt_util but
fp32, not rounded to bf16; and "exact", which needs no tolerance: every element is h + m 2^-12 with h in +-{1, 2, 3} and m an
integer in [-7, 7], bias / residual small integers, dropout at p = 0.5 (keep factor exactly 2).  Then hi = h and lo = m 2^-12
exactly, every partial sum of hi_a hi_b + hi_a lo_b + lo_a hi_b is a multiple of 2^-12 far below 2^12, and a correct bf16x3
kernel equals oracle.bf16x3.matmul BIT FOR BIT whatever its order, split count or fold; that result differs from the exact
product by the lo_a lo_b the kernel must not compute.  With m = 0 in W (exact_operands(..., w_lo=False)) every a b and every
partial sum is exact in fp32 too and both arithmetics equal the fp64 product bit for bit: the form the gemm_f32_kernel cases
take.  (|m| <= 7: with 15, values just below a power of two round to the next-lower bf16 and hi is no longer h.)"""
import itertools
import math

import torch

import gemm_nt_util as NT
from gemm_nt_util import (ACT, DGELU_MAX, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_DGELU, EPI_NAMES, EPI_NONE, SPECIAL_AUX, U,  # noqa: F401
                          dgelu_tanh, gelu_tanh)
from oracle import bf16x3 as X3

EPIS = (EPI_NONE, EPI_BIAS_RES, EPI_BIAS_GELU, EPI_DGELU)
BOUNDED = ("normal", "wide", "cancel")
FAMILIES = BOUNDED + ("exact",)
EMU_K_MAX = 160
P_DROP, P_DROP_EXACT = 0.2, 0.5
ORIENT = {"NT": (False, True), "NN": (False, False), "TN": (True, False), "TT": (True, True)}  # name -> (trans_a, trans_b)


def f32_acc_factor(K, S):
    """(K + S) U: a k-ordered fmaf chain of K products and the S - 1 fold additions"""
    return (K + S) * U


def x3_exact_factor(K):
    return X3.PER_PRODUCT_BOUND + 2.0 * K * U


def x3_emu_factor(K):
    return 6.0 * K * U


# ------------------------------------------------------------------------------------------------
# data
def exact_operands(M, N, K, seed, w_lo=True):
    g = torch.Generator().manual_seed(seed)

    def draw(rows, lo):
        h = torch.randint(1, 4, (rows, K), generator=g).float() * (torch.randint(0, 2, (rows, K), generator=g).float() * 2 - 1)
        m = torch.randint(-7, 8, (rows, K), generator=g).float()
        return h + m * 2.0 ** -12 if lo else h
    return draw(M, True), draw(N, w_lo)


def make_operands(M, N, K, seed, family, w_lo=True):
    """fp32 A [M, K] and W [N, K] of a data family: the same for every epilogue of a (shape, family, seed)"""
    assert family in FAMILIES
    if family == "exact":
        return exact_operands(M, N, K, seed, w_lo)
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    if family == "wide":
        a = a * torch.pow(10.0, torch.rand(M, K, generator=g) * 8 - 4)
    elif family == "cancel" and K >= 2:  # the second half of K undoes the first up to 2^-6
        h = K // 2
        a[:, h:2 * h] = -a[:, :h]
        w[:, h:2 * h] = w[:, :h] * (1.0 + 2.0 ** -6 * torch.randn(N, h, generator=g))
    p = a.double() @ w.double().t()
    w = (w * (3.3 / float(p.std()))).float()  # u = P + bias: P within about +-10 at three sigma
    return a, w


def make_inputs(M, N, K, seed, family, epilogue, operands, S=1, kchunk=0, res_row=False, bias=True):
    """operands (A, W) of make_operands; fp32 bias [N] (None for DGELU or bias=False); res (BIAS_RES) [M, N], or [N] with
    res_row (the broadcast positional row, ldres = 0); aux_in (DGELU) [M, N].  S / kchunk: the split the plan reports."""
    a, w = operands
    if family == "exact":
        g = torch.Generator().manual_seed(seed * 8 + epilogue + 1)
        inp = dict(M=M, N=N, K=K, family=family, epilogue=epilogue, c_dtype=torch.float32, a=a, w=w, res=None, aux_in=None,
                   bias=None if epilogue == EPI_DGELU else torch.randint(-3, 4, (N,), generator=g).float())
        if epilogue == EPI_BIAS_RES:
            inp["res"] = torch.randint(-8, 9, (M, N), generator=g).float()
        assert epilogue in (EPI_NONE, EPI_BIAS_RES), "the GELU epilogues use the bounded families"
    else:
        inp = NT.make_inputs(M, N, K, seed, family, torch.float32, epilogue, operands=(a, w))
    if not bias:
        inp["bias"] = None
    if res_row and inp["res"] is not None:
        inp["res"] = inp["res"][M // 2].clone()
    inp.update(S=S, kchunk=kchunk)
    return inp


def products(a, w):
    """everything fp64 a (shape, data) needs, once: P, magP, the bf16x3 emulation and its magnitude"""
    ad, wd = a.double(), w.double()
    ah, al = (t.double() for t in X3.split(a))
    bh, bl = (t.double() for t in X3.split(w))
    return dict(P=ad @ wd.t(), magP=ad.abs() @ wd.abs().t(), emu=X3.matmul(a, w.t()),
                mag3=ah.abs() @ bh.abs().t() + ah.abs() @ bl.abs().t() + al.abs() @ bh.abs().t())


def reference(inp, kind, f, prod):
    """gemm_nt_util.reference with this family's accumulation bound.  kind: "f32" (against P), "x3_exact" (against P),
    "x3_emu" (against the emulation).  That function takes its accumulation bound as 2 K U magP from inp["K"], which it uses
    for nothing else: it is handed the K that makes 2 K U the factor wanted here."""
    K = inp["K"]
    if kind == "f32":
        P, mag, factor = prod["P"], prod["magP"], f32_acc_factor(K, inp["S"])
    elif kind == "x3_exact":
        P, mag, factor = prod["P"], prod["magP"], x3_exact_factor(K)
    else:
        assert kind == "x3_emu"
        P, mag, factor = prod["emu"], prod["mag3"], x3_emu_factor(K)
    return NT.reference(dict(inp, K=factor / (2.0 * U)), f, (P, mag))


class BitsDiffer(AssertionError):
    pass


def chain_rows(M):
    """up to 128 rows spread over M: the rows the fmaf-chain comparison looks at (every tile row of the shapes in the table)"""
    return torch.arange(0, M, max(1, M // 128))[:128]


def fmaf_chain(inp, rows):
    """What gemm_f32_kernel returns for NONE / BIAS_RES without dropout if its header's claim holds to the letter, as fp32
    [len(rows), N]: per split a chain acc = fma(a_k, b_k, acc) from zero in the order of k (one rounding per step: a b is exact
    in fp64, and the sum is rounded to fp64 and then to fp32, which differs from the single rounding of an fma only when the
    fp64 sum lands exactly on an fp32 tie), the splits added in order, then bias and residual, each one fp32 addition."""
    assert inp["epilogue"] in (EPI_NONE, EPI_BIAS_RES)
    a, w, K, S = inp["a"][rows].double(), inp["w"].double(), inp["K"], inp["S"]
    kchunk = inp["kchunk"] if S > 1 else K
    total = None
    for z in range(S):
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float64)
        for k in range(z * kchunk, min(K, (z + 1) * kchunk)):
            acc = (acc + a[:, k, None] * w[None, :, k]).float().double()
        total = acc.float() if total is None else total + acc.float()
    if inp["bias"] is not None:
        total = total + inp["bias"]
    if inp["epilogue"] == EPI_BIAS_RES:
        total = total + (inp["res"] if inp["res"].dim() == 1 else inp["res"][rows])
    return total


def check_case(what, inp, kernel, f, prod, c, aux=None):
    """assert what a call returned against everything that binds it; -> the worst error / bound ratio per output.
    kernel: "x3" or "mfma" (which arithmetic ran: the plan's answer, not the mode asked for)."""
    assert c.dtype == torch.float32 and (aux is None or aux.dtype == torch.float32)
    if inp["family"] == "exact":
        ref = reference(inp, "x3_emu" if kernel == "x3" else "f32", f, prod)
        want = ref["C"].float()
        assert torch.equal(want.double(), ref["C"]), what + ": the exact family's reference is not representable in fp32"
        bad = int((c != want).sum())
        if bad or not bool(torch.isfinite(c).all()):
            raise BitsDiffer(f"{what}: {bad} of {c.numel()} elements differ from the exact result (bit-exact family), "
                             f"max |diff| {float((c.double() - ref['C']).abs().max()):.3e}")
        return {"C": 0.0}
    if kernel != "x3":
        return NT.check_outputs(what, reference(inp, "f32", f, prod), c, aux)
    stats = NT.check_outputs(what + " (exact product)", reference(inp, "x3_exact", f, prod), c, aux)
    if inp["K"] <= EMU_K_MAX:
        emu = NT.check_outputs(what + " (emulation)", reference(inp, "x3_emu", f, prod), c, aux)
        stats.update({k + "_emu": v for k, v in emu.items()})
    return stats


# ------------------------------------------------------------------------------------------------
# the GPU case table: tests/test_gpu_gemm_f32.py runs it, tests/test_gemm_f32_ref_cpu.py asks the plan query about every entry
def _case(name, arith, orient, M, N, K, kernel, S=1, kchunk=0, vec=None, epis=EPIS, ws=True, **layout):
    """kernel / S / kchunk / vec: what gemm_f32 must decide (vec is None for gemm_f32_kernel, or where it depends on the
    epilogue: `novec_epis`).  layout: how the test lays the operands out -
      a = "pad8" (lda = row + 8) | "pad9" (lda % 4 != 0) | "off1" (A one float past a 16-byte boundary)
      c_pad = 8 | 9 (odd ldc);  bias_off = 0 | 1 (floats past a 16-byte boundary);  res = "pad8" | "pad9" | "row" (ldres = 0);
      aux_pad = 8 | 9.   novec_epis: the epilogues whose operands lose the 16-byte accesses through that layout."""
    ta, tb = ORIENT[orient]
    lay = dict(a="pad8", c_pad=8, bias_off=0, res="pad8", aux_pad=8, novec_epis=None)
    assert set(layout) <= set(lay), layout
    lay.update(layout)
    return dict(name=name, arith=arith, orient=orient, ta=ta, tb=tb, M=M, N=N, K=K, kernel=kernel, S=S, kchunk=kchunk, vec=vec,
                epis=tuple(epis), ws=ws, **lay)


def case_id(c):
    return f"{c['name']}-{c['orient']}-{c['M']}x{c['N']}x{c['K']}"


X3_MN = ((96, 96), (128, 128), (129, 130), (257, 132))  # the eligibility edge; one full tile; N % 4 != 0; a one-row last tile
X3_K = (32, 64, 96, 128, 160)                           # one to five K-steps: every branch of the two-step look-ahead


def _x3_unsplit():
    out = []
    for i, (orient, K) in enumerate(itertools.product(ORIENT, X3_K)):
        M, N = X3_MN[i % 4]
        out.append(_case("x3", "bf16x3", orient, M, N, K, "x3", vec=N % 4 == 0))
    for K, (M, N) in ((40, X3_MN[2]), (100, X3_MN[3])):  # KTAIL inside the first and inside the fourth K-step
        out.append(_case("x3_ktail", "bf16x3", "TN", M, N, K, "x3", vec=N % 4 == 0))
    # vec switched off by ONE operand each (N % 4 == 0 everywhere here)
    out.append(_case("x3_odd_ldc", "bf16x3", "NT", 128, 128, 64, "x3", vec=False, c_pad=9))
    out.append(_case("x3_bias_off1", "bf16x3", "NN", 129, 132, 96, "x3", novec_epis=(EPI_NONE, EPI_BIAS_RES, EPI_BIAS_GELU), bias_off=1))
    out.append(_case("x3_odd_ldres", "bf16x3", "TN", 257, 132, 64, "x3", novec_epis=(EPI_BIAS_RES,), res="pad9"))
    out.append(_case("x3_odd_ldaux", "bf16x3", "TT", 96, 96, 128, "x3", novec_epis=(EPI_BIAS_GELU, EPI_DGELU), aux_pad=9))
    out.append(_case("x3_res_row", "bf16x3", "NT", 129, 132, 96, "x3", vec=True, epis=(EPI_BIAS_RES,), res="row"))
    return out


def _x3_split():
    """tiles < 256 and K >= 512: S = min(512 / tiles, K / 256), kchunk = ceil(ceil(K / S) / 32) * 32.  Only NONE and BIAS_RES
    split (the fold applies them); the same call without a workspace runs unsplit (the test asks both)."""
    fold = (EPI_NONE, EPI_BIAS_RES)
    out = []
    for orient in ORIENT:
        out.append(_case("x3_split", "bf16x3", orient, 257, 260, 512, "x3", S=2, kchunk=256, vec=True, epis=fold))
        out.append(_case("x3_split_novec", "bf16x3", orient, 129, 130, 512, "x3", S=2, kchunk=256, vec=False, epis=fold))
    out.append(_case("x3_split3", "bf16x3", "NN", 257, 260, 800, "x3", S=3, kchunk=288, vec=True, epis=fold))  # 288 / 288 / 224; 27 workgroups
    out.append(_case("x3_split3_ragged", "bf16x3", "TN", 257, 260, 1000, "x3", S=3, kchunk=352, vec=True, epis=fold))  # 352 / 352 / 296
    out.append(_case("x3_split_res_row", "bf16x3", "NT", 257, 260, 512, "x3", S=2, kchunk=256, vec=True, epis=(EPI_BIAS_RES,), res="row"))
    return out


def _mfma():
    out = []
    small = ((5, 12, 8), (33, 31, 7), (130, 70, 52))
    for i, (orient, (M, N, K)) in enumerate(itertools.product(ORIENT, small)):
        out.append(_case("t1", "f32", orient, M, N, K, "mfma_t1"))
    # under "bf16x3", shapes f32x3_ok turns away: K % 32 != 0 on a k-fast operand, lda % 4 != 0, an unaligned A
    out.append(_case("t1_x3_ragged_k", "bf16x3", "NT", 130, 100, 52, "mfma_t1"))
    out.append(_case("t1_x3_ragged_k", "bf16x3", "NN", 130, 100, 52, "mfma_t1"))
    out.append(_case("t1_x3_odd_lda", "bf16x3", "NT", 130, 100, 64, "mfma_t1", a="pad9"))
    out.append(_case("t1_x3_unaligned_a", "bf16x3", "NT", 130, 100, 64, "mfma_t1", a="off1"))
    # T = 2 unsplit: at least 256 tiles of 64 x 64, tiny K
    out.append(_case("t2", "f32", "NT", 1000, 1030, 8, "mfma_t2"))
    out.append(_case("t2", "f32", "TN", 1000, 1030, 20, "mfma_t2"))
    out.append(_case("t2", "bf16x3", "NN", 1025, 1000, 9, "mfma_t2"))  # (K < 32: not the bf16x3 kernel in either mode)
    # T = 1 split (f32_splits): S0 = min(ceil(256 / tiles32), K / 64, 16), kchunk = ceil(ceil(K / S0) / 32) * 32
    fold = (EPI_NONE, EPI_BIAS_RES)
    out.append(_case("t1_split", "f32", "NN", 40, 70, 300, "mfma_t1", S=4, kchunk=96, epis=fold))        # 6 tiles: 96 / 96 / 96 / 12
    out.append(_case("t1_split", "f32", "NT", 33, 12, 1000, "mfma_t1", S=11, kchunk=96, epis=(EPI_BIAS_RES,)))  # 2 tiles, S0 = 15
    # T = 2 split (f32_split64): >= 192 tiles of 32 x 32, < 512 of 64 x 64, K >= 2048: S0 = min(ceil(1024 / 56), K / 256) = 8
    out.append(_case("t2_split", "f32", "TN", 420, 450, 2080, "mfma_t2", S=8, kchunk=288, epis=(EPI_NONE,)))  # 7 x 288 + 64
    out.append(_case("t2_split", "f32", "NT", 420, 450, 2080, "mfma_t2", S=8, kchunk=288, epis=(EPI_BIAS_RES,)))
    return out


CASES = _x3_unsplit() + _x3_split() + _mfma()

GROUP_MN = ((96, 96), (128, 384), (130, 100), (257, 132))  # 1, 3, 2 and 6 tiles of 128 x 128
# (problems, K, row-strided operands?, expected S, kchunk): S = min(512 / tiles, K / 256), kchunk as above
GROUP_CASES = (
    (GROUP_MN[:2], 512, False, 2, 256),
    (GROUP_MN[1:], 1000, True, 3, 352),    # 352 / 352 / 296: a ragged last K-step inside the last split
    (GROUP_MN, 2112, False, 8, 288),       # 7 x 288 + 96
    (GROUP_MN, 512, True, 2, 256),
)
GROUP_INELIGIBLE = (  # (problems, K, why)
    ((GROUP_MN[1],), 512, "one problem"),
    ((GROUP_MN[0], (128, 130)), 512, "N % 4 != 0"),
    ((GROUP_MN[0], (95, 128)), 512, "M < 96"),
    (GROUP_MN[:2], 480, "K < 512"),
)


def case_family(i):
    """the bounded family of case i: cycled over the table, not crossed with it"""
    return BOUNDED[i % 3]


def kernel_of(case):
    return "x3" if case["kernel"] == "x3" else "mfma"


def case_vec(case, epi):
    """the vec the plan must report for this epilogue of the case (None: not the x3 kernel)"""
    if case["kernel"] != "x3":
        return None
    if case["novec_epis"] is not None:
        return epi not in case["novec_epis"]
    return case["vec"]


def case_leading_dims(case):
    """(lda, ldb, ldc, ldres, ldaux) of the layout the GPU test builds, and the names of its unaligned operands"""
    M, N, K = case["M"], case["N"], case["K"]
    arow = M if case["ta"] else K
    brow = K if case["tb"] else N
    a_pad = {"pad8": 8, "pad9": 9, "off1": 8}[case["a"]]
    lda, ldb, ldc = arow + a_pad, brow + 8, N + case["c_pad"]
    ldres = {"pad8": N + 8, "pad9": N + 9, "row": 0}[case["res"]]
    ldaux = N + case["aux_pad"]
    return lda, ldb, ldc, ldres, ldaux


def case_misaligned(case, epi):
    """operands of the GPU test's layout that are not 16-byte aligned (a view's first row starts a whole number of parent rows
    in: an odd leading dimension also moves the pointer off the boundary)"""
    lda, ldb, ldc, ldres, ldaux = case_leading_dims(case)
    mis = []
    if case["a"] in ("off1", "pad9"):
        mis.append("a")
    if ldc % 4:
        mis.append("out")
    if case["bias_off"] and epi != EPI_DGELU:
        mis.append("bias")
    if epi == EPI_BIAS_RES and ldres % 4:
        mis.append("residual")
    if epi in (EPI_BIAS_GELU, EPI_DGELU) and ldaux % 4:
        mis.append("aux")
    return mis


# ------------------------------------------------------------------------------------------------
# Mutants: what a subtly wrong kernel would return.  simulate() computes the arithmetic a correct kernel implements (the
# emulation for "x3", the exact product for "mfma") with one of them applied and rounds to fp32; check_case must pass the
# unmutated result and refuse every mutant somewhere in the case table.
# name -> (kernels it applies to, epilogue or None for all, needs dropout, needs a split, needs a ragged K-step)
MUTANTS = {
    "lo_a_hi_b_dropped": (("x3",), None, False, False, False),
    "hi_a_lo_b_dropped": (("x3",), None, False, False, False),
    "split_truncated": (("x3",), None, False, False, False),       # hi / lo by truncation instead of round-to-nearest
    "k_tail_zeroed": (("x3", "mfma"), None, False, False, True),   # the last partial K-step zeroed
    "k_row_beyond_kend": (("x3", "mfma"), None, False, True, False),  # split 0 also adds row kend, read from split 1's range
    "slab_skipped": (("x3", "mfma"), None, False, True, False),    # the last slab left out of the fold
    "slab_twice": (("x3", "mfma"), None, False, True, False),      # ... or counted twice
    "tiles_swapped": (("x3",), None, False, False, False),         # two 128 x 128 tiles swapped (a wrong xcd_contiguous)
    "lane_cols_rotated": (("x3",), None, False, False, False),     # the 4-column group of a lane rotated by one
    "mask_index_ldc": (("x3", "mfma"), None, True, False, False),  # the mask indexed with m * ldc + n
    "bias_shifted": (("x3", "mfma"), EPI_BIAS_GELU, False, False, False),  # bias shifted by one column
    "residual_row_plus1": (("x3", "mfma"), EPI_BIAS_RES, False, False, False),
    "aux_masked": (("x3", "mfma"), EPI_BIAS_GELU, True, False, False),
}
GROUP_MUTANTS = ("group_fold_offset", "group_tile_other_n")


def _split_trunc(x):
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    r = x - hi
    lo = (r.view(torch.int32) & -65536).view(torch.float32)
    return hi, lo


def _dev_product(a, w, kernel, mutant=None):
    """-> f(k0, k1): what a correct kernel of that arithmetic accumulates over the reduction rows k0 .. k1 - 1, in fp64"""
    if kernel != "x3":
        ad, wd = a.double(), w.double()
        return lambda k0, k1: ad[:, k0:k1] @ wd[:, k0:k1].t()
    ah, al = _split_trunc(a) if mutant == "split_truncated" else X3.split(a)
    bh, bl = _split_trunc(w) if mutant == "split_truncated" else X3.split(w)
    ah, al, bh, bl = (t.double() for t in (ah, al, bh, bl))

    def f(k0, k1):
        s = slice(k0, k1)
        out = ah[:, s] @ bh[:, s].t()
        if mutant != "hi_a_lo_b_dropped":
            out = out + ah[:, s] @ bl[:, s].t()
        if mutant != "lo_a_hi_b_dropped":
            out = out + al[:, s] @ bh[:, s].t()
        return out
    return f


def k_step(kernel_name):
    return {"x3": 32, "mfma_t1": 32, "mfma_t2": 8}[kernel_name]


def simulate(inp, kernel_name, f=None, f_ldc=None, mutant=None):
    """-> (C, aux or None) in fp32 as the (mutated) kernel would return them"""
    M, K, S, kchunk = inp["M"], inp["K"], inp["S"], inp["kchunk"]
    kernel = "x3" if kernel_name == "x3" else "mfma"
    dev = _dev_product(inp["a"], inp["w"], kernel, mutant)
    P = dev(0, K)
    if mutant == "k_tail_zeroed":
        tail = K % k_step(kernel_name)
        assert tail
        P = dev(0, K - tail)
    if mutant in ("k_row_beyond_kend", "slab_skipped", "slab_twice"):
        assert S > 1
    if mutant == "k_row_beyond_kend":
        P = P + dev(kchunk, kchunk + 1)
    if mutant == "slab_skipped":
        P = dev(0, (S - 1) * kchunk)
    if mutant == "slab_twice":
        P = P + dev((S - 1) * kchunk, K)
    bias, res = inp["bias"], inp["res"]
    if mutant == "bias_shifted":
        bias = torch.roll(bias, 1)
    if mutant == "residual_row_plus1":
        assert res.dim() == 2
        res = torch.roll(res, -1, 0)
    fm = f_ldc if mutant == "mask_index_ldc" else f
    ref = NT.reference(inp, fm, (P, P.abs()), bias=bias, res=res)
    C = ref["C"].clone()
    aux = None if ref["aux"] is None else ref["aux"].clone()
    if mutant == "aux_masked":
        aux = aux * fm.double()
    if mutant == "tiles_swapped":
        assert M > 128
        r = min(128, M - 128)
        top = C[:r].clone()
        C[:r] = C[128:128 + r]
        C[128:128 + r] = top
    if mutant == "lane_cols_rotated":
        C[16:32, 4:8] = torch.roll(C[16:32, 4:8], 1, 1)
    return C.float(), (None if aux is None else aux.float())


def simulate_group(pairs, S, mutant=None):
    """pairs [(A_i [K, M_i], B_i [K, N_i])] -> [C_i] fp32 as the (mutated) grouped bf16x3 launch would return them"""
    outs = [X3.matmul(a.t(), b) for a, b in pairs]
    if mutant == "group_fold_offset":  # problem 0 folded from problem 1's element offset in the concatenated index space
        flat = torch.cat([c.reshape(-1) for c in outs])
        n0 = outs[0].numel()
        outs[0] = flat[n0:2 * n0].reshape(outs[0].shape).clone()
    if mutant == "group_tile_other_n":  # the tiles of problem i laid out with the tile columns of problem i + 1
        for i in range(len(outs)):
            M, N = outs[i].shape
            gx, gy = -(-N // 128), -(-M // 128)
            gx_wrong = -(-outs[(i + 1) % len(outs)].shape[1] // 128)
            if gx_wrong == gx:
                continue
            got = torch.zeros_like(outs[i])  # (slab elements no tile writes: whatever the workspace held)
            for local in range(gx * gy):
                by, bx = divmod(local, gx_wrong)
                got[by * 128:(by + 1) * 128, bx * 128:(bx + 1) * 128] = outs[i][by * 128:(by + 1) * 128, bx * 128:(bx + 1) * 128]
            outs[i] = got
    return [c.float() for c in outs]


def group_products(pairs):
    """per problem dict(P, magP, emu, mag3) on the logical A^T [M, K], B^T [N, K]"""
    return [products(a.t().contiguous(), b.t().contiguous()) for a, b in pairs]


def check_group(what, family, K, prods, outs):
    """the grouped launch's outputs: bit for bit on "exact", within the two bf16x3 bounds (no epilogue) otherwise"""
    stats = {}
    for i, (pr, c) in enumerate(zip(prods, outs)):
        if family == "exact":
            want = pr["emu"].float()
            assert torch.equal(want.double(), pr["emu"])
            bad = int((c != want).sum())
            if bad or not bool(torch.isfinite(c).all()):
                raise BitsDiffer(f"{what}: problem {i}: {bad} of {c.numel()} elements differ from the exact result")
            stats[f"C{i}"] = 0.0
            continue
        stats[f"C{i}"] = NT._ratio(c, pr["P"], x3_exact_factor(K) * pr["magP"])
        # (K >= 512 here: the emulation bound holds but is too loose to catch a lost cross term; "exact" data does that)
        stats[f"C{i}_emu"] = NT._ratio(c, pr["emu"], x3_emu_factor(K) * pr["mag3"])
    bad = {k: v for k, v in stats.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1: {bad} (all: {stats})"
    return {k: round(v, 4) for k, v in stats.items()}
