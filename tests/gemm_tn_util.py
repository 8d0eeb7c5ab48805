"""fp64 reference, element-wise bound, data families, mutants and the case table for the bf16 weight-gradient (TN) GEMM family
of csrc/gemm_bf16.hip: gemm_bf16_tn_kernel + fold_slabs_kernel (one problem, up to 32 split-K slabs), gemm_bf16_tn_group_kernel<2|4>
(grouped, 128 x 128 tile), gemm_bf16_tn_group_big_kernel<3> (grouped, 256 x 128 tile, three block orders) and fold_group_kernel<SS>.
CPU only: tests/test_gpu_gemm_tn.py feeds it what the device returned, tests/test_gemm_tn_ref_cpu.py shows without a device that
the bound bites, that an honest fp32 computation stays inside it, and that the case table below plans to the variants it names.

The operation:  C[M, N] = A[K, M]^T B[K, N],  magC = |A|^T |B|   (bf16 operands are exact in fp64).

Bound on |device - reference| per ELEMENT, with U = 2^-24 (half an fp32 ulp, relative):   (2 K + S) * U * magC.
  accumulation  A product of two bf16 values is exact in fp32 (8 + 8 significand bits).  Slab s sums the k_s reduction rows of
                its K-range in fp32: in any order that errs by at most k_s * U * mag_s, mag_s = the slab's share of magC; the
                factor 2 covers the rounding inside the MFMA's 32-term sum, which is not documented (tests/gemm_nt_util.py
                takes the same term, measured there at most 0.914 used).  The ranges partition K, so sum_s 2 k_s U mag_s
                <= 2 K U magC.
  fold          S slabs are added with S - 1 fp32 additions; each rounds a partial sum whose magnitude is at most magC
                (1 + 2 K U), i.e. adds at most U magC up to second order: (S - 1) U magC <= S U magC.  S = 1: no fold, and
                the term is one spare U magC.
A slab of a K-range that starts past the end of K ("dead") must hold zeros: the fold adds it like any other.

Data families (make_operands), each along the reduction rows:
  "normal"  randn.
  "wide"    magnitudes of A spread over six decades inside every column's reduction.
  "cancel"  the second half of the reduction rows undoes the first up to 2^-6: |C| << magC, the slabs are large and cancel.
  "int"     integers in [-8, 8]: every product and every partial sum (|sum| <= 64 K < 2^24 for K <= 2^18) is an integer that
            fp32 holds exactly, so the result equals the fp64 product BIT FOR BIT whatever the order, split or fold."""
import torch

FAMILIES = ("normal", "wide", "cancel", "int")
U = 2.0 ** -24
TR = 64                # reduction rows per K-step of every TN kernel
SENTINEL = -24576.0    # exact in fp32 and bf16; no family produces it


def make_operands(K, M, N, seed, family):
    """bf16 A [K, M] and B [K, N] of a data family"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed)
    if family == "int":
        a = torch.randint(-8, 9, (K, M), generator=g).float()
        b = torch.randint(-8, 9, (K, N), generator=g).float()
        return a.bfloat16(), b.bfloat16()
    a = torch.randn(K, M, generator=g)
    b = torch.randn(K, N, generator=g)
    if family == "wide":
        a = a * torch.pow(10.0, torch.rand(K, M, generator=g) * 6 - 3)
    elif family == "cancel":
        h = K // 2
        a[h:2 * h] = -a[:h]
        b[h:2 * h] = b[:h] * (1.0 + 2.0 ** -6 * torch.randn(h, N, generator=g))
    return a.bfloat16(), b.bfloat16()


def products(a, b):
    """C and magC in fp64"""
    a, b = a.double(), b.double()
    return a.t() @ b, a.abs().t() @ b.abs()


def bound(mag, K, S):
    return (2.0 * K + S) * U * mag


def split_kchunk(K, S):
    """reduction rows per split as split_plan (csrc/gemm_dispatch.hpp) cuts them: whole K-steps of 64"""
    per = -(-K // S)
    return -(-per // TR) * TR


def slab_steps(K, S, kchunk):
    """K-steps of 64 rows (the last may be ragged) each split runs; 0 = a dead slab"""
    return [max(0, -(-(min(s * kchunk + kchunk, K) - s * kchunk) // TR)) for s in range(S)]


def ratio(got, ref, mag, K, S):
    """worst |got - ref| / bound; inf where got is not finite"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bound(mag, K, S).clamp_min(1e-300)).max())


def check(what, got, ref, mag, K, S, family):
    """assert got [M, N] fp32 element-wise within the bound, and equal to the reference on "int" -> error / bound"""
    assert got.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, got.shape)
    r = ratio(got, ref, mag, K, S)
    assert r <= 1.0, f"{what}: error / bound above 1: {r}"
    if family == "int":
        assert torch.equal(got.double(), ref), f"{what}: an integer product is not exact (error / bound {r})"
    return r


# ------------------------------------------------------------------------------------------------
# The honest chain and its mutants.  chain() is what a correct kernel family computes, in fp32: one float32 matmul per slab
# (a dead slab is zeros), folded in slab order in fp32.  A mutant is one subtle mistake applied to it.
MUTANTS = (
    "kstep_dropped",       # one 64-row K-step left out of one 16 x 16 block (a ring slot read before it landed)
    "slab_dropped",        # the fold leaves one slab out                                  (S >= 2)
    "slab_twice",          # the fold adds one slab twice                                  (S >= 2)
    "dead_slab_nan",       # a slab past the end of K is not written: the fold adds what the workspace held (NaN)  (dead slab)
    "cols_swapped",        # two 16-column blocks of the output swapped
    "tile_transposed",     # the leading 128 x 128 tile transposed                        (M, N >= 128)
    "float4_sentinel",     # one float4 of the output never stored
    "row_k_included",      # the reduction runs one row past K (a NaN guard row)
    "bf16_accumulate",     # the accumulator rounded to bf16 after every K-step
)


def chain(a, b, S, mutant=None):
    """A [K, M], B [K, N] bf16 -> C [M, N] fp32 by S slabs of split_kchunk(K, S) rows"""
    K, M = a.shape
    N = b.shape[1]
    kchunk = split_kchunk(K, S)
    af, bf = a.float(), b.float()
    slabs = []
    for s in range(S):
        kb, ke = s * kchunk, min(s * kchunk + kchunk, K)
        if ke <= kb:
            slabs.append(torch.full((M, N), float("nan")) if mutant == "dead_slab_nan" else torch.zeros(M, N))
            continue
        if mutant == "bf16_accumulate":
            acc = torch.zeros(M, N)
            for k0 in range(kb, ke, TR):
                acc = (acc + af[k0:min(k0 + TR, ke)].t() @ bf[k0:min(k0 + TR, ke)]).bfloat16().float()
        else:
            acc = af[kb:ke].t() @ bf[kb:ke]
        if mutant == "kstep_dropped" and s == S // 2:
            r0, c0 = (16 if M >= 32 else 0), (32 if N >= 48 else 0)
            k1 = min(kb + TR, ke)
            acc[r0:r0 + 16, c0:c0 + 16] -= af[kb:k1, r0:r0 + 16].t() @ bf[kb:k1, c0:c0 + 16]
        if mutant == "row_k_included" and ke == K:
            acc = acc + float("nan")
        slabs.append(acc)
    if mutant == "dead_slab_nan":
        assert any(bool(torch.isnan(x).any()) for x in slabs), "dead_slab_nan needs a split that starts past K"
    if mutant in ("slab_dropped", "slab_twice"):
        assert S >= 2
    c = slabs[0].clone()
    for s in range(1, S):
        if mutant == "slab_dropped" and s == S - 1:
            continue
        c = c + slabs[s]
        if mutant == "slab_twice" and s == 1:
            c = c + slabs[s]
    if mutant == "cols_swapped":
        assert N >= 48
        blk = c[:, 16:32].clone()
        c[:, 16:32] = c[:, 32:48]
        c[:, 32:48] = blk
    if mutant == "tile_transposed":
        assert M >= 128 and N >= 128
        c[:128, :128] = c[:128, :128].t().clone()
    if mutant == "float4_sentinel":
        c[M // 2, 4:8] = SENTINEL
    return c


# ------------------------------------------------------------------------------------------------
# The case table of tests/test_gpu_gemm_tn.py.  tests/test_gemm_tn_ref_cpu.py asks the library (avf_gemm_tn_group_plan,
# avf_gemm_tn_plan: host code, no device) that every row plans to what it names, before a row ever reaches a GPU.
R4 = [(264, 136), (8, 8), (256, 128), (120, 248)]  # ragged and full in both extents of both tiles; a one-tile problem
_R16_SHAPES = [(136, 72), (256, 128), (264, 136), (512, 64)]
R16 = [_R16_SHAPES[(i + i // 4) % 4] for i in range(16)]  # the list of test_gpu_dw_deferred.py::test_gemm_tn_group_8_and_16_problems
P2 = [(136, 72), (8, 264)]
SQ1024 = [(1024, 1024)]
GROUPS = {"R4": R4, "R16": R16, "P2": P2, "SQ1024": SQ1024}


def xcd_order(S, on=True):
    """TnGroup::xcd_groups of the 256 x 128 kernel for a split count"""
    if not on:
        return 0
    return 8 // S if S in (1, 2, 4, 8) else -1


def _rows(group, Ks, splits, big, waves, xcd_on=True, heuristic_S=None):
    """rows (group name, K, forced split count or None, what the plan must say)"""
    out = []
    for K in Ks:
        for sp in splits:
            S = sp if sp is not None else heuristic_S(K)
            want = dict(big=big, waves=waves, S=S, fold=(-1 if S == 1 else (S if S <= 8 else 0)),
                        xcd_groups=xcd_order(S, xcd_on) if big else 0)
            out.append((group, K, sp, want))
    return out


# child name -> (environment beside AVF_TUNING=1, rows).  AVF_TN_BIG / AVF_TN_XCD are read once per process;
# AVF_TN_SPLITS per call: a child sweeps it.
CHILDREN = {
    "default": ({},
                _rows("R16", [320], [None, 1, 2, 3, 5, 8, 9], 0, 4, heuristic_S=lambda K: 1)
                + _rows("P2", [256 * s for s in range(1, 9)], [None], 0, 4, heuristic_S=lambda K: K // 256)  # fold <2..8> unforced
                + _rows("SQ1024", [2048], [None], 1, 8, heuristic_S=lambda K: 8)),      # the heuristic's own 256 x 128 pick
    "big": ({"AVF_TN_BIG": "1"},
            _rows("R4", [320, 448], list(range(1, 10)), 1, 8)
            + _rows("SQ1024", [576], [9], 1, 8)   # 288 workgroups on 256 slots: a second round
            + _rows("R16", [192], [1, 3], 1, 8)),
    "big_tile_major": ({"AVF_TN_BIG": "1", "AVF_TN_XCD": "0"}, _rows("R4", [320], [1, 3, 8], 1, 8, xcd_on=False)),
}

# the single-problem path: (M, N, K) -> the plan avf_gemm_tn_plan must report
SINGLE = [
    ((8, 8, 8), dict(S=1, kchunk=64)),
    ((264, 136, 72), dict(S=1, kchunk=128)),      # a full K-step and a ragged one of 8 rows
    ((128, 128, 64), dict(S=1, kchunk=64)),
    ((48, 40, 1000), dict(S=3, kchunk=384)),      # last chunk 3 * 64 + 40 rows
    ((136, 264, 2568), dict(S=10, kchunk=320)),   # splits 0 .. 7 full, split 8 = the 8-row tail, split 9 dead
    ((8, 8, 8192), dict(S=32, kchunk=256)),
]


def kernel_of(plan):
    return "big" if plan["big"] else "g128"


def reached_by_group(plan, K):
    """what a grouped launch of this plan exercises, as a set of facts"""
    kern = kernel_of(plan)
    steps = slab_steps(K, plan["S"], plan["kchunk"])
    out = {("kernel", kern), ("fold", plan["fold"])}
    if 0 in steps:
        out.add(("dead", kern))
    if plan["big"]:
        out.add(("xcd", plan["xcd_groups"]))
        out |= {("steps", min(n, 7)) for n in steps}  # 7 = seven or more: the ring has wrapped twice
    return out


def reached_by_single(plan, K):
    out = {("kernel", "single"), ("single_S", plan["S"])}
    if 0 in slab_steps(K, plan["S"], plan["kchunk"]):
        out.add(("dead", "single"))
    return out


# what the whole GPU file must have reached (test_every_variant_was_reached; proven on the CPU for the table first)
WANT = ({("kernel", k) for k in ("single", "g128", "big")}
        | {("fold", f) for f in (-1, 0, 2, 3, 4, 5, 6, 7, 8)}
        | {("xcd", x) for x in (8, 4, 2, 1, -1, 0)}
        | {("dead", k) for k in ("single", "g128", "big")}
        | {("steps", n) for n in (0, 1, 2, 3, 4, 5, 7)}
        | {("single_S", s) for s in (1, 3, 10, 32)})
