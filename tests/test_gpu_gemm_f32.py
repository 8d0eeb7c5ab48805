"""-m gpu: every variant of the parity-mode fp32 GEMM family that csrc/gemm_f32.hip can launch, element by element against the
fp64 reference of tests/gemm_f32_util.py (bounds, data families and their reasons: that module's docstring;
tests/test_gemm_f32_ref_cpu.py shows without a device that they bite).  Reached through avf_gemm_f32_ex and
avf_gemm_f32_tn_group; every case first asserts with avf_gemm_f32_plan / avf_gemm_f32_tn_group_plan - the launcher's own
decision - the kernel, orientation (AKF / BKF), split count, rows per split and access width it expects.

The case table is gemm_f32_util.CASES / GROUP_CASES:
  x3*          gemm_f32x3_kernel unsplit: NT / NN / TN / TT x {96 x 96, 128 x 128, 129 x 130, 257 x 132} x K = 32 .. 160 (one to
               five K-steps), TN with K = 40 and 100 (KTAIL), the four epilogues, dropout off and p = 0.2; vec switched off by
               N % 4, by an odd ldc, by a bias one float off, by an odd ldres, by an odd ldaux; ldres = 0
  x3_split*    the same kernel split 2 and 3 ways + gemm_f32_fold_kernel (NONE, BIAS_RES with and without dropout, ldres = 0),
               vec and non-vec slab stores, a ragged last K-step inside the last split; and the same call without a workspace
  t1 / t2*     gemm_f32_kernel<T = 1 | 2> unsplit and split, under "f32" and - for shapes f32x3_ok turns away - under "bf16x3"
  groups       gemm_f32x3_group_kernel + gemm_f32x3_group_fold_kernel with 2, 3 and 4 problems, dense and row-strided

Every run: operands as views into NaN-filled parents, outputs in sentinel-guarded parents, a sentinel tail right after the
workspace bytes avf_gemm_workspace_bytes promised, C (and aux) element-wise within the bounds - or bit for bit on the "exact"
family, which every NONE / BIAS_RES case also runs -, a second call with the same bits, one "GEMMF32STAT {json}" line with the
worst error / bound ratio per output.

gemm_f32_kernel's NONE / BIAS_RES results without dropout are also compared BIT FOR BIT with the k-ordered fmaf chain its
header promises (gemm_f32_util.fmaf_chain: per split, splits folded in order, then bias and residual).

Worst error / bound ratios measured on an MI355X over the whole file (608 GEMMF32STAT lines, 221 of them bit-exact runs, which
all matched), per arithmetic, epilogue and output:
  gemm_f32_kernel, bound (K + S) U magP     NONE 0.824   BIAS_RES 0.875   BIAS_GELU 0.196   DGELU 0.156   aux 0.883
      the first two and aux at t2 TN 1000 x 1030 x 20, "wide", the GELU pair at t2 NT 1000 x 1030 x 8, "normal", p = 0.2.  The
      fmaf-chain claim stands: its worst case is not exceeded and the bits are the chain's; no factor 2 was needed.
  gemm_f32x3_kernel against the exact product   NONE 0.344   BIAS_RES 0.344   BIAS_GELU 0.253   DGELU 0.279   aux 0.345
  gemm_f32x3_kernel against its emulation       NONE 0.063   BIAS_RES 0.154   BIAS_GELU 0.056   DGELU 0.115   aux 0.043
      all ten at x3 TN 129 x 130 x 32, "wide" (one K-step: the largest share of the per-product term)
  grouped launch   exact product 0.022, emulation 0.0007 (3 problems, K = 1000, "wide"); against the per-problem launches 0.000
      of twice the emulation bound (they returned the same bits in every case here)
45 of the gemm_f32_kernel runs were compared with the fmaf chain and returned its bits.  The GELU / dGELU outputs use at most 0.28
of their whole bound with tanhf and with the exp2 / rcp forms alike: the activation constant (ACT = 16) is never the binding
term and stands for both kernels."""
import json

import pytest
import torch

import gemm_f32_util as G
import gemm_nt_util as NT
from gpu_util import SENTINEL, _bias_in_nan, _guarded, _guards_intact, _in_nan, f32_arithmetic

pytestmark = pytest.mark.gpu

F32 = torch.float32
SEED, LAYER, SITE = 0x1234567887654321, 2, 1  # the dropout site, as ops.dropout_factors takes it
TAIL = 1024                                   # sentinel floats behind the promised workspace

REACHED = set()  # ("x3", orientation, vec, split) / ("mfma", T, split) / ("group", problems), as the plan queries reported them


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


def _note(plan):
    split = plan["S"] > 1
    if plan["kernel"] == "x3":
        orient = {(True, True): "NT", (True, False): "NN", (False, False): "TN", (False, True): "TT"}[(plan["akf"], plan["bkf"])]
        REACHED.add(("x3", orient, plan["vec"], split))
    else:
        REACHED.add(("mfma", int(plan["kernel"][-1]), split))


def _nan_rows(t, pad, pre=4):
    """_in_nan for operands that must stay 16-byte aligned whatever their row length: four NaN rows in front"""
    R, Cn = t.shape
    buf = torch.full((R + pre + 1, Cn + pad), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[pre:pre + R, :Cn]
    view.copy_(t)
    return view


def _lay_a(stored, mode):
    if mode == "off1":  # one float past a 16-byte boundary, lda = row + 8: a NaN column in front of every row
        wide = torch.cat([torch.full((stored.shape[0], 1), float("nan")), stored], 1)
        return _in_nan(wide, pad=7)[:, 1:]
    return _in_nan(stored, pad=9 if mode == "pad9" else 8)


def _vec_in_nan(v, off):
    """a [N] vector `off` floats past a 16-byte boundary, NaN around"""
    if off == 0:
        return _bias_in_nan(v)
    buf = torch.full((v.numel() + 12,), float("nan"), dtype=F32, device="cuda")
    buf[4 + off:4 + off + v.numel()] = v
    return buf[4 + off:4 + off + v.numel()]


_cache = {}


def _operands(i, case, family):
    """A, W, their fp64 products and the device layouts, once per (case, data)"""
    key = (i, family)
    if key not in _cache:
        _cache.clear()  # one entry: the runs come grouped by case and family
        M, N, K = case["M"], case["N"], case["K"]
        a, w = G.make_operands(M, N, K, M * 7919 + N * 31 + K + i, family, w_lo=case["kernel"] == "x3")
        a_dev = _lay_a(a.t().contiguous() if case["ta"] else a, case["a"])
        b_dev = _in_nan(w if case["tb"] else w.t().contiguous())
        _cache[key] = dict(a=a, w=w, prod=G.products(a, w), a_dev=a_dev, b_dev=b_dev)
    return _cache[key]


_factors = {}


def _drop_factors(ops, M, N, p):
    """the device's own factors of the site over the flat element index m * N + n"""
    if (M, N, p) not in _factors:
        _factors.clear()
        n = -(-M * N // 4) * 4
        _factors[(M, N, p)] = ops.dropout_factors(SEED, LAYER, SITE, p, 1, n).cpu().view(-1)[:M * N].view(M, N).clone()
    return _factors[(M, N, p)]


def run(ops, i, case, epi, family, drop, workspace=True):
    """one call of gemm_f32_ex under the case's arithmetic, checked in full -> C on the device"""
    M, N, K = case["M"], case["N"], case["K"]
    p = 0.0 if not drop else (G.P_DROP_EXACT if family == "exact" else G.P_DROP)
    what = f"{G.case_id(case)}/{G.EPI_NAMES[epi]}/p={p}/ws={int(workspace)}/{family}"
    op = _operands(i, case, family)
    S, kchunk = (case["S"], case["kchunk"]) if workspace else (1, 0)
    inp = G.make_inputs(M, N, K, M + N + K + i, family, epi, (op["a"], op["w"]), S, kchunk, res_row=case["res"] == "row")
    f = _drop_factors(ops, M, N, p) if drop else None
    bias = None if inp["bias"] is None else _vec_in_nan(inp["bias"], case["bias_off"])
    res = None
    if inp["res"] is not None:
        res = _bias_in_nan(inp["res"]) if case["res"] == "row" else _in_nan(inp["res"], pad=9 if case["res"] == "pad9" else 8)
    aux_in = None if inp["aux_in"] is None else _in_nan(inp["aux_in"], pad=case["aux_pad"])
    promised = ops.gemm_f32_workspace_bytes(M, N, K, case["ta"], case["tb"])
    assert promised % 4 == 0 and promised >= (S * M * N * 4 if S > 1 else 0), (what, promised)

    def call():
        cbuf, cview, cpre = _guarded(M, N, F32, pad=case["c_pad"])
        abuf = aview = apre = None
        if epi == G.EPI_BIAS_GELU:
            abuf, aview, apre = _guarded(M, N, F32, pad=case["aux_pad"])
        wbuf = torch.full((promised // 4 + TAIL,), SENTINEL, dtype=F32, device="cuda")
        with f32_arithmetic(case["arith"]):
            c, aux, plan = ops.gemm_f32_ex(op["a_dev"], op["b_dev"], case["ta"], case["tb"], out=cview, epilogue=epi, bias=bias,
                                           residual=res, aux=aview if epi == G.EPI_BIAS_GELU else aux_in,
                                           drop=(SEED, LAYER, SITE, p) if drop else None,
                                           workspace=wbuf[:promised // 4] if workspace else None)
        torch.cuda.synchronize()
        _guards_intact(what + ":C", cbuf, cview, cpre)
        if abuf is not None:
            _guards_intact(what + ":aux", abuf, aview, apre)
        assert bool((wbuf[promised // 4:] == SENTINEL).all()), what + ": a write behind the promised workspace"
        if plan["S"] == 1:
            assert bool((wbuf == SENTINEL).all()), what + ": an unsplit launch wrote to the workspace"
        return c, (aux if epi == G.EPI_BIAS_GELU else None), plan

    c, aux, plan = call()
    _note(plan)
    want = dict(kernel=case["kernel"] if workspace or case["kernel"] != "mfma_t2" else "mfma_t1", akf=not case["ta"], bkf=case["tb"],
                S=S, kchunk=kchunk)
    assert {k: plan[k] for k in want} == want, (what, plan)
    if case["kernel"] == "x3":
        assert plan["vec"] == G.case_vec(case, epi), (what, plan)
    c2, aux2, _ = call()
    for n_, x, y in (("C", c, c2), ("aux", aux, aux2)):
        assert x is None or torch.equal(x, y), f"{what}:{n_}: a second call differs"
        assert x is None or bool(torch.isfinite(x).all()), f"{what}:{n_}: not finite (a read outside an operand?)"
    stats = G.check_case(what, inp, G.kernel_of(case), f, op["prod"], c.cpu(), None if aux is None else aux.cpu())
    if G.kernel_of(case) == "mfma" and epi in (G.EPI_NONE, G.EPI_BIAS_RES) and not drop and family != "exact":
        rows = G.chain_rows(M)  # the header's claim to the letter: "bit-for-bit a k-ordered fmaf chain"
        assert torch.equal(c.cpu()[rows], G.fmaf_chain(inp, rows)), what + ": not the k-ordered fmaf chain (+ fold, bias, residual)"
        stats["fmaf_chain_rows"] = len(rows)
    if drop:
        stats.update(NT.mask_not_vacuous(G.reference(inp, "f32", f, op["prod"])))
    print("GEMMF32STAT " + json.dumps(dict(case=case["name"], orient=case["orient"], shape=[M, N, K], epi=G.EPI_NAMES[epi], p=p,
                                           family=family, arith=case["arith"], ws=int(workspace), **plan, **stats)))
    return c


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=[G.case_id(c) for c in G.CASES])
def test_case(ops, i):
    case = G.CASES[i]
    family = G.case_family(i)
    for epi in case["epis"]:
        for drop in ((False,) if epi == G.EPI_NONE else (False, True)):
            run(ops, i, case, epi, family, drop)
    for epi in case["epis"]:  # the bit-exact family: the cheapest and sharpest check, on every NONE / BIAS_RES case
        if epi not in (G.EPI_NONE, G.EPI_BIAS_RES):
            continue
        for drop in ((False,) if epi == G.EPI_NONE else (False, True)):
            c = run(ops, i, case, epi, "exact", drop)
            if case["S"] > 1:  # the same call without a workspace runs unsplit and agrees (here: in every bit)
                c1 = run(ops, i, case, epi, "exact", drop, workspace=False)
                assert torch.equal(c, c1), f"{G.case_id(case)}/{G.EPI_NAMES[epi]}: split and unsplit differ on exact data"
    if case["S"] > 1:  # ... and within the bounds on the case's own family
        for epi in case["epis"]:
            run(ops, i, case, epi, family, epi != G.EPI_NONE, workspace=False)


def _flat_guarded(M, N):
    buf = torch.full((M * N + 128,), SENTINEL, dtype=F32, device="cuda")
    return buf, buf[64:64 + M * N].view(M, N)


@pytest.mark.parametrize("gi", range(len(G.GROUP_CASES)), ids=[f"{len(g[0])}x-K{g[1]}-{'strided' if g[2] else 'dense'}" for g in G.GROUP_CASES])
def test_group(ops, gi):
    shapes, K, strided, S, kchunk = G.GROUP_CASES[gi]
    n = len(shapes)
    for family in (G.BOUNDED[gi % 3], "exact"):
        what = f"group{n}/K={K}/strided={int(strided)}/{family}"
        pairs = []
        for j, (M, N) in enumerate(shapes):
            a, w = G.make_operands(M, N, K, 977 * gi + 31 * j + K, family)
            pairs.append((a.t().contiguous(), w.t().contiguous()))  # A_j [K, M], B_j [K, N]: token-major, as the layer holds them
        prods = G.group_products(pairs)
        dev = [(_nan_rows(a, 4 if strided else 0), _nan_rows(b, 4 if strided else 0)) for a, b in pairs]
        with f32_arithmetic("bf16x3"):
            plan = ops.gemm_f32_tn_group_plan(shapes, K)
            tiles = sum(-(-m // 128) * -(-k // 128) for m, k in shapes)
            assert plan["ok"] and plan["tiles"] == tiles and plan["S"] == S and plan["kchunk"] == kchunk, (what, plan)
            promised = plan["workspace_bytes"]
            assert promised == 4 * S * sum(m * k for m, k in shapes), (what, plan)
            REACHED.add(("group", n))

            def call():
                outs = [_flat_guarded(M, N) for M, N in shapes]
                wbuf = torch.full((promised // 4 + TAIL,), SENTINEL, dtype=F32, device="cuda")
                cs = ops.gemm_f32_tn_group(dev, outs=[v for _, v in outs], workspace=wbuf[:promised // 4])
                torch.cuda.synchronize()
                for j, (buf, v) in enumerate(outs):
                    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + v.numel():] == SENTINEL).all()), f"{what}: a write outside C{j}"
                assert bool((wbuf[promised // 4:] == SENTINEL).all()), what + ": a write behind the promised workspace"
                return cs

            cs = call()
            cs2 = call()
            # the per-problem launches on the same data (gemm_f32x3_kernel<false, false>, split on its own)
            singles = [ops.gemm_f32_ex(a, b, True, False)[0] for a, b in dev]
            torch.cuda.synchronize()
        for j in range(n):
            assert torch.equal(cs[j], cs2[j]), f"{what}: C{j}: a second call differs"
        outs = [c.cpu() for c in cs]
        stats = G.check_group(what, family, K, prods, outs)
        for j, (one, pr) in enumerate(zip(singles, prods)):
            if family == "exact":
                assert torch.equal(one, cs[j]), f"{what}: C{j}: the grouped and the single launch differ on exact data"
            else:  # each is within 6 K U mag3 of the emulation, whatever its order and split: twice that apart at most
                r = NT._ratio(one.cpu(), outs[j].double(), 2.0 * G.x3_emu_factor(K) * pr["mag3"])
                assert r <= 1.0, f"{what}: C{j}: grouped and single launch are {r} of the accumulation bound apart"
                stats[f"C{j}_vs_single"] = round(r, 4)
        print("GEMMF32STAT " + json.dumps(dict(case="group", problems=n, K=K, strided=int(strided), family=family, **plan, **stats)))


def test_group_refuses_what_its_plan_turns_away(ops):
    """one problem, N % 4 != 0, M < 96, K < 512: the plan says not eligible and the call raises before it launches"""
    with f32_arithmetic("bf16x3"):
        for shapes, K, why in G.GROUP_INELIGIBLE:
            plan = ops.gemm_f32_tn_group_plan(shapes, K)
            assert not plan["ok"] and plan["workspace_bytes"] == 0, (why, plan)
            dev = [(torch.zeros(K, M, device="cuda"), torch.zeros(K, N, device="cuda")) for M, N in shapes]
            outs = [_flat_guarded(M, N) for M, N in shapes]
            with pytest.raises(RuntimeError, match="not eligible"):
                ops.gemm_f32_tn_group(dev, outs=[v for _, v in outs])
            torch.cuda.synchronize()
            for buf, _ in outs:
                assert bool((buf == SENTINEL).all()), why + ": a refused call wrote to C"


def test_every_variant_was_reached():
    """coverage by assertion: over this file the plan queries have reported the bf16x3 kernel in every orientation, with and
    without 16-byte accesses, unsplit and split; gemm_f32_kernel on both tiles, unsplit and split; and the grouped launch with
    2, 3 and 4 problems (runs last; needs the tests above to have run)"""
    want = {("x3", o, v, s) for o in G.ORIENT for v in (True, False) for s in (True, False)}
    want |= {("mfma", t, s) for t in (1, 2) for s in (True, False)}
    want |= {("group", n) for n in (2, 3, 4)}
    assert want <= REACHED, sorted(want - REACHED, key=str)
