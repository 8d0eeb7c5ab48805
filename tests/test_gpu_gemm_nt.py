"""-m gpu: every variant of the tiled bf16 NT GEMM that csrc/gemm_bf16.hip can launch, element by element against the fp64
reference of tests/gemm_nt_util.py (bounds and their reasons: that module's docstring; tests/test_gemm_nt_ref_cpu.py shows
without a device that they bite).  Reached through avf_gemm_nt_ex; every case first asserts with avf_gemm_nt_plan - the
launcher's own decision - that it runs the kernel, tile and LEAN code it names.

variant (pick_nt_tile_bf16, kWorkgroupSlots = 512)      kernel                                              shapes (M, N, K)
K % 64 != 0                                             gemm_bf16_nt_kernel + nt_epilogue                   REG
M <= 2048, few tiles: tile 6 (32 x 64, 3 stages)        gemm_bf16_nt_glds_kernel<.., 1, 4, 2, 1, 3>         TILE6
tile 5 (96 x 128, 8 waves), N % 128 == 0                ... <.., 2, 4, 3, 2, 2, LEAN 1 / 2 / 5 / 6>         TILE5_LEAN
tile 5, ragged N                                        ... <.., 2, 4, 3, 2, 2, 0> + nt_epilogue            TILE5_GEN
tile 1 (64 x 128, 4 waves)                              ... <.., 2, 2, 2, 4, 2, 0>                          TILE1
tile 2 (128 x 128, 8 waves), N % 128 == 0               ... <.., 2, 4, 4, 2, 2, LEAN 1 / 2 / 5 / 6>         TILE2_LEAN
tile 2, ragged N                                        ... <.., 2, 4, 4, 2, 2, 0>                          TILE2_GEN

Every case: the four epilogues (one test each), bf16 and fp32 C, dropout off and p = 0.2 on the fused epilogues, column sums
on DGELU (LEAN 2 / 6 on the lean tiles) and on NONE for one general shape per kernel; C, aux and the column sums element-wise
within the bounds; outputs in sentinel-guarded parents (rows before and after, columns N .. N + 7); operands as views into
NaN-filled parents; a second call returns the same bits.  The fp32-C runs read a row-strided W (ldb = K + 8: no weight
warm-up), the bf16-C runs a dense one (warm-up on where the grid leaves slots empty: asserted on tile 5).  Each run prints a
line "GEMMSTAT {json}" with the worst error / bound ratio per output.

Worst error / bound ratios measured on an MI355X over the whole file (230 runs), all at REG 257 x 136 x 8, "wide" data:
  fp32 C   NONE 0.914   BIAS_RES 0.829   BIAS_GELU 0.118   DGELU 0.300      fp32 aux 0.914
  bf16 C   NONE 0.9999  BIAS_RES 0.9998  BIAS_GELU 0.9991  DGELU 0.9990     bf16 aux 0.9998
  column sums 0.060 (1 x 64 x 64; 0.0001 - 0.001 at M >= 2000)
The bf16 figures sit just under 1 by construction: among millions of elements some land within 1e-4 of a rounding tie, where
a correct round-to-nearest errs by half an ulp, which is the bound.  The activation constant (16) is never the binding term:
the GELU / dGELU outputs use at most 0.30 of their fp32 bound."""
import json

import pytest
import torch

import gemm_nt_util as G
from gpu_util import SENTINEL, _bias_in_nan, _guarded, _guards_intact, _in_nan  # noqa: F401

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DROP = (0x1234567887654321, 2, 1, 0.2)  # (seed, layer, site, p) as ops.dropout_factors takes them
EPIS = (G.EPI_NONE, G.EPI_BIAS_RES, G.EPI_BIAS_GELU, G.EPI_DGELU)

# name -> (kind, tile, lean tile?, shapes)
VARIANTS = {
    "REG": (0, -1, False, [(130, 132, 72), (257, 136, 8), (128, 128, 200)]),
    "TILE6": (1, 6, False, [(1, 64, 64), (33, 68, 64), (100, 260, 192), (2048, 896, 256)]),
    "TILE5_LEAN": (1, 5, True, [(2100, 256, 128), (2100, 128, 192)]),
    "TILE5_GEN": (1, 5, False, [(2100, 264, 128), (2100, 260, 64)]),
    "TILE1": (1, 1, False, [(3100, 2048, 64), (3100, 2044, 128)]),
    "TILE2_LEAN": (1, 2, True, [(4000, 2048, 64), (4096, 2048, 128)]),  # the ragged and the FULL last row tile
    "TILE2_GEN": (1, 2, False, [(4000, 2040, 64)]),
}
CASES = [(name, shape) for name, v in VARIANTS.items() for shape in v[3]]
# column sums on NONE (the general epilogue's): one general shape per kernel
NONE_COLSUM = {("REG", (130, 132, 72)), ("TILE5_GEN", (2100, 264, 128))}
LEAN_CASES = [(name, shape) for name, shape in CASES if VARIANTS[name][2]]

REACHED = set()  # what the plan query has reported: ("kind", k), ("tile", t), ("lean", l)


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


def _note(plan):
    REACHED.add(("kind", plan["kind"]))
    if plan["kind"] == 1:
        REACHED.add(("tile", plan["tile"]))
        REACHED.add(("lean", plan["lean"]))


_cache = {}


def _operands(shape, family):
    """A, W, P, magP and the device copies of A and W (dense-row and row-strided), once per (shape, data)"""
    key = (shape, family)
    if key not in _cache:
        _cache.clear()  # one entry: the cases come grouped by shape
        M, N, K = shape
        a, w = G.make_operands(M, N, K, M * 7919 + N * 31 + K, family)
        inp = dict(a=a, w=w)
        _cache[key] = dict(a=a, w=w, prod=G.products(inp), a_dev=_in_nan(a), w_strided=_in_nan(w), w_dense=_in_nan(w, pad=0))
    return _cache[key]


_factors = {}


def _drop_factors(ops, M, N):
    if (M, N) not in _factors:
        _factors.clear()
        _factors[(M, N)] = ops.dropout_factors(*DROP, M, N).cpu()
    return _factors[(M, N)]


def run(ops, name, shape, epi, cdt, p, colsum, lean_expected, dense_w, force_general_aux=False, light=False):
    """one call of gemm_nt_ex, checked in full -> (C, aux) on the device.  light: the plan and the guards only (the caller
    compares the bits with a fully checked run)"""
    kind, tile, _, _ = VARIANTS[name]
    M, N, K = shape
    family = G.FAMILIES[CASES.index((name, shape)) % 3]
    what = f"{name}{list(shape)}/{G.EPI_NAMES[epi]}/{str(cdt)[6:]}/p={p}/cs={int(colsum)}/{family}"
    op = _operands(shape, family)
    inp = G.make_inputs(M, N, K, M + N + K, family, cdt, epi, operands=(op["a"], op["w"]))
    f = _drop_factors(ops, M, N) if p and not light else None
    ref = None if light else G.reference(inp, f, op["prod"])
    w_dev = op["w_dense"] if dense_w else op["w_strided"]
    bias = None if inp["bias"] is None else _bias_in_nan(inp["bias"])
    res = None if inp["res"] is None else _in_nan(inp["res"])
    aux_in = None if inp["aux_in"] is None else _in_nan(inp["aux_in"], pad=4 if force_general_aux else 8)

    def call():
        cbuf, cview, cpre = _guarded(M, N, cdt)
        abuf = aview = apre = None
        if epi == G.EPI_BIAS_GELU:
            abuf, aview, apre = _guarded(M, N, cdt)
        c, aux, cs, plan = ops.gemm_nt_ex(op["a_dev"], w_dev, out=cview, epilogue=epi, bias=bias, residual=res,
                                          aux=aview if epi == G.EPI_BIAS_GELU else aux_in, want_colsum=colsum,
                                          drop=DROP if p else None)
        torch.cuda.synchronize()
        _guards_intact(what + ":C", cbuf, cview, cpre)
        if abuf is not None:
            _guards_intact(what + ":aux", abuf, aview, apre)
        return c, (aux if epi == G.EPI_BIAS_GELU else None), cs, plan

    c, aux, cs, plan = call()
    _note(plan)
    assert plan["kind"] == kind and plan["tile"] == tile and plan["lean"] == lean_expected, (what, plan)
    if kind == 1:
        assert plan["wpf"] == (dense_w and tile == 5), (what, plan)  # tile 5 here: 44 - 66 workgroups on 512 slots
    assert (cs is not None) == colsum and (aux is not None) == (epi == G.EPI_BIAS_GELU)
    if light:
        return c, aux
    c2, aux2, cs2, _ = call()
    for n_, x, y in (("C", c, c2), ("aux", aux, aux2), ("colsum", cs, cs2)):
        assert x is None or torch.equal(x, y), f"{what}:{n_}: a second call differs"
    for n_, x in (("C", c), ("aux", aux), ("colsum", cs)):
        assert x is None or bool(torch.isfinite(x).all()), f"{what}:{n_}: not finite (a read outside an operand?)"
    stats = G.check_outputs(what, ref, c.cpu(), None if aux is None else aux.cpu(), None if cs is None else cs.cpu())
    if p:
        stats.update(G.mask_not_vacuous(ref))
    print("GEMMSTAT " + json.dumps(dict(variant=name, shape=list(shape), epi=G.EPI_NAMES[epi], c=str(cdt)[6:], p=p,
                                        family=family, kind=plan["kind"], tile=plan["tile"], lean=plan["lean"],
                                        wpf=plan["wpf"], **stats)))
    return c, aux


def _lean_code(name, epi, p, colsum):
    """the LEAN code the launcher must pick on this variant (nt_lean_ok / nt_lean_exists in words)"""
    if not VARIANTS[name][2] or (colsum and epi != G.EPI_DGELU):
        return 0
    return (2 if colsum else 1) + (4 if p else 0)


@pytest.mark.parametrize("name,shape,epi", [(n, s, e) for n, s in CASES for e in EPIS],
                         ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}-{G.EPI_NAMES[e]}" for n, s in CASES for e in EPIS])
def test_variant(ops, name, shape, epi):
    lean_tile = VARIANTS[name][2]
    for cdt in (BF, F32):
        for p in ((0.0,) if epi == G.EPI_NONE else (0.0, DROP[3])):
            colsum = epi == G.EPI_DGELU or (epi == G.EPI_NONE and (name, shape) in NONE_COLSUM and cdt == BF)
            run(ops, name, shape, epi, cdt, p, colsum, _lean_code(name, epi, p, colsum), dense_w=cdt == BF)
    if epi == G.EPI_NONE and (name, shape) in NONE_COLSUM:  # ... and the same shape without them
        run(ops, name, shape, epi, BF, 0.0, False, 0, dense_w=False)
    if epi == G.EPI_DGELU and lean_tile:  # DGELU without column sums: the LEAN 1 / 5 instantiations of this epilogue
        i = CASES.index((name, shape)) % 2
        run(ops, name, shape, epi, (BF, F32)[i], (0.0, DROP[3])[i], False, 1 + 4 * i, dense_w=True)


@pytest.mark.parametrize("name,shape", LEAN_CASES, ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in LEAN_CASES])
def test_lean_epilogue_returns_the_bits_of_the_general_one(ops, name, shape):
    """nt_epilogue_lean_body promises "same arithmetic, same order, same bits": each epilogue once on the lean path and once
    with an argument that sends the same call to the general epilogue (column sums for NONE / BIAS_RES / BIAS_GELU, an aux
    with ldaux = N + 4 for DGELU), dropout off and on, one process.  test_variant holds the lean runs to the fp64 reference."""
    for epi in EPIS:
        # (an fp32 aux with ldaux = N + 4 still satisfies the lean path: DGELU can be sent to the general epilogue with bf16 C only)
        for cdt in ((BF,) if epi == G.EPI_DGELU else (BF, F32)):
            for p in ((0.0,) if epi == G.EPI_NONE else (0.0, DROP[3])):
                c_l, aux_l = run(ops, name, shape, epi, cdt, p, False, _lean_code(name, epi, p, False), dense_w=True, light=True)
                if epi == G.EPI_DGELU:
                    c_g, aux_g = run(ops, name, shape, epi, cdt, p, False, 0, dense_w=True, force_general_aux=True, light=True)
                else:
                    c_g, aux_g = run(ops, name, shape, epi, cdt, p, True, 0, dense_w=True, light=True)
                what = f"{name}{list(shape)}/{G.EPI_NAMES[epi]}/{cdt}/p={p}"
                assert torch.equal(c_l, c_g), what + ": C of the lean epilogue differs from the general one's"
                assert (aux_l is None) == (aux_g is None) and (aux_l is None or torch.equal(aux_l, aux_g)), what + ": aux differs"


def test_every_kernel_was_reached():
    """coverage by assertion: over this file the plan query has reported the register-staged kernel, every tile and every
    LEAN code (runs last; needs the tests above to have run)"""
    want = {("kind", 0), ("kind", 1)} | {("tile", t) for t in (1, 2, 5, 6)} | {("lean", l) for l in (0, 1, 2, 5, 6)}
    assert want <= REACHED, sorted(want - REACHED)
