"""-m gpu: every variant of the MX-FP8 NT GEMM that csrc/gemm_mx8.hip can launch, element by element against the fp64 reference
of tests/gemm_mx8_util.py (data families, bounds, the bit-for-bit checks and their reasons: that module's docstring;
tests/test_gemm_mx8_ref_cpu.py shows without a device that they bite).  Reached through avf_gemm_mx8_nt_ex; every case first
asserts with avf_gemm_mx8_nt_plan - the launcher's own decision - that it runs the tile and LEAN code it names.

variant (pick_nt_tile on (M, N, K / 2), kWorkgroupSlots = 512)   kernel                                           shapes
tile 5 (96 x 128, 8 waves), N % 128 == 0                        gemm_mx8_nt_kernel<.., 2, 4, 3, 2, LEAN 1 / 3 / 5 / 7>   TILE5_LEAN
tile 5, ragged N                                                ... <.., 2, 4, 3, 2, 0> + nt_epilogue                    TILE5_GEN
tile 1 (64 x 128, 4 waves)                                      ... <.., 2, 2, 2, 4, 0>                                  TILE1
tile 2 (128 x 128, 8 waves), N % 128 == 0                       ... <.., 2, 4, 4, 2, LEAN 1 / 3 / 5 / 7>                 TILE2_LEAN
tile 2, ragged N                                                ... <.., 2, 4, 4, 2, 0>                                  TILE2_GEN

Every case: the four epilogues (one test each) on "dense-int" data with bf16 and fp32 C, dropout off and p = 0.2 on the fused
epilogues (LEAN 0: this kernel has no lean dropout site), column sums on DGELU (LEAN 3 on the lean tiles) and on NONE for one
general shape per tile; EPI_NONE on both one-block-wide orientations (scale bytes 87 .. 167, zero blocks with scale byte 0) on
every variant and on "quantised" data for one shape per tile.  C, aux and the column sums element-wise within the bounds, and
for the exact families bit for bit where the module names it; outputs in sentinel-guarded parents; operand images as views into
0xFF-filled parents (e4m3 NaN, E8M0 NaN), row-strided (lda = ldb = K + 16 bytes) on the fp32-C runs; everything finite; a second
call returns the same bits.

The MX-FP8 image of C (BIAS_GELU, DGELU; N % 32 == 0).  Contract, read from nt_epilogue and nt_epilogue_lean_body: BOTH
epilogues quantise the fp32 value of the epilogue before its rounding to C's type (dropout factors applied).  fp32 C: the image
is oracle.mx8_quant of the stored C bit for bit, on "dense-int" data (LEAN 5 / 7 on the lean tiles, the general epilogue's
branch at (130, 160, 384) and on tile 1).  bf16 C: on "unit" data (integer products; aux = 30, bias = 64: the fp32 value is the
stored bf16 value) C is exact and the image is the conversion of it bit for bit.

Each run prints a line "MX8STAT {json}" with the worst error / bound ratio per output.

Worst error / bound ratios measured on an MI355X over the whole file (249 runs; every bit-for-bit comparison and all 37
images equal):
  exact families (eP = 0; what is left is the epilogue's own rounding)
    fp32 C   NONE 0 (C == P)   BIAS_RES 0 without dropout, 0.959 with (4000 x 2040 x 128)   BIAS_GELU 0.111   DGELU 0.345
             fp32 aux 0 (aux == P + bias)
    bf16 C   NONE 1.0   BIAS_RES 1.0   BIAS_GELU 0.9997   DGELU 0.9995   bf16 aux 1.0: a correct rounding of an exact value
             meets the half-ulp bound with equality at a tie, and the integer-valued data is full of ties
    column sums 0.21 (7 x 128 x 128, bf16 C, p = 0.2; below 0.01 at M >= 2000)
  "quantised" (eP = 2e-3 magP)   fp32 C 0.0065 (1.3e-5 magP: the three shapes here stay far inside the stated bound)
             bf16 C 0.76 (the half-ulp term dominates)
With dropout at least 85 % of the masked elements are non-zero before the mask."""
import json

import pytest
import torch

import gemm_mx8_util as X
from gpu_util import SENTINEL, _bias_in_nan, _guarded, _guards_intact, _in_nan  # noqa: F401

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DROP = (0x1234567887654321, 2, 1, 0.2)  # (seed, layer, site, p) as ops.dropout_factors takes them
EPIS = (X.EPI_NONE, X.EPI_BIAS_RES, X.EPI_BIAS_GELU, X.EPI_DGELU)
VARIANTS = X.VARIANTS
CASES = [(name, shape) for name, v in VARIANTS.items() for shape in v[2]]
IDS = [f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in CASES]
# column sums on NONE (the general epilogue's partials): one general shape per tile
NONE_COLSUM = {("TILE5_GEN", (2100, 264, 128)), ("TILE1", (3100, 2044, 384)), ("TILE2_GEN", (4000, 2040, 128))}
QUANTISED = [("TILE5_LEAN", (200, 256, 384)), ("TILE1", (3100, 2044, 384)), ("TILE2_LEAN", (4000, 2048, 384))]
IMAGE_CASES = [(n, s) for n, s in CASES if s[1] % 32 == 0]
GUARD_BYTE = 0xA5

REACHED = set()  # what the plan query has reported: ("tile", t), ("lean", l)


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


def _note(plan):
    REACHED.add(("tile", plan["tile"]))
    REACHED.add(("lean", plan["lean"]))


def _in_ff(t, pad):
    """a copy of the uint8 image t [rows, K] on the device as a view into a 0xFF parent: `pad` 0xFF bytes per row, 0xFF rows around"""
    rows, K = t.shape
    buf = torch.full((rows + 2, K + pad), 0xFF, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + rows, :K]
    view.copy_(t)
    return view


def _flat_guarded(shape, fill):
    """a contiguous uint8 tensor of `shape` inside a flat parent with 64 bytes of `fill` before and after -> (parent, view)"""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 128,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[64:64 + n].view(shape)


def _scales_in_ff(s):
    _, view = _flat_guarded(tuple(s.shape), 0xFF)
    view.copy_(s)
    return view


def _flat_intact(what, buf, fill):
    assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), what + ": a write outside the output"


_cache = {}


def _operands(ops, shape, family):
    """the images, P, magP and the device copies (dense-row and row-strided), once per (shape, data)"""
    key = (shape, family)
    if key not in _cache:
        _cache.clear()  # one entry: the cases come grouped by shape
        M, N, K = shape
        img = X.make_images(M, N, K, M * 7919 + N * 31 + K, family, quant=lambda x: ops.quant_mx8(x.cuda()))
        _cache[key] = dict(img=img, prod=X.products(img), as_=_scales_in_ff(img["as_"]), bs=_scales_in_ff(img["bs"]),
                           aq_strided=_in_ff(img["aq"], 16), bq_strided=_in_ff(img["bq"], 16),
                           aq_dense=_in_ff(img["aq"], 0), bq_dense=_in_ff(img["bq"], 0))
    return _cache[key]


_factors = {}


def _drop_factors(ops, M, N):
    if (M, N) not in _factors:
        _factors.clear()
        _factors[(M, N)] = ops.dropout_factors(*DROP, M, N).cpu()
    return _factors[(M, N)]


def _lean_code(name, epi, p, colsum, image):
    """the LEAN code the launcher must pick on this variant (nt_lean_ok / mx8_lean_exists in words)"""
    if not VARIANTS[name][1] or p or (colsum and epi != X.EPI_DGELU):
        return 0
    return 1 + (2 if colsum else 0) + (4 if image else 0)


def run(ops, name, shape, family, epi, cdt, p=0.0, colsum=False, image=False):
    """one call of gemm_mx8_ex, checked in full"""
    tile = VARIANTS[name][0]
    M, N, K = shape
    what = f"{name}{list(shape)}/{family}/{X.EPI_NAMES[epi]}/{str(cdt)[6:]}/p={p}/cs={int(colsum)}/img={int(image)}"
    op = _operands(ops, shape, family)
    inp = X.make_inputs(M, N, K, M + N + K, family, cdt, epi, op["img"])
    f = _drop_factors(ops, M, N) if p else None
    ref = X.reference(inp, f, op["prod"])
    strided = cdt == F32
    aq, bq = (op["aq_strided"], op["bq_strided"]) if strided else (op["aq_dense"], op["bq_dense"])
    assert aq.stride(0) == K + (16 if strided else 0)
    bias = None if inp["bias"] is None else _bias_in_nan(inp["bias"])
    res = None if inp["res"] is None else _in_nan(inp["res"])
    aux_in = None if inp["aux_in"] is None else _in_nan(inp["aux_in"])
    lean = _lean_code(name, epi, p, colsum, image)

    def call():
        cbuf, cview, cpre = _guarded(M, N, cdt)
        abuf = aview = apre = None
        if epi == X.EPI_BIAS_GELU:
            abuf, aview, apre = _guarded(M, N, cdt)
        qbuf = sbuf = None
        want = False
        if image:
            qbuf, qv = _flat_guarded((M, N), GUARD_BYTE)
            sbuf, sv = _flat_guarded((M, N // 32), GUARD_BYTE)
            want = (qv, sv)
        c, aux, cs, img, plan = ops.gemm_mx8_ex(aq, op["as_"], bq, op["bs"], out=cview, epilogue=epi, bias=bias, residual=res,
                                                aux=aview if epi == X.EPI_BIAS_GELU else aux_in, want_colsum=colsum,
                                                drop=DROP if p else None, want_image=want)
        torch.cuda.synchronize()
        _guards_intact(what + ":C", cbuf, cview, cpre)
        if abuf is not None:
            _guards_intact(what + ":aux", abuf, aview, apre)
        if image:
            _flat_intact(what + ":image bytes", qbuf, GUARD_BYTE)
            _flat_intact(what + ":image scales", sbuf, GUARD_BYTE)
        return c, (aux if epi == X.EPI_BIAS_GELU else None), cs, img, plan

    c, aux, cs, img, plan = call()
    _note(plan)
    assert plan == dict(tile=tile, lean=lean), (what, plan)
    assert (cs is not None) == colsum and (aux is not None) == (epi == X.EPI_BIAS_GELU) and (img is not None) == image
    c2, aux2, cs2, img2, _ = call()
    outs = (("C", c, c2), ("aux", aux, aux2), ("colsum", cs, cs2)) + \
        ((("image bytes", img[0], img2[0]), ("image scales", img[1], img2[1])) if image else ())
    for n_, x, y in outs:
        assert x is None or torch.equal(x, y), f"{what}:{n_}: a second call differs"
    for n_, x in (("C", c), ("aux", aux), ("colsum", cs)):
        assert x is None or bool(torch.isfinite(x).all()), f"{what}:{n_}: not finite (a read outside an operand?)"
    stats = X.check_outputs(what, ref, c.cpu(), None if aux is None else aux.cpu(), None if cs is None else cs.cpu())
    if family in X.EXACT_FAMILIES:
        stats["exact"] = X.check_exact(what, inp, op["prod"], c, aux, dropout=bool(p))
    if p:
        stats.update(X.mask_not_vacuous(ref))
    if image:
        if cdt == BF:  # the quantised fp32 value must be the stored one: only where check_exact has shown C to be exact
            assert family == "unit" and not p and stats["exact"] >= 1
            u = ref["C"] if epi == X.EPI_DGELU else ref["aux"]
            assert 8 <= float(u.min()) or epi == X.EPI_DGELU
            assert float(ref["C"].abs().max()) <= 256
        X.check_image(what, c.float().cpu(), img[0], img[1])
        stats["image"] = "equal"
    print("MX8STAT " + json.dumps(dict(variant=name, shape=list(shape), family=family, epi=X.EPI_NAMES[epi], c=str(cdt)[6:], p=p,
                                       tile=plan["tile"], lean=plan["lean"], **stats)))


@pytest.mark.parametrize("name,shape,epi", [(n, s, e) for n, s in CASES for e in EPIS],
                         ids=[f"{i}-{X.EPI_NAMES[e]}" for i in IDS for e in EPIS])
def test_variant(ops, name, shape, epi):
    lean_tile = VARIANTS[name][1]
    for cdt in (BF, F32):
        for p in ((0.0,) if epi == X.EPI_NONE else (0.0, DROP[3])):
            colsum = epi == X.EPI_DGELU or (epi == X.EPI_NONE and (name, shape) in NONE_COLSUM and cdt == BF)
            run(ops, name, shape, "dense-int", epi, cdt, p, colsum)
    if epi == X.EPI_NONE and (name, shape) in NONE_COLSUM:  # ... and the same shape without them
        run(ops, name, shape, "dense-int", epi, BF)
    if epi == X.EPI_DGELU and lean_tile:  # DGELU without column sums: the LEAN 1 instantiation of this epilogue
        run(ops, name, shape, "dense-int", epi, (BF, F32)[CASES.index((name, shape)) % 2])


@pytest.mark.parametrize("family", ["sparse-a", "sparse-b"])
@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_one_block_wide(ops, name, shape, family):
    """EPI_NONE over the E8M0 range, one non-zero 32-block per row of A or of B: C == P bit for bit"""
    for cdt in (BF, F32):
        run(ops, name, shape, family, X.EPI_NONE, cdt)


@pytest.mark.parametrize("name,shape", QUANTISED, ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in QUANTISED])
def test_quantised(ops, name, shape):
    """randn data through the device's quantiser, held to the stated accumulation bound 2e-3 magP per element"""
    for cdt in (BF, F32):
        run(ops, name, shape, "quantised", X.EPI_NONE, cdt)


@pytest.mark.parametrize("epi", [X.EPI_BIAS_GELU, X.EPI_DGELU], ids=["bias_gelu", "dgelu"])
@pytest.mark.parametrize("name,shape", IMAGE_CASES, ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in IMAGE_CASES])
def test_image_of_c(ops, name, shape, epi):
    """LEAN 5 (and 7: DGELU with column sums) on the lean tiles, the general epilogue's image branch elsewhere"""
    run(ops, name, shape, "dense-int", epi, F32, colsum=epi == X.EPI_DGELU, image=True)
    run(ops, name, shape, "unit", epi, BF, image=True)
    if epi == X.EPI_DGELU:  # ... and DGELU's image without the column sums (LEAN 5)
        run(ops, name, shape, "unit", epi, F32, image=True)
    if shape == (130, 160, 384):  # the general epilogue's image beside a dropout site: the masked values are what is quantised
        run(ops, name, shape, "dense-int", epi, F32, p=DROP[3], image=True)


def test_every_variant_was_reached():
    """coverage by assertion: over this file the plan query has reported every tile and every LEAN code (runs last; needs the
    tests above to have run)"""
    want = {("tile", t) for t in (1, 2, 5)} | {("lean", l) for l in (0, 1, 3, 5, 7)}
    assert want <= REACHED, sorted(want - REACHED)
