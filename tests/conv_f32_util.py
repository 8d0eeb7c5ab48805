"""fp64 references, bounds, cases and mutants for the parity-mode NHWC convolution (csrc/conv_f32.hip: conv_nhwc_kernel<ConvBf16x3>).
CPU only: tests/test_gpu_conv_f32.py feeds it what the device returned, tests/test_conv_f32_ref_cpu.py shows without a device that
the two checks bite.  Built on tests/conv_util.py: its shapes, its gather (with the staging mutants), out_hw and MUTANTS.

The operation (x and w fp32, NOT bf16-exact; hi = bf16(v), lo = bf16(v - hi), oracle/bf16x3.split):
    P[m, co] = sum over the taps in range and ci of x * w                                     (the exact product)
    E[m, co] = sum of hi_w lo_x + lo_w hi_x + hi_w hi_x                                        (what the kernel computes, in fp64)
    y = . * scale[co] + shift[co],  z = y + residual (optional),  C = max(z, 0) (optional)     (one fp64 epilogue for both)

Two checks, because neither refuses every wrong kernel:
  element-wise against the exact reference.  DERIVED: per product the bf16x3 arithmetic drops lo lo and the two split residuals,
      at most oracle.bf16x3.PER_PRODUCT_BOUND = 3 * 2^-16 of |x w|; the kernel sums 3 K fp32 terms, 2 * (3 K) * U * magP with
      magP = sum |x| |w| and U = 2^-24 (the accumulation rule of conv_util with three terms per product).  So
          eP = (PER_PRODUCT_BOUND + 2 * (3 K) * U) * magP
      and it is carried through the epilogue by conv_util's rules: every fp32 multiply or add costs U * (|its exact result| + the
      bound carried into it), the carried bound scaled by |scale| through the multiply; ReLU is 1-Lipschitz.
      This refuses every indexing mutant of conv_util (a tap, a chunk, a stride, the padding, the image boundary, the epilogue's
      order).  It does NOT refuse a wrong arithmetic: a split by truncation stays at 0.02 .. 0.39 of the bound on every shape
      here, and a dropped cross term (2^-8 of each product, random in sign, so its sum grows like sqrt(K) where the bound grows
      like K) exceeds it only by 1.3 x at K = 864 - a margin that is gone at the K of layer3 and layer4 (2304, 4608).
  arithmetic cap against the emulated reference: relative Frobenius error of the final output <= CAP = 1e-6.  A condition
      placed between two sets of figures measured on the CPU from the reference arithmetic alone (test_conv_f32_ref_cpu.py
      asserts both sides with margin): fp32 simulations of the correct arithmetic - 32-deep chunks with three terms per chunk,
      or torch's own order, fp32 epilogue, with and without residual and ReLU - reach at most 1.3e-7 over the eight small
      shapes and the first big one (4.2e-7 was the largest seen over other operands when the cap was set); the arithmetic
      mutants start at 1.3e-5 (split by truncation, up to 2.5e-5) and reach 8.5e-4 .. 1.5e-3 (a cross term dropped, an operand
      rounded to bf16).  This refuses every arithmetic mutant and says nothing about the split's own error, which the first
      check bounds.  On an MI355X the kernel shows 3.8e-8 .. 2.6e-7, and 0.003 .. 0.079 of the element-wise bound.

Vacuity guard (guard): conv_util.guard's rules on these operands - a ReLU case has at least a quarter of its outputs non-zero and
at least a tenth of its pre-activations negative; a 3x3 case has a padded tap; a case whose image holds one has an interior
output pixel; N >= 2 and a tile crosses an image boundary."""
import torch

import conv_util as cu
from conv_util import U
from oracle.bf16x3 import PER_PRODUCT_BOUND, split

CAP = 1e-6
# (residual, ReLU): the four epilogue instantiations of each tile
COMBOS = [(None, False), ("f32", True), (None, True), ("f32", False)]
ARITH_MUTANTS = ("lo_x_hi_w_dropped", "hi_x_lo_w_dropped", "split_by_truncation", "x_rounded_to_bf16", "w_rounded_to_bf16")


def _cases():
    """the eight small shapes and the three big ones, the four (residual, ReLU) combinations cycled; a fourth big case (the first
    big shape again) so that each tile meets all four"""
    out = []
    for tile, shapes, n in ((1, cu.SMALL_SHAPES, 8), (0, cu.BIG_SHAPES, 4)):
        for i in range(n):
            shp = shapes[i % len(shapes)]
            N, H, W, Cin, Cout, k, s = shp
            res, relu = COMBOS[i % 4]
            c = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, res=res, relu=relu, shape_id=shp, tile=tile, x="f32", out="f32")
            c["id"] = f"{N}x{H}x{W}x{Cin}-{Cout}-k{k}s{s}-r{res}-relu{int(relu)}-t{tile}"
            out.append(c)
    return out


CASES = _cases()
_OPERANDS, _PRODUCTS = {}, {}


def operands(case):
    """as conv_util.operands, but x AND w fp32 and not bf16-exact (the kernel splits both): w scaled so that P is of order 1"""
    key = case["shape_id"]
    if key not in _OPERANDS:
        N, H, W, Cin, Cout, k, s = key
        g = torch.Generator().manual_seed(1000 + cu._seed(key))
        Ho, Wo = cu.out_hw(H, W, k, s)
        x = torch.randn(N, H, W, Cin, generator=g)
        w = torch.randn(Cout, k, k, Cin, generator=g) / (k * k * Cin) ** 0.5
        scale = (torch.rand(Cout, generator=g) + 0.5) * (torch.randint(0, 2, (Cout,), generator=g) * 2 - 1).float()
        shift = torch.randn(Cout, generator=g) * 0.5
        res = torch.randn(N, Ho, Wo, Cout, generator=g)
        _OPERANDS[key] = dict(x=x, w=w, scale=scale, shift=shift, res=res)
    return _OPERANDS[key]


def inputs(case):
    o = operands(case)
    return dict(x=o["x"], w=o["w"], scale=o["scale"], shift=o["shift"], res=None if case["res"] is None else o["res"])


def _gemm(case, x, w, rows=None, **kw):
    """gather(x) [R, K] @ w [Cout, K]^T in fp64; -> (product, patches, in_range)"""
    p, ok = cu.gather(case, x.double(), rows, **kw)
    p = p.reshape(p.shape[0], -1)
    return p @ w.double().reshape(case["Cout"], -1).t(), p, ok


def three_terms(case, x, w, rows=None, drop=None, **kw):
    """E on `rows` in fp64: hi_w lo_x + lo_w hi_x + hi_w hi_x; `drop` leaves a cross term out"""
    (xh, xl), (wh, wl) = split(x), split(w)
    e = _gemm(case, xh, wh, rows, **kw)[0]
    if drop != "lo_x_hi_w":
        e = e + _gemm(case, xl, wh, rows, **kw)[0]
    if drop != "hi_x_lo_w":
        e = e + _gemm(case, xh, wl, rows, **kw)[0]
    return e


def products(case):
    """P, magP, E [M, Cout] in fp64 and the in-range map: once per shape, shared by every epilogue"""
    key = case["shape_id"]
    if key not in _PRODUCTS:
        o = operands(case)
        P, p, ok = _gemm(case, o["x"], o["w"])
        magP = p.abs() @ o["w"].double().abs().reshape(case["Cout"], -1).t()
        _PRODUCTS[key] = (P, magP, three_terms(case, o["x"], o["w"]), ok)
    return _PRODUCTS[key]


def product_bound(case, magP):
    K = case["k"] * case["k"] * case["Cin"]
    return (PER_PRODUCT_BOUND + 2.0 * (3 * K) * U) * magP


def epilogue(case, P, eP, scale, shift, res, relu_first=False):
    """-> dict(C, bC, pre) from a product and its bound: conv_util.epilogue's rules with eP given"""
    sc, sh = scale.double(), shift.double()
    t = P * sc
    et = eP * sc.abs() + U * (t.abs() + eP * sc.abs())
    y = t + sh
    b = et + U * (y.abs() + et)
    if relu_first:
        y = y.clamp_min(0)
    if res is not None:
        y = y + res.double().reshape(y.shape)
        b = b + U * (y.abs() + b)
    return dict(C=y.clamp_min(0) if case["relu"] else y, bC=b, pre=y)


def reference(case):
    """-> (exact: dict(C, bC, pre), emulated: C of E through the same epilogue)"""
    P, magP, E, _ = products(case)
    inp = inputs(case)
    exact = epilogue(case, P, product_bound(case, magP), inp["scale"], inp["shift"], inp["res"])
    emulated = epilogue(case, E, torch.zeros_like(E), inp["scale"], inp["shift"], inp["res"])["C"]
    return exact, emulated


def ratio(got, exact, rows=None):
    """worst |got - C| / bound over the elements"""
    C, b = exact["C"], exact["bC"]
    if rows is not None:
        C, b = C[rows], b[rows]
    return cu._ratio(got.reshape(C.shape), C, b)


def rel_fro(got, want):
    got, want = got.double().reshape(want.shape), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - want).norm() / want.norm())


def guard(case):
    """the vacuity guard of the module docstring; -> its figures"""
    _, _, _, ok = products(case)
    exact, _ = reference(case)
    out = {}
    if case["relu"]:
        out["nonzero"] = float((exact["C"] != 0).double().mean())
        out["negative"] = float((exact["pre"] < 0).double().mean())
        assert out["nonzero"] >= 0.25 and out["negative"] >= 0.1, out
    Ho, Wo = cu.out_hw(case["H"], case["W"], case["k"], case["s"])
    out["padded_taps"] = int((~ok).sum())
    out["interior_pixels"] = int(ok.all(1).sum())
    if case["k"] == 3:
        assert out["padded_taps"] > 0, out
    if case["k"] == 1 or (case["H"] >= 3 and case["W"] >= 3):
        assert out["interior_pixels"] > 0, out
    assert case["N"] >= 2 and (Ho * Wo) % cu.TILES[case["tile"]][0] != 0  # a tile crosses an image boundary
    return out


# ------------------------------------------------------------------------------------------------
def simulate_index(case, mutant=None, rows=None):
    """what a kernel with an INDEXING mutant of conv_util.MUTANTS (None: a correct one) returns on `rows` (conv_util.mutant_rows
    by default): the three-term arithmetic in fp64, rounded to fp32"""
    rows = cu.mutant_rows(case) if rows is None else rows
    o, inp = operands(case), inputs(case)
    k, Cin, Cout = case["k"], case["Cin"], case["Cout"]
    kw, x, w = {}, o["x"], o["w"]
    if mutant == "pad_wrapped":
        kw["wrap"] = True
    if mutant == "stride_off_by_one":
        kw["stride_off"] = 1
    if mutant == "tile_carry":
        kw["carry_tile"] = cu.TILES[case["tile"]][0]
    if mutant == "kh_kw_swapped":
        w = w.transpose(1, 2).contiguous()
    if mutant in ("tap_dropped", "k_chunk_skipped"):  # a zero weight is a skipped product, and splits to (0, 0)
        w = w.clone()
        w[:, k // 2, k // 2, (0 if mutant == "tap_dropped" else Cin - 32):] = 0
    E = three_terms(case, x, w, rows, **kw)
    scale, shift = inp["scale"], inp["shift"]
    if mutant == "scale_shift_swapped":
        scale, shift = shift, scale
    res = None if inp["res"] is None else inp["res"].reshape(-1, Cout)[rows]
    return epilogue(case, E, torch.zeros_like(E), scale, shift, res, relu_first=mutant == "relu_before_residual")["C"].float()


def _fp32_epilogue(case, acc, inp):
    y = acc * inp["scale"] + inp["shift"]
    if inp["res"] is not None:
        y = y + inp["res"].reshape(y.shape)
    return y.clamp_min(0) if case["relu"] else y


def simulate_arith(case, mutant=None, order="chunks"):
    """the whole output of a kernel with correct indexing, every sum in FP32: `order` "chunks" = 32-deep chunks in order, the
    three terms of a chunk added to one accumulator, small ones first (the kernel's order up to the order inside an MFMA);
    "torch" = one fp32 matmul per term.  `mutant`: one of ARITH_MUTANTS or None."""
    o, inp = operands(case), inputs(case)
    x, w = o["x"], o["w"]
    if mutant == "x_rounded_to_bf16":
        x = x.bfloat16().float()
    if mutant == "w_rounded_to_bf16":
        w = w.bfloat16().float()
    if mutant == "split_by_truncation":
        def sp(v):
            hi = (v.view(torch.int32) & -65536).view(torch.float32)
            return hi, ((v - hi).view(torch.int32) & -65536).view(torch.float32)
    else:
        sp = split
    (xh, xl), (wh, wl) = sp(x), sp(w)
    Cout = case["Cout"]
    ph, pl = [cu.gather(case, t.double())[0].float().reshape(-1, case["k"] ** 2 * case["Cin"]) for t in (xh, xl)]
    wh, wl = wh.reshape(Cout, -1), wl.reshape(Cout, -1)
    terms = [(pl, wh), (ph, wl), (ph, wh)]
    if mutant == "lo_x_hi_w_dropped":
        terms.pop(0)
    if mutant == "hi_x_lo_w_dropped":
        terms.pop(1)
    acc = torch.zeros(ph.shape[0], Cout)
    if order == "torch":
        for p, v in terms:
            acc = acc + p @ v.t()
    else:
        for c in range(0, ph.shape[1], 32):
            for p, v in terms:
                acc = acc + p[:, c:c + 32] @ v[:, c:c + 32].t()
    return _fp32_epilogue(case, acc, inp)
