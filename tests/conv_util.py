"""fp64 reference, element-wise bounds, cases and mutants for the NHWC implicit-GEMM convolution and the NHWC average pool
(csrc/conv_kernel.hpp: conv_nhwc_kernel with bf16 operands; csrc/conv.hip: avgpool_nhwc_kernel).  The reference is CPU only:
tests/test_gpu_conv.py feeds it what the device returned, tests/test_conv_ref_cpu.py shows without a device that the bounds bite.
The guarded device views of the GPU tests (conv, parity conv, stem) are at the end.

The operation (x rounded to bf16 first when it is fp32, as the kernel does while staging; w bf16):
    P[m, co] = sum over the taps (ky, kx) IN RANGE and ci of x[n, oy*s - pad + ky, ox*s - pad + kx, ci] * w[co, ky, kx, ci]
    y = P * scale[co] + shift[co]          (the folded eval-mode BatchNorm, fp32)
    z = y + residual[m, co]                (optional)
    C = max(z, 0)                          (optional)
Bounds, with U = 2^-24 and the rules of tests/gemm_nt_util.py (every one a bound on |device - reference| per ELEMENT):
  accumulation  eP = 2 * K * U * magP, magP = sum |x| |w| over the taps in range, K = kh * kw * Cin.
  epilogue      every fp32 multiply or add: U * (|its exact result| + the bound carried into it), the carried bound scaled by
                |scale| through the multiply.  (An fma rounds once where this counts twice.)
  ReLU          1-Lipschitz: adds nothing.
  bf16 output   gemm_nt_util.bf16_bound (half a bf16 ulp of the largest value that can be rounded).
  avgpool       HW * U * (sum |x|) / HW  (an fp32 sum of HW terms in any order, divided)  +  2 U |mean|  (the division, or a
                reciprocal and a multiply).

Vacuity guard (guard): a ReLU case has at least a quarter of its outputs non-zero and at least a tenth of its
pre-activations negative; a 3x3 case has at least one padded tap; a case whose image holds one has at least one interior
output pixel (all taps in range).  Two kinds of case in the issue's list cannot meet "a padded tap and an interior pixel"
by construction and are exempt from that half only: 1x1 convolutions have no padding, 1x1 images have no interior."""
import itertools

import torch

from gemm_nt_util import U, _ratio, bf16_bound, round_to

TILES = {0: (128, 64), 1: (64, 32)}  # avf_conv_plan's tile ids -> (pixels, channels)
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def out_hw(H, W, k, s):
    pad = 1 if k == 3 else 0
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def expected_tile(case):
    """the dispatch rule as DESIGN.md states it: the 128 x 64 tile once its grid gives each of the 256 CUs a workgroup"""
    Ho, Wo = out_hw(case["H"], case["W"], case["k"], case["s"])
    M = case["N"] * Ho * Wo
    return 0 if -(-M // 128) * -(-case["Cout"] // 64) >= 256 else 1


# (N, H, W, Cin, Cout, k, stride).  Small shapes: 2 and 3 images (a tile crosses image boundaries), 7x7 / 5x4 / 1x1 maps
# (non-square catches H/W swaps), both kernels and strides (7 -> 4, 5 -> 3 at stride 2), Cin = 32 / 64 / 96 (one, two, three
# chunks per tap), Cout = 16 / 48 / 144 (below, not a multiple of, above a channel tile), M = 2*7*7 = 98 (no multiple of a
# tile).  They run on the 64 x 32 tile.
SMALL_SHAPES = [
    (2, 7, 7, 32, 16, 3, 1), (3, 5, 4, 64, 48, 3, 1), (2, 7, 7, 96, 144, 3, 2), (3, 5, 4, 32, 48, 3, 2),
    (3, 1, 1, 64, 16, 3, 1), (2, 7, 7, 64, 144, 1, 1), (3, 5, 4, 96, 16, 1, 2), (2, 1, 1, 32, 48, 1, 1),
]
# The 128 x 64 tile runs from 256 workgroups on, so its cases are the smallest with that many: ragged in M (11163 = 87 * 128 +
# 27: also "M above two M tiles of the largest tile"), Cout = 144 / 80 (a channel tile with 16 live columns), every kernel /
# stride, non-square.
BIG_SHAPES = [(3, 61, 61, 32, 144, 3, 1), (2, 181, 179, 64, 80, 1, 2), (3, 123, 121, 96, 144, 3, 2)]
# x type, out type, residual type, ReLU: the 24 epilogue instantiations of each tile
COMBOS = list(itertools.product(("f32", "bf16"), ("f32", "bf16"), (None, "f32", "bf16"), (False, True)))


def _cases():
    out = []
    for shapes in (SMALL_SHAPES, BIG_SHAPES):
        for i, (xd, od, rd, relu) in enumerate(COMBOS):
            N, H, W, Cin, Cout, k, s = shapes[i % len(shapes)]
            c = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, x=xd, out=od, res=rd, relu=relu, shape_id=shapes[i % len(shapes)])
            c["tile"] = 0 if shapes is BIG_SHAPES else 1
            c["id"] = f"{N}x{H}x{W}x{Cin}-{Cout}-k{k}s{s}-x{xd}-o{od}-r{rd}-relu{int(relu)}-t{c['tile']}"
            out.append(c)
    # the remaining small shapes meet every kernel / stride with a residual and a ReLU too
    for j, shp in enumerate(SMALL_SHAPES):
        N, H, W, Cin, Cout, k, s = shp
        xd, od, rd = ("bf16", "f32")[j % 2], ("bf16", "f32")[(j // 2) % 2], ("bf16", "f32")[(j // 4) % 2]
        c = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, x=xd, out=od, res=rd, relu=True, shape_id=shp, tile=1)
        c["id"] = f"{N}x{H}x{W}x{Cin}-{Cout}-k{k}s{s}-x{xd}-o{od}-r{rd}-relu1-t1-block"
        out.append(c)
    return out


CASES = _cases()
# HW, C, x type
POOL_CASES = [(hw, c, xd) for hw in (16, 49, 1) for c in (16, 144) for xd in ("f32", "bf16")]


def _seed(shape_id):
    return 7 + sum((i + 1) * v for i, v in enumerate(shape_id))


_OPERANDS = {}


def operands(case):
    """x [N, H, W, Cin] fp32 (NOT bf16-exact: the kernel's rounding is part of the test), w [Cout, k, k, Cin] bf16 scaled so
    that P is of order 1; scale of either sign in 0.5 .. 1.5, shift, residual fp32: shared by every epilogue of a shape"""
    key = case["shape_id"]
    if key not in _OPERANDS:
        N, H, W, Cin, Cout, k, s = key
        g = torch.Generator().manual_seed(_seed(key))
        Ho, Wo = out_hw(H, W, k, s)
        x = torch.randn(N, H, W, Cin, generator=g)
        w = (torch.randn(Cout, k, k, Cin, generator=g) / (k * k * Cin) ** 0.5).bfloat16()
        scale = (torch.rand(Cout, generator=g) + 0.5) * (torch.randint(0, 2, (Cout,), generator=g) * 2 - 1).float()
        shift = torch.randn(Cout, generator=g) * 0.5
        res = torch.randn(N, Ho, Wo, Cout, generator=g)
        _OPERANDS[key] = dict(x=x, w=w, scale=scale, shift=shift, res=res)
    return _OPERANDS[key]


def inputs(case):
    """the operands in the case's storage types (residual None without one)"""
    o = operands(case)
    return dict(x=o["x"].to(DT[case["x"]]), w=o["w"], scale=o["scale"], shift=o["shift"],
                res=None if case["res"] is None else o["res"].to(DT[case["res"]]))


def gather(case, xb, rows=None, wrap=False, stride_off=0, carry_tile=0):
    """-> (patches [R, k*k, Cin] fp64 with zeros where a tap is padding, in_range [R, k*k]) for the output pixels `rows`
    (all by default) of xb [N, H, W, Cin] fp64.  The keyword arguments are the staging mutants (see MUTANTS)."""
    N, H, W, Cin, k, s = case["N"], case["H"], case["W"], case["Cin"], case["k"], case["s"]
    pad = 1 if k == 3 else 0
    Ho, Wo = out_hw(H, W, k, s)
    m = torch.arange(N * Ho * Wo) if rows is None else rows
    n, r = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = r // Wo, r % Wo
    if carry_tile:  # (n, oy, ox) decoded at the tile's first row and carried on without wrapping into the next image
        n0 = (m // carry_tile * carry_tile) // (Ho * Wo)
        oy = oy + (n - n0) * Ho
        n = n0
    ky, kx = torch.arange(k).repeat_interleave(k), torch.arange(k).repeat(k)
    iy = (oy * s - pad + stride_off)[:, None] + ky[None]
    ix = (ox * s - pad + stride_off)[:, None] + kx[None]
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    flat = (n[:, None] * H + iy) * W + ix
    px = xb.reshape(N * H * W, Cin)
    if wrap:  # the address of the out-of-range tap is read as it comes: the neighbouring pixel in memory
        return px[flat % (N * H * W)], ok
    return px[flat.clamp(0, N * H * W - 1)] * ok[..., None].double(), ok


_PRODUCTS = {}


def products(case):
    """P, magP [M, Cout] in fp64 and the in-range map: once per shape, shared by every epilogue"""
    key = case["shape_id"]
    if key not in _PRODUCTS:
        o = operands(case)
        xb = o["x"].bfloat16().double()
        p, ok = gather(case, xb)
        wf = o["w"].double().reshape(case["Cout"], -1)
        P = p.reshape(p.shape[0], -1) @ wf.t()
        magP = p.abs().reshape(p.shape[0], -1) @ wf.abs().t()
        _PRODUCTS[key] = (P, magP, ok)
    return _PRODUCTS[key]


def epilogue(case, P, magP, scale, shift, res, relu_first=False):
    """-> dict(C, bC, pre) from the products: the reference and its fp32 bound, [M, Cout]"""
    K = case["k"] * case["k"] * case["Cin"]
    sc, sh = scale.double(), shift.double()
    eP = 2.0 * K * U * magP
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
    P, magP, _ = products(case)
    inp = inputs(case)
    return epilogue(case, P, magP, inp["scale"], inp["shift"], inp["res"])


def bound_for(ref, dtype):
    return ref["bC"] if dtype == torch.float32 else bf16_bound(ref["C"], ref["bC"])


def check(what, ref, got, rows=None):
    """assert got [M, Cout] (or its rows) element-wise within the bound; -> the worst error / bound ratio"""
    C, b = ref["C"], bound_for(ref, got.dtype)
    if rows is not None:
        C, b = C[rows], b[rows]
    r = _ratio(got.reshape(C.shape), C, b)
    assert r <= 1.0, f"{what}: error / bound = {r}"
    return r


def guard(case):
    """the vacuity guard of the module docstring; -> its figures"""
    P, _, ok = products(case)
    ref = reference(case)
    out = {}
    if case["relu"]:
        out["nonzero"] = float((ref["C"] != 0).double().mean())
        out["negative"] = float((ref["pre"] < 0).double().mean())
        assert out["nonzero"] >= 0.25 and out["negative"] >= 0.1, out
    Ho, Wo = out_hw(case["H"], case["W"], case["k"], case["s"])
    out["padded_taps"] = int((~ok).sum())
    out["interior_pixels"] = int(ok.all(1).sum())
    if case["k"] == 3:
        assert out["padded_taps"] > 0, out
    if case["k"] == 1 or (case["H"] >= 3 and case["W"] >= 3):
        assert out["interior_pixels"] > 0, out
    assert case["N"] >= 2 and (Ho * Wo) % TILES[case["tile"]][0] != 0  # a tile crosses an image boundary
    return out


# ------------------------------------------------------------------------------------------------
# Mutants: what a subtly wrong kernel would return, computed with the reference's own arithmetic on a subset of the output
# pixels (mutant_rows: the first tiles and the rows around the first image boundary - a border, an interior and a tile that
# crosses into the next image are all there).  name -> the cases it applies to.
MUTANTS = {
    "tap_dropped": lambda c: True,                               # the centre tap (always in range) left out
    "kh_kw_swapped": lambda c: c["k"] == 3 and (c["H"] > 1 or c["W"] > 1),  # w[co, kx, ky] for w[co, ky, kx]
    "pad_wrapped": lambda c: c["k"] == 3,                        # padding read as the neighbouring pixel in memory
    "stride_off_by_one": lambda c: c["s"] == 2,                  # sampled at oy * 2 - pad + 1
    "tile_carry": lambda c: True,                                # (oy, ox) carried across the image boundary inside a tile
    "scale_shift_swapped": lambda c: True,
    "relu_before_residual": lambda c: c["relu"] and c["res"] is not None,
    "k_chunk_skipped": lambda c: True,                           # the last 32 channels of the centre tap skipped
}


def mutant_rows(case):
    Ho, Wo = out_hw(case["H"], case["W"], case["k"], case["s"])
    M, b = case["N"] * Ho * Wo, Ho * Wo
    r = torch.cat([torch.arange(0, min(M, 256)), torch.arange(max(b - 64, 0), min(b + 128, M))])
    return torch.unique(r)


def simulate(case, mutant=None, rows=None):
    """-> the (mutated) output on `rows` (mutant_rows by default), rounded to the case's output type"""
    rows = mutant_rows(case) if rows is None else rows
    o, inp = operands(case), inputs(case)
    k, Cin, Cout = case["k"], case["Cin"], case["Cout"]
    xb = o["x"].bfloat16().double()
    w = o["w"].double()
    kw = {}
    if mutant == "pad_wrapped":
        kw["wrap"] = True
    if mutant == "stride_off_by_one":
        kw["stride_off"] = 1
    if mutant == "tile_carry":
        kw["carry_tile"] = TILES[case["tile"]][0]
    p, _ = gather(case, xb, rows, **kw)
    if mutant == "kh_kw_swapped":
        w = w.transpose(1, 2)
    if mutant == "tap_dropped":
        p = p.clone()
        p[:, (k * k) // 2] = 0
    if mutant == "k_chunk_skipped":
        p = p.clone()
        p[:, (k * k) // 2, Cin - 32:] = 0
    wf = w.reshape(Cout, -1)
    P = p.reshape(len(rows), -1) @ wf.t()
    magP = p.abs().reshape(len(rows), -1) @ wf.abs().t()
    scale, shift = inp["scale"], inp["shift"]
    if mutant == "scale_shift_swapped":
        scale, shift = shift, scale
    res = None if inp["res"] is None else inp["res"].reshape(-1, Cout)[rows]
    r = epilogue(case, P, magP, scale, shift, res, relu_first=mutant == "relu_before_residual")
    return round_to(r["C"], DT[case["out"]])


# ------------------------------------------------------------------------------------------------
def pool_inputs(HW, Cn, xd, N=3):
    g = torch.Generator().manual_seed(HW * 1000 + Cn)
    return (torch.randn(N, HW, Cn, generator=g) + 0.25).to(DT[xd])


def pool_reference(x):
    """-> (mean [N, C] fp64, bound)"""
    xd = x.double()
    HW = x.shape[1]
    mean = xd.mean(1)
    return mean, HW * U * xd.abs().sum(1) / HW + 2 * U * mean.abs()


def pool_simulate(x, mutant=None):
    HW = x.shape[1]
    return (x.double().sum(1) / (HW + 1 if mutant == "avgpool_wrong_count" else HW)).float()


# ---- guarded device operands of the GPU tests -------------------------------------------------------
SENTINEL = -24576.0  # exact in bf16
GUARD = 64           # elements either side: keeps every unshifted view 16-byte aligned in both types


def _inside(t, fill, shift=0):
    """a device copy of t as a view into a parent that holds `fill` on both sides, starting `shift` elements further in"""
    buf = torch.full((t.numel() + 2 * GUARD + shift,), fill, dtype=t.dtype, device="cuda")
    view = buf[GUARD + shift:GUARD + shift + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _intact(what, buf, n):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), what + ": a write outside the output"
