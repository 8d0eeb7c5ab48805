"""fp64 reference, element-wise bounds, cases and mutants for the data gradient of the NHWC implicit-GEMM convolution and the
backward of the NHWC average pool (csrc/conv_dgrad_kernel.hpp: conv_dgrad_nhwc_kernel; csrc/conv_dgrad.hip:
avgpool_nhwc_bwd_kernel).  The reference is CPU only: tests/test_gpu_conv_dgrad.py and tests/test_gpu_conv_dgrad_f32.py feed it
what the device returned, tests/test_conv_dgrad_ref_cpu.py anchors it to torch.autograd and shows without a device that the
bounds bite.  Built on tests/conv_util.py (out_hw, the tiles, the guarded device views) and tests/gemm_nt_util.py (the rules).

The operation, with pad = 1 for k = 3 and 0 for k = 1 and (Ho, Wo) = conv_util.out_hw(H, W, k, s) (gy rounded to bf16 first
when it is fp32, as the kernel does while staging; wt bf16):
    acc[n, iy, ix, ci] = sum over the LIVE taps (ky, kx) and co of gy[n, oy, ox, co] * wt[ci, ky, kx, co]
                         live: ty = iy + pad - ky, tx = ix + pad - kx, ty % s == 0, tx % s == 0,
                               oy = ty / s in [0, Ho), ox = tx / s in [0, Wo)
    v   = acc + addend[n, iy, ix, ci]       (optional)
    out = gate[n, iy, ix, ci] > 0 ? v : 0   (optional)
Bounds, with U = 2^-24 and the rules of tests/gemm_nt_util.py (every one a bound on |device - reference| per ELEMENT):
  accumulation  eP = 2 * K * U * mag, mag = sum |gy_bf16| |wt| over the live taps, K = k * k * Cout (the kernel adds the dead
                taps' zeros too: K counts them).
  addend        one fp32 add: U * (|v| + eP).
  gate          a select: adds nothing; where the gate is closed the output is exactly 0 (bound 0).
  bf16 output   gemm_nt_util.bf16_bound.
  parity form   the two checks of tests/conv_f32_util.py: element-wise against the exact product of the fp32 operands with
                eP = (oracle.bf16x3.PER_PRODUCT_BOUND + 2 * (3 K) * U) * mag, and relative Frobenius <= conv_f32_util.CAP = 1e-6
                against the three-term emulation (oracle.bf16x3.split).
  pool backward dout / HW is one fp32 division (or a reciprocal and a multiply): 2 U |v|; + bf16_bound for a bf16 output.

Vacuity guard (guard): a gated case has at least a quarter of its gate zero and a quarter positive; a stride-2 case has input
pixels of all four parity classes where its map has them (H, W >= 2); a stride-2 3x3 case on an even map has a tap that is on
the lattice but maps to oy == Ho or ox == Wo (dropped); N >= 2 and H * W is no multiple of the tile's rows: a tile crosses an
image boundary."""
import itertools

import torch

import conv_util as cu
from conv_util import DT, TILES, out_hw
from gemm_nt_util import U, _ratio, bf16_bound, round_to
from oracle.bf16x3 import PER_PRODUCT_BOUND, split

CAP = 1e-6  # conv_f32_util.CAP

# (N, H, W, Cin, Cout, k, stride); H, W are the INPUT map's.  Small, on the 64 x 32 tile: odd and even maps at stride 2 (on an
# even map the tap at the bottom / right edge maps to oy == Ho and must be dropped), 2x2 -> 1x1, 1x1 maps, Cout = 32 / 64 / 96
# (one, two, three chunks per tap), Cin = 16 / 48 / 144 (below, not a multiple of, above a channel tile).
SMALL_SHAPES = [
    (2, 7, 7, 16, 32, 3, 1), (3, 5, 4, 48, 64, 3, 1), (2, 7, 7, 144, 96, 3, 2), (3, 8, 6, 48, 32, 3, 2), (2, 2, 2, 16, 32, 3, 2),
    (3, 1, 1, 16, 64, 3, 1), (2, 7, 7, 144, 64, 1, 1), (3, 5, 4, 16, 96, 1, 2), (3, 8, 6, 48, 64, 1, 2), (2, 1, 1, 48, 32, 1, 1),
]
# on the 128 x 64 tile: 256 workgroups and more, ragged in M
BIG_SHAPES = [(3, 61, 61, 144, 32, 3, 1), (2, 181, 179, 80, 64, 1, 2), (3, 62, 61, 144, 96, 3, 2)]
SQUARE_SHAPE = (2, 5, 4, 32, 32, 3, 1)  # Cin == Cout: where a weight that was not transposed still fits
# gy type, out type, addend, gate: the 16 instantiations of each tile
COMBOS = list(itertools.product(("f32", "bf16"), ("f32", "bf16"), (False, True), (False, True)))
F32_COMBOS = [(False, False), (True, True), (False, True), (True, False)]  # (addend, gate) of the parity form


def expected_tile(shape):
    """conv_util.expected_tile's rule on M = N*H*W rows and Cin columns"""
    N, H, W, Cin = shape[:4]
    return 0 if -(-(N * H * W) // 128) * -(-Cin // 64) >= 256 else 1


def _case(shape, tile, gyd, od, add, gate):
    N, H, W, Cin, Cout, k, s = shape
    return dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, gy=gyd, out=od, add=add, gate=gate, shape_id=shape, tile=tile,
                id=f"{N}x{H}x{W}x{Cin}-{Cout}-k{k}s{s}-g{gyd}-o{od}-add{int(add)}-gate{int(gate)}-t{tile}")


def _cases():
    out = []
    for tile, shapes in ((1, SMALL_SHAPES), (0, BIG_SHAPES)):
        for i, (gyd, od, add, gate) in enumerate(COMBOS):
            out.append(_case(shapes[i % len(shapes)], tile, gyd, od, add, gate))
    return out


def _f32_cases():
    out = []
    for tile, shapes, n in ((1, SMALL_SHAPES, len(SMALL_SHAPES)), (0, BIG_SHAPES, 4)):
        for i in range(n):
            out.append(_case(shapes[i % len(shapes)], tile, "f32", "f32", *F32_COMBOS[i % 4]))
    return out


CASES = _cases()
F32_CASES = _f32_cases()
SQUARE_CASE = _case(SQUARE_SHAPE, 1, "f32", "f32", True, True)
# HW, C, out type, gate
POOL_CASES = [(hw, c, od, g) for hw in (16, 49, 1) for c in (16, 144) for od in ("f32", "bf16") for g in (False, True)]


# ---- the index formula ----------------------------------------------------------------------------------
def taps(N, H, W, k, s, rows=None, lattice=True, edge=True, carry_tile=0):
    """-> (flat [R, k*k]: index of gy's pixel (n, oy, ox) in [0, N*Ho*Wo) for every tap of the input pixels `rows` (all by
    default), live [R, k*k]).  lattice=False, edge=False and carry_tile are the staging mutants (see MUTANTS)."""
    pad = 1 if k == 3 else 0
    Ho, Wo = out_hw(H, W, k, s)
    m = torch.arange(N * H * W) if rows is None else rows
    n, r = m // (H * W), m % (H * W)
    iy, ix = r // W, r % W
    if carry_tile:  # (n, iy, ix) decoded at the tile's first row and carried on without wrapping into the next image
        n0 = (m // carry_tile * carry_tile) // (H * W)
        iy = iy + (n - n0) * H
        n = n0
    ky, kx = torch.arange(k).repeat_interleave(k), torch.arange(k).repeat(k)
    ty, tx = (iy + pad)[:, None] - ky[None], (ix + pad)[:, None] - kx[None]
    live = (ty >= 0) & (tx >= 0)
    if lattice:  # (dropped: ty / s is floored)
        live = live & (ty % s == 0) & (tx % s == 0)
    oy, ox = torch.div(ty, s, rounding_mode="floor"), torch.div(tx, s, rounding_mode="floor")
    if edge:     # (dropped: oy == Ho reads the next image, ox == Wo the next row)
        live = live & (oy < Ho) & (ox < Wo)
    return (n[:, None] * Ho + oy) * Wo + ox, live


def dgrad(gy, wt, H, W, k, s, rows=None, **mut):
    """-> (acc [R, Cin], mag [R, Cin], live [R, k*k]) in fp64 from gy [N, Ho, Wo, Cout] and wt [Cin, k, k, Cout]"""
    N, Cout = gy.shape[0], gy.shape[-1]
    flat, live = taps(N, H, W, k, s, rows, **mut)
    px = gy.double().reshape(-1, Cout)
    p = (px[flat % px.shape[0]] * live[..., None].double()).reshape(flat.shape[0], -1)  # (% : a mutant's address as it comes)
    wf = wt.double().reshape(wt.shape[0], -1)
    return p @ wf.t(), p.abs() @ wf.abs().t(), live


def wt_of(w, scale=None):
    """nn.Conv2d's w [Cout, Cin, k, k] (times scale[co]) -> wt [Cin, k, k, Cout]"""
    if scale is not None:
        w = w * scale.view(-1, 1, 1, 1)
    return w.permute(1, 2, 3, 0).contiguous()


def block_backward(gs, h, ws, scales, in_hw, stride, x_gate=None):
    """FrozenBasicBlock.backward_nhwc restated with dgrad: ws = (conv1.weight, conv2.weight, downsample weight or None) as
    [Cout, Cin, k, k], scales the folded BatchNorm scales; gs [N, Ho, Wo, planes], h the inner ReLU map -> dx [N, H, W, inplanes]"""
    N, (H, W) = gs.shape[0], in_hw
    Ho, Wo = h.shape[1:3]
    dh = dgrad(gs, wt_of(ws[1], scales[1]), Ho, Wo, 3, 1)[0].reshape(h.shape) * (h > 0)
    add = gs if ws[2] is None else dgrad(gs, wt_of(ws[2], scales[2]), H, W, 1, stride)[0].reshape(N, H, W, -1)
    dx = dgrad(dh, wt_of(ws[0], scales[0]), H, W, 3, stride)[0].reshape(N, H, W, -1) + add
    return dx if x_gate is None else dx * (x_gate > 0)


# ---- operands, reference, bounds ----------------------------------------------------------------------------
_OPERANDS, _PRODUCTS = {}, {}


def operands(case):
    """gy [N, Ho, Wo, Cout] fp32 (NOT bf16-exact: the kernel's rounding is part of the test), wt [Cin, k, k, Cout] scaled so that
    acc is of order 1 (wt_f32: not bf16-exact, what the parity form splits; wt = its bf16 rounding), addend fp32, gate a
    ReLU-like map with exact zeros: shared by every epilogue of a shape"""
    key = case["shape_id"]
    if key not in _OPERANDS:
        N, H, W, Cin, Cout, k, s = key
        g = torch.Generator().manual_seed(11 + cu._seed(key))
        Ho, Wo = out_hw(H, W, k, s)
        gy = torch.randn(N, Ho, Wo, Cout, generator=g)
        wt_f32 = torch.randn(Cin, k, k, Cout, generator=g) / max(k * k * Cout / (s * s), 1.0) ** 0.5
        addend = torch.randn(N, H, W, Cin, generator=g)
        gate = torch.randn(N, H, W, Cin, generator=g).clamp_min(0)
        _OPERANDS[key] = dict(gy=gy, wt_f32=wt_f32, wt=wt_f32.bfloat16(), addend=addend, gate=gate)
    return _OPERANDS[key]


def inputs(case):
    """the operands in the case's storage types (addend / gate None without one); addend and gate have out's type"""
    o = operands(case)
    return dict(gy=o["gy"].to(DT[case["gy"]]), wt=o["wt"], wt_f32=o["wt_f32"],
                addend=o["addend"].to(DT[case["out"]]) if case["add"] else None,
                gate=o["gate"].to(DT[case["out"]]) if case["gate"] else None)


def products(case):
    """acc, mag [M, Cin] in fp64 and the live map of the bf16 form: once per shape"""
    key = case["shape_id"]
    if key not in _PRODUCTS:
        o = operands(case)
        _PRODUCTS[key] = dgrad(o["gy"].bfloat16(), o["wt"], *key[1:3], *key[5:7])
    return _PRODUCTS[key]


def epilogue(case, acc, eP, addend, gate, gate_first=False, gate_ge=False):
    """-> dict(C, bC) from the products and their bound, [R, Cin]"""
    v, b = acc, eP
    open_ = None if gate is None else ((gate.double() >= 0) if gate_ge else (gate.double() > 0)).reshape(acc.shape)
    if gate_first and open_ is not None:
        v = v * open_
    if addend is not None:
        v = v + addend.double().reshape(acc.shape)
        b = b + U * (v.abs() + b)
    if open_ is not None and not gate_first:
        v, b = v * open_, b * open_
    return dict(C=v, bC=b)


def reference(case):
    acc, mag, _ = products(case)
    inp = inputs(case)
    K = case["k"] * case["k"] * case["Cout"]
    return epilogue(case, acc, 2.0 * K * U * mag, inp["addend"], inp["gate"])


def check(what, ref, got, rows=None):
    """assert got [M, Cin] (or its rows) element-wise within the bound; -> the worst error / bound ratio.  Where the gate is
    closed the bound is 0: the output must be exactly 0."""
    C, b = ref["C"], ref["bC"]
    bb = b if got.dtype == torch.float32 else torch.where(b > 0, bf16_bound(C, b), b)
    if rows is not None:
        C, bb = C[rows], bb[rows]
    r = _ratio(got.reshape(C.shape), C, bb)
    assert r <= 1.0, f"{what}: error / bound = {r}"
    return r


def ratio(got, ref, rows=None):
    C, b = ref["C"], ref["bC"]
    bb = b if got.dtype == torch.float32 else torch.where(b > 0, bf16_bound(C, b), b)
    if rows is not None:
        C, bb = C[rows], bb[rows]
    return _ratio(got.reshape(C.shape), C, bb)


def guard(case):
    """the vacuity guard of the module docstring; -> its figures"""
    N, H, W, Cin, Cout, k, s = case["shape_id"]
    out = {}
    if case["gate"]:
        g = inputs(case)["gate"]
        out["gate_zero"], out["gate_positive"] = float((g == 0).double().mean()), float((g > 0).double().mean())
        assert out["gate_zero"] >= 0.25 and out["gate_positive"] >= 0.25, out
    if s == 2:
        m = torch.arange(H * W)
        classes = set(zip(((m // W) % 2).tolist(), ((m % W) % 2).tolist()))
        out["parity_classes"] = len(classes)
        assert len(classes) == min(H, 2) * min(W, 2), out
        _, live_noedge = taps(N, H, W, k, s, edge=False)
        _, live = taps(N, H, W, k, s)
        out["dropped_edge_taps"] = int((live_noedge & ~live).sum())
        if k == 3 and (H % 2 == 0 or W % 2 == 0):
            assert out["dropped_edge_taps"] > 0, out
    _, live = taps(N, H, W, k, s)
    out["dead_taps"] = int((~live).sum())
    assert N >= 2 and (H * W) % TILES[case["tile"]][0] != 0  # a tile crosses an image boundary
    assert expected_tile(case["shape_id"]) == case["tile"]
    return out


# ---- the parity form ------------------------------------------------------------------------------------
_F32_PRODUCTS = {}


def three_terms(gy, wt, H, W, k, s, rows=None, drop=None, **mut):
    """E in fp64: hi_w lo_g + lo_w hi_g + hi_w hi_g; `drop` leaves a cross term out"""
    (gh, gl), (wh, wl) = split(gy), split(wt)
    e = dgrad(gh, wh, H, W, k, s, rows, **mut)[0]
    if drop != "lo_g_hi_w":
        e = e + dgrad(gl, wh, H, W, k, s, rows, **mut)[0]
    if drop != "hi_g_lo_w":
        e = e + dgrad(gh, wl, H, W, k, s, rows, **mut)[0]
    return e


def f32_products(case):
    """P (exact product of the fp32 operands), mag, E (three terms) in fp64: once per shape"""
    key = case["shape_id"]
    if key not in _F32_PRODUCTS:
        o = operands(case)
        P, mag, _ = dgrad(o["gy"], o["wt_f32"], *key[1:3], *key[5:7])
        _F32_PRODUCTS[key] = (P, mag, three_terms(o["gy"], o["wt_f32"], *key[1:3], *key[5:7]))
    return _F32_PRODUCTS[key]


def f32_reference(case):
    """-> (exact: dict(C, bC), emulated: C of E through the same epilogue)"""
    P, mag, E = f32_products(case)
    inp = inputs(case)
    K = case["k"] * case["k"] * case["Cout"]
    exact = epilogue(case, P, (PER_PRODUCT_BOUND + 2.0 * (3 * K) * U) * mag, inp["addend"], inp["gate"])
    return exact, epilogue(case, E, torch.zeros_like(E), inp["addend"], inp["gate"])["C"]


def rel_fro(got, want):
    got, want = got.double().reshape(want.shape), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


# ---- mutants -------------------------------------------------------------------------------------------------
# What a subtly wrong kernel would return, computed with the reference's own arithmetic on a subset of the input pixels
# (mutant_rows: the first tiles and the rows around the first image boundary).  name -> the cases it applies to.
def _even_edge(c):
    return c["s"] == 2 and c["k"] == 3 and (c["H"] % 2 == 0 or c["W"] % 2 == 0)


MUTANTS = {
    "lattice_dropped": lambda c: c["s"] == 2 and (c["k"] == 3 or c["H"] > 1 or c["W"] > 1),  # ty / stride floored, odd ty taken
    "edge_kept": _even_edge,                                       # oy < Ho dropped: the tap reads the next image or row
    "kh_kw_swapped": lambda c: c["k"] == 3 and (c["H"] > 1 or c["W"] > 1),
    "weight_not_transposed": lambda c: c["Cin"] == c["Cout"],
    "tap_dropped": lambda c: True,                                 # the centre tap (live at every pixel on the lattice) left out
    "k_chunk_skipped": lambda c: True,                             # the last 32 output channels of the centre tap skipped
    "tile_carry": lambda c: True,                                  # (iy, ix) carried across the image boundary inside a tile
    "gate_before_addend": lambda c: c["add"] and c["gate"],
    "gate_ge": lambda c: c["gate"],                                # gate >= 0 for gate > 0
}


def mutant_rows(case):
    M, b = case["N"] * case["H"] * case["W"], case["H"] * case["W"]
    r = torch.cat([torch.arange(0, min(M, 256)), torch.arange(max(b - 64, 0), min(b + 128, M))])
    return torch.unique(r)


def _mutated(case, mutant, wt):
    k, Cout = case["k"], case["Cout"]
    kw = {}
    if mutant == "lattice_dropped":
        kw["lattice"] = False
    if mutant == "edge_kept":
        kw["edge"] = False
    if mutant == "tile_carry":
        kw["carry_tile"] = TILES[case["tile"]][0]
    if mutant == "kh_kw_swapped":
        wt = wt.transpose(1, 2).contiguous()
    if mutant == "weight_not_transposed":
        wt = wt.permute(3, 1, 2, 0).contiguous()
    if mutant in ("tap_dropped", "k_chunk_skipped"):  # a zero weight is a skipped product (and splits to (0, 0))
        wt = wt.clone()
        wt[:, k // 2, k // 2, (0 if mutant == "tap_dropped" else Cout - 32):] = 0
    return wt, kw


def simulate(case, mutant=None, rows=None, f32=False):
    """-> the (mutated) output on `rows` (mutant_rows by default), rounded to the case's output type; f32: the parity form's
    three-term arithmetic on the fp32 operands"""
    rows = mutant_rows(case) if rows is None else rows
    o, inp = operands(case), inputs(case)
    N, H, W, Cin, Cout, k, s = case["shape_id"]
    wt, kw = _mutated(case, mutant, o["wt_f32"] if f32 else o["wt"])
    if f32:
        acc = three_terms(o["gy"], wt, H, W, k, s, rows, **kw)
    else:
        acc = dgrad(o["gy"].bfloat16(), wt, H, W, k, s, rows, **kw)[0]
    add = None if inp["addend"] is None else inp["addend"].reshape(-1, Cin)[rows]
    gate = None if inp["gate"] is None else inp["gate"].reshape(-1, Cin)[rows]
    r = epilogue(case, acc, torch.zeros_like(acc), add, gate, gate_first=mutant == "gate_before_addend", gate_ge=mutant == "gate_ge")
    return round_to(r["C"], DT[case["out"]])


def simulate_fp32(case, f32=False):
    """the whole output of a correct kernel with every sum in FP32: 32-deep chunks in the kernel's order (dead taps add their
    zeros), the parity form's three terms of a chunk small ones first; fp32 epilogue; rounded to the case's output type"""
    o, inp = operands(case), inputs(case)
    N, H, W, Cin, Cout, k, s = case["shape_id"]
    flat, live = taps(N, H, W, k, s)

    def patches(g):
        px = g.float().reshape(-1, Cout)
        return (px[flat % px.shape[0]] * live[..., None].float()).reshape(flat.shape[0], -1)

    if f32:
        (gh, gl), (wh, wl) = split(o["gy"]), split(o["wt_f32"])
        terms = [(patches(gl), wh.reshape(Cin, -1)), (patches(gh), wl.reshape(Cin, -1)), (patches(gh), wh.reshape(Cin, -1))]
    else:
        terms = [(patches(o["gy"].bfloat16()), o["wt"].float().reshape(Cin, -1))]
    acc = torch.zeros(flat.shape[0], Cin)
    for c in range(0, k * k * Cout, 32):
        for p, v in terms:
            acc = acc + p[:, c:c + 32] @ v[:, c:c + 32].t()
    if inp["addend"] is not None:
        acc = acc + inp["addend"].float().reshape(acc.shape)
    if inp["gate"] is not None:
        acc = torch.where(inp["gate"].float().reshape(acc.shape) > 0, acc, torch.zeros_like(acc))
    return round_to(acc.double(), DT[case["out"]])


# ---- pool backward -------------------------------------------------------------------------------------
def pool_inputs(HW, Cn, od, gate, N=3):
    g = torch.Generator().manual_seed(HW * 1000 + Cn + 5)
    dout = torch.randn(N, Cn, generator=g)
    gt = torch.randn(N, HW, Cn, generator=g).clamp_min(0).to(DT[od]) if gate else None
    return dout, gt


def pool_reference(dout, HW, gate):
    """-> (out [N, HW, C] fp64, fp32 bound)"""
    v = (dout.double() / HW)[:, None, :].expand(-1, HW, -1)
    if gate is not None:
        v = v * (gate.double() > 0)
    return v, 2 * U * v.abs()


def pool_simulate(dout, HW, gate, od, mutant=None):
    v = (dout / (HW + 1 if mutant == "avgpool_bwd_wrong_count" else HW))[:, None, :].expand(-1, HW, -1)
    if gate is not None:
        v = torch.where(gate.float() > 0, v, torch.zeros_like(v))
    return round_to(v.double(), DT[od])


def pool_check(what, got, dout, HW, gate):
    ref, b = pool_reference(dout, HW, gate)
    bb = b if got.dtype == torch.float32 else torch.where(b > 0, bf16_bound(ref, b), b)
    r = _ratio(got.reshape(ref.shape), ref, bb)
    assert r <= 1.0, f"{what}: error / bound = {r}"
    return r
