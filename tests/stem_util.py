"""fp64 reference, element-wise bounds, cases and mutants for the fused ResNet stem (csrc/stem.hip: stem_nchw_kernel).  CPU
only: tests/test_gpu_stem.py feeds it what the device returned, tests/test_stem_ref_cpu.py shows without a device that the
bounds bite.

The operation (x [N, Cin, H, W] rounded to bf16 first when it is fp32, as the kernel does while staging; w [64, Cin, 7, 7] bf16):
    P[n, cy, cx, co] = sum over ci and the taps (ky, kx) IN RANGE of x[n, ci, 2 cy - 3 + ky, 2 cx - 3 + kx] * w[co, ci, ky, kx]
    y = max(P * scale[co] + shift[co], 0)                                  (the folded eval-mode BatchNorm and the ReLU, fp32)
    out[n, py, px, co] = max of y over the window (2 py - 1 + dy, 2 px - 1 + dx), dy, dx in 0..2, INSIDE the Hc x Wc conv map
Bounds, with the rules of tests/conv_util.py (every one a bound on |device - reference| per ELEMENT):
  accumulation  eP = 2 * K * U * magP with K = 49 * Cin: the kernel's K is padded with zero weights, and a zero product is exact.
  epilogue      conv_util.epilogue: the two fp32 roundings of the multiply and the add.
  ReLU          1-Lipschitz: adds nothing.
  pool          the max is 1-Lipschitz in the sup norm: |max a - max b| <= max |a - b|, so the pooled bound is the largest conv
                bound of the window.
  bf16 output   gemm_nt_util.bf16_bound.

Vacuity guard (guard): at least 40 % of the pooled outputs are non-zero, at least 40 % of the conv pre-activations are negative,
and, where the pooled map is at least 2 x 2, each of the nine window positions is the (positive) maximum of at least one output.

The shapes: (2, 3, 112, 112) is the video frame and (2, 1, 64, 1001) the mel map of the audio stream.  Both have EVEN conv maps
(56 x 56, 32 x 501 has an odd width), and on an even axis the last pooling window ends at the last conv pixel: a kernel that lets
the conv pixel at oy == Hc or ox == Wc - computed from the zero-padded input by a tile's halo - into the max (halo_unmasked) is
INVISIBLE there: error / bound = 0 on (2, 3, 112, 112).  That is why the odd shapes are in the list: 37 x 29 (19 x 15), 30 x 45
(15 x 23), 9 x 70 (5 x 35), 7 x 5 (4 x 3), 113 x 111 (57 x 56: several tiles, ragged), 2 x 3 and 1 x 1 (the conv map is smaller
than one window)."""
import torch
from torch.nn import functional as F

import conv_util
from gemm_nt_util import U, _ratio, bf16_bound, round_to  # noqa: F401

COUT = 64
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
SHAPES = [(2, 3, 112, 112), (2, 1, 64, 1001), (3, 3, 37, 29), (2, 4, 30, 45), (3, 1, 9, 70), (2, 1, 7, 5), (2, 4, 113, 111),
          (3, 3, 2, 3), (2, 3, 1, 1)]
CASES = [dict(shape=s, x=xd, out=od, id="x".join(map(str, s)) + f"-x{xd}-o{od}")
         for s in SHAPES for xd in ("f32", "bf16") for od in ("f32", "bf16")]


def conv_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def out_hw(H, W):
    Hc, Wc = conv_hw(H, W)
    return (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


_OPERANDS = {}


def operands(shape):
    """x [N, Cin, H, W] fp32 (NOT bf16-exact: the kernel's rounding is part of the test), w [64, Cin, 7, 7] bf16 scaled so that P
    is of order 1; scale of either sign in 0.5 .. 1.5, shift = 0.5 randn: shared by every type combination of a shape"""
    if shape not in _OPERANDS:
        N, Cin, H, W = shape
        g = torch.Generator().manual_seed(conv_util._seed(shape))
        x = torch.randn(N, Cin, H, W, generator=g)
        w = (torch.randn(COUT, Cin, 7, 7, generator=g) / (49 * Cin) ** 0.5).bfloat16()
        scale = (torch.rand(COUT, generator=g) + 0.5) * (torch.randint(0, 2, (COUT,), generator=g) * 2 - 1).float()
        shift = torch.randn(COUT, generator=g) * 0.5
        _OPERANDS[shape] = dict(x=x, w=w, scale=scale, shift=shift)
    return _OPERANDS[shape]


def inputs(case):
    o = operands(case["shape"])
    return dict(x=o["x"].to(DT[case["x"]]), w=o["w"], scale=o["scale"], shift=o["shift"])


def gather(shape, xb, extra=0, wrap=False, stride_off=0, carry_rows=0):
    """-> patches [N, Hc + extra, Wc + extra, Cin * 49] fp64 of xb [N, Cin, H, W], zero where a tap leaves the image.  The
    keyword arguments are the staging mutants (see MUTANTS); extra = 1 adds the conv row / column past the map."""
    N, Cin, H, W = shape
    Hc, Wc = conv_hw(H, W)
    n = torch.arange(N).view(N, 1, 1, 1, 1, 1)
    oy = torch.arange(Hc + extra).view(1, -1, 1, 1, 1, 1)
    ox = torch.arange(Wc + extra).view(1, 1, -1, 1, 1, 1)
    ci = torch.arange(Cin).view(1, 1, 1, Cin, 1, 1)
    ky = torch.arange(7).view(1, 1, 1, 1, 7, 1)
    kx = torch.arange(7).view(1, 1, 1, 1, 1, 7)
    iy = 2 * oy - 3 + stride_off + ky
    ix = 2 * ox - 3 + stride_off + kx
    total = N * Cin * H * W
    flat_x = xb.reshape(-1)
    if carry_rows:  # the tile's image index is not advanced: image n is read at image 0's planes, carry_rows * n input rows down
        iy = iy + n * carry_rows
        flat = (ci * H + iy) * W + ix + 0 * n
        ok = (iy >= 0) & (ix >= 0) & (ix < W) & (flat < total)
    else:
        flat = ((n * Cin + ci) * H + iy) * W + ix
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W) & (n >= 0)
    flat, ok = torch.broadcast_tensors(flat, ok)
    if wrap:  # the address of an out-of-range tap is read as it comes: the neighbouring element in memory
        p = flat_x[flat % total]
    else:
        p = flat_x[flat.clamp(0, total - 1)] * ok.double()
    return p.reshape(N, Hc + extra, Wc + extra, Cin * 49)


def conv_products(shape, w=None, **kw):
    """P, magP [N, Hc(+extra), Wc(+extra), 64] in fp64"""
    o = operands(shape)
    xb = o["x"].bfloat16().double()
    wf = (o["w"] if w is None else w).double().reshape(COUT, -1)
    p = gather(shape, xb, **kw)
    return p @ wf.t(), p.abs() @ wf.abs().t()


def conv_epilogue(shape, P, magP, scale, shift):
    """conv_util.epilogue on the conv pixels: dict(C = relu(y), bC, pre = y), shaped like P"""
    case = dict(k=7, Cin=shape[1], relu=True)
    r = conv_util.epilogue(case, P.reshape(-1, COUT), magP.reshape(-1, COUT), scale, shift, None)
    return {k: v.reshape(P.shape) for k, v in r.items()}


def pool(y, start=-1, extra=0):
    """3x3 / stride 2 max over y [N, Hc + extra, Wc + extra, C], windows starting at 2 p + start, positions outside the given map
    left out; -> (pooled [N, Hp, Wp, C], flat index of the argmax inside its window, 0 .. 8)"""
    N, Hy, Wy, Cn = y.shape
    Hp, Wp = (Hy - extra - 1) // 2 + 1, (Wy - extra - 1) // 2 + 1
    t = y.permute(0, 3, 1, 2)
    lo = -start                                       # rows of -inf above / left of the map
    hi_y, hi_x = max(2 * (Hp - 1) + start + 3 - Hy, 0), max(2 * (Wp - 1) + start + 3 - Wy, 0)
    t = F.pad(t, (lo, hi_x, lo, hi_y), value=float("-inf"))
    win = t.unfold(2, 3, 2).unfold(3, 3, 2)[:, :, :Hp, :Wp]   # [N, C, Hp, Wp, 3, 3]
    m, arg = win.reshape(N, Cn, Hp, Wp, 9).max(-1)
    return m.permute(0, 2, 3, 1).contiguous(), arg.permute(0, 2, 3, 1).contiguous()


_REFERENCE = {}


def reference(shape):
    """-> dict(C [N, Hp, Wp, 64] fp64, bC its fp32 bound, pre the conv pre-activations, arg the winning window position)"""
    if shape not in _REFERENCE:
        o = operands(shape)
        P, magP = conv_products(shape)
        r = conv_epilogue(shape, P, magP, o["scale"], o["shift"])
        C, arg = pool(r["C"])
        bC, _ = pool(r["bC"])
        _REFERENCE[shape] = dict(C=C, bC=bC, pre=r["pre"], arg=arg)
    return _REFERENCE[shape]


def bound_for(ref, dtype):
    return ref["bC"] if dtype == torch.float32 else bf16_bound(ref["C"], ref["bC"])


def ratio(ref, got):
    """the worst error / bound of got [N, Hp, Wp, 64] in its own type"""
    return _ratio(got.reshape(ref["C"].shape), ref["C"], bound_for(ref, got.dtype))


def guard(shape):
    """the vacuity guard of the module docstring; -> its figures"""
    ref = reference(shape)
    out = dict(nonzero=float((ref["C"] != 0).double().mean()), negative=float((ref["pre"] < 0).double().mean()))
    assert out["nonzero"] >= 0.4 and out["negative"] >= 0.4, out
    Hp, Wp = out_hw(*shape[2:])
    if Hp >= 2 and Wp >= 2:
        out["argmax_counts"] = [int(((ref["arg"] == i) & (ref["C"] > 0)).sum()) for i in range(9)]
        assert min(out["argmax_counts"]) >= 1, out
    return out


# ------------------------------------------------------------------------------------------------
# Mutants: what a subtly wrong kernel would return, computed with the reference's own arithmetic.  name -> the shapes it
# applies to (N, Cin, H, W).
def _odd_conv_axis(s):
    Hc, Wc = conv_hw(s[2], s[3])
    return Hc % 2 == 1 or Wc % 2 == 1


MUTANTS = {
    "tap_dropped": lambda s: True,                                   # the centre tap (always in range) left out
    "ky_kx_swapped": lambda s: s[2] > 1 or s[3] > 1,                 # w[co, ci, kx, ky] for w[co, ci, ky, kx]
    "channel_order_reversed": lambda s: s[1] > 1,                    # w[co, Cin - 1 - ci]
    "scale_shift_swapped": lambda s: True,
    "pool_window_off_by_one": lambda s: min(out_hw(s[2], s[3])) >= 2,  # the window starts at 2 p instead of 2 p - 1
    "halo_unmasked": _odd_conv_axis,                                 # the conv pixel at oy == Hc / ox == Wc enters the max
    "pad_wrapped": lambda s: True,                                   # padding read as the neighbouring element in memory
    "stride_off_by_one": lambda s: True,                             # sampled at 2 oy - 3 + 1
    "image_carry": lambda s: True,                                   # tile coordinates carried across an image boundary
}
TILE = (7, 7)  # avf_stem_plan's answer, asserted on the device by tests/test_gpu_stem.py; image_carry is modelled with it

_MUTATED = {}


def simulate(shape, mutant=None):
    """-> the (mutated) output [N, Hp, Wp, 64] in fp64, before the rounding to the output type"""
    key = (shape, mutant)
    if key in _MUTATED:
        return _MUTATED[key]
    o = operands(shape)
    w, scale, shift = o["w"], o["scale"], o["shift"]
    kw, pkw = {}, {}
    if mutant == "tap_dropped":
        w = w.clone()
        w[:, :, 3, 3] = 0
    if mutant == "ky_kx_swapped":
        w = w.transpose(2, 3)
    if mutant == "channel_order_reversed":
        w = w.flip(1)
    if mutant == "scale_shift_swapped":
        scale, shift = shift, scale
    if mutant == "pad_wrapped":
        kw["wrap"] = True
    if mutant == "stride_off_by_one":
        kw["stride_off"] = 1
    if mutant == "image_carry":  # image n's tile rows continue below image 0's: 4 input rows per pooled row
        kw["carry_rows"] = 4 * TILE[0] * -(-out_hw(*shape[2:])[0] // TILE[0])
    if mutant == "halo_unmasked":
        kw["extra"] = pkw["extra"] = 1
    if mutant == "pool_window_off_by_one":
        pkw["start"] = 0
    P, magP = conv_products(shape, w=w, **kw)
    y = conv_epilogue(shape, P, magP, scale, shift)["C"]
    if mutant == "halo_unmasked":  # the extra row and column take part as they were computed
        Hy, Wy = y.shape[1:3]
        Hp, Wp = out_hw(*shape[2:])
        t = F.pad(y.permute(0, 3, 1, 2), (1, 0, 1, 0), value=float("-inf"))
        t = t[:, :, :min(Hy + 1, 2 * Hp + 1), :min(Wy + 1, 2 * Wp + 1)]
        t = F.pad(t, (0, 2 * Wp + 1 - t.shape[3], 0, 2 * Hp + 1 - t.shape[2]), value=float("-inf"))
        out = t.unfold(2, 3, 2).unfold(3, 3, 2).reshape(t.shape[0], COUT, Hp, Wp, 9).max(-1)[0].permute(0, 2, 3, 1).contiguous()
    else:
        out = pool(y, **pkw)[0]
    _MUTATED[key] = out
    return out
