"""fp64 reference, cases and mutants for the SECOND pool geometry of the fused ResNet stem (csrc/stem.hip, AVF_STEM_POOL_CEIL:
maxpool 3x3 / 2 / pad 0 with ceil_mode, the stem of the VGGFace2 ResNet-50), built on tests/stem_util.py: its operands, gather,
epilogue, element-wise bounds and ``pool(..., start=0)``.  CPU only: tests/test_gpu_stem_pool.py feeds it what the device
returned, tests/test_stem_pool_ref_cpu.py shows without a device that it is torch's stem and that the bounds bite.

The operation differs from stem_util's in the pool alone:
    out[n, py, px, co] = max of y over the window (2 py + dy, 2 px + dx), dy, dx in 0..2, INSIDE the Hc x Wc conv map
    Hp = ceil((Hc - 3) / 2) + 1 = (Hc - 2) // 2 + 1, the same for W (torch's max_pool2d; Hc, Wc >= 2, i.e. H, W >= 3)
so the bounds are stem_util's (the max is 1-Lipschitz in the sup norm: the pooled bound is the largest conv bound of the window).

On an EVEN conv axis the last window starts at Hc - 2 and hangs one pixel over the edge of the map: there the conv pixel at
oy == Hc / ox == Wc, which a tile computes from the zero-padded input, must stay out of the max (``halo_unmasked``) - the opposite
of the pad-1 geometry, where that mutant shows on ODD axes only and is invisible on the 112 x 112 video frame.  On an odd axis the
last window ends at the last conv pixel.

The shapes: (2, 3, 112, 112) the video frame (56 x 56: several tiles, a partial last window), (3, 3, 37, 29) (19 x 15, odd maps),
(2, 4, 30, 45) (15 x 23), (2, 1, 7, 5) (4 x 3 -> 2 x 1), (2, 4, 113, 111) (57 x 56: ragged tiles), (3, 3, 3, 4) (2 x 2 -> one
output, from a partial window)."""
import torch

import stem_util as su

COUT = su.COUT
DT = su.DT
SHAPES = [(2, 3, 112, 112), (3, 3, 37, 29), (2, 4, 30, 45), (2, 1, 7, 5), (2, 4, 113, 111), (3, 3, 3, 4)]
CASES = [dict(shape=s, x=xd, out=od, id="x".join(map(str, s)) + f"-x{xd}-o{od}")
         for s in SHAPES for xd in ("f32", "bf16") for od in ("f32", "bf16")]
inputs = su.inputs
ratio = su.ratio


def pooled(L):
    """torch's max_pool2d(3, 2, padding=0, ceil_mode=True) output length of a conv axis of L >= 2 pixels"""
    return (L - 2) // 2 + 1


def out_hw(H, W):
    Hc, Wc = su.conv_hw(H, W)
    return pooled(Hc), pooled(Wc)


def pool_ceil(y):
    """y [N, Hc, Wc, C] -> (pooled [N, Hp, Wp, C], argmax): stem_util.pool with windows from 2 p.  On an odd axis it also makes a
    window that starts at the last pixel, which torch's size rule does not have: cut to Hp x Wp"""
    Hp, Wp = pooled(y.shape[1]), pooled(y.shape[2])
    m, arg = su.pool(y, start=0)
    return m[:, :Hp, :Wp].contiguous(), arg[:, :Hp, :Wp].contiguous()


_REFERENCE = {}


def reference(shape):
    """-> dict(C [N, Hp, Wp, 64] fp64, bC its fp32 bound, pre the conv pre-activations, arg the winning window position)"""
    if shape not in _REFERENCE:
        o = su.operands(shape)
        P, magP = su.conv_products(shape)
        r = su.conv_epilogue(shape, P, magP, o["scale"], o["shift"])
        C, arg = pool_ceil(r["C"])
        bC, _ = pool_ceil(r["bC"])
        _REFERENCE[shape] = dict(C=C, bC=bC, pre=r["pre"], arg=arg)
    return _REFERENCE[shape]


def guard(shape):
    """not vacuous: at least 40 % of the pooled outputs are non-zero and at least 40 % of the conv pre-activations negative"""
    ref = reference(shape)
    out = dict(nonzero=float((ref["C"] != 0).double().mean()), negative=float((ref["pre"] < 0).double().mean()))
    assert out["nonzero"] >= 0.4 and out["negative"] >= 0.4, out
    return out


# ------------------------------------------------------------------------------------------------
# Mutants: what a kernel that got the new geometry subtly wrong would return.  name -> the shapes it can show on.
def _even_conv_axis(s):
    Hc, Wc = su.conv_hw(s[2], s[3])
    return Hc % 2 == 0 or Wc % 2 == 0


MUTANTS = {
    # the pad-1 origin kept: windows start at 2 p - 1 (a conv map of 2 x 2 lies inside the first window from either origin)
    "window_from_minus_one": lambda s: max(su.conv_hw(s[2], s[3])) > 2,
    "floor_size": _even_conv_axis,             # Hp = (Hc - 3) // 2 + 1: the partial last window's outputs are never written
    "halo_unmasked": _even_conv_axis,          # the conv pixel at oy == Hc / ox == Wc enters the max
}


def simulate(shape, mutant=None):
    """-> the (mutated) output [N, Hp, Wp, 64] in fp64, before the rounding to the output type"""
    o = su.operands(shape)
    Hp, Wp = out_hw(*shape[2:])
    extra = 1 if mutant == "halo_unmasked" else 0
    P, magP = su.conv_products(shape, extra=extra)
    y = su.conv_epilogue(shape, P, magP, o["scale"], o["shift"])["C"]
    if mutant == "window_from_minus_one":
        return su.pool(y, start=-1)[0][:, :Hp, :Wp].contiguous()
    if mutant == "halo_unmasked":  # the extra row and column take part as they were computed; every window ends at or before them
        return su.pool(y, start=0)[0][:, :Hp, :Wp].contiguous()
    out = pool_ceil(y)[0]
    if mutant == "floor_size":     # what is not written keeps the zeros the buffer is modelled with
        Hc, Wc = su.conv_hw(*shape[2:])
        Hf, Wf = max((Hc - 3) // 2 + 1, 0), max((Wc - 3) // 2 + 1, 0)
        kept = torch.zeros_like(out)
        kept[:, :Hf, :Wf] = out[:, :Hf, :Wf]
        return kept
    return out
