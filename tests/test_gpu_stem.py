"""-m gpu: the fused ResNet stem of csrc/stem.hip (conv 7x7 / 2 -> folded BatchNorm -> ReLU -> maxpool 3x3 / 2, NCHW planes in,
NHWC out) at the operator level, element by element against the fp64 reference of tests/stem_util.py (bounds, shapes and their
reasons: that module; tests/test_stem_ref_cpu.py shows without a device that the bounds refuse every mutant).  Reached through
ops.stem_nchw / avf_stem_nchw; the tile comes from avf_stem_plan, and the file asserts with it that a case has two or more tiles
with a ragged last one along each axis.

x is a view at an ODD element offset inside a NaN-filled buffer (a read outside x poisons the output; the kernel asks for element
alignment only), w / scale / shift sit between NaNs too, the output between sentinels that must be intact afterwards.  A second
call returns the same bits.  Each run prints a line "STEMSTAT {json}" with its worst error / bound ratio.

Worst error / bound ratios measured on an MI355X over the whole file: 0.028 with an fp32 output, 0.997 with a bf16 output (by
construction: some element sits at a rounding tie, where a correct round-to-nearest errs by the half ulp that is the bound)."""
import json

import pytest
import torch

import stem_util as su
from conv_util import GUARD, SENTINEL, _inside

pytestmark = pytest.mark.gpu

ODD = 3              # x starts this many elements further in


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


def _packed(ops, inp):
    """the packed image of the case's bf16 weights with scale / shift passed through the fold: gamma = scale, beta = shift,
    mean = 0, var = 1, eps = 0 (scale / sqrt(1) and shift - 0 are exact)"""
    one, zero = torch.ones(su.COUT), torch.zeros(su.COUT)
    wp, sc, sh = ops.stem_pack_weight(*[t.cuda() for t in (inp["w"].float(), inp["scale"], inp["shift"], zero, one)], eps=0.0)
    assert torch.equal(sc.cpu(), inp["scale"]) and torch.equal(sh.cpu(), inp["shift"])
    return wp, sc, sh


@pytest.mark.parametrize("case", su.CASES, ids=[c["id"] for c in su.CASES])
def test_stem_matches_fp64_reference(ops, case):
    N, Cin, H, W = case["shape"]
    plan = ops.stem_plan(N, Cin, H, W)
    assert (plan["tile_h"], plan["tile_w"]) == su.TILE, plan
    inp = su.inputs(case)
    Hp, Wp = su.out_hw(H, W)
    nan = float("nan")
    wp, sc, sh = _packed(ops, inp)
    _, x = _inside(inp["x"], nan, shift=ODD)
    assert (x.data_ptr() // x.element_size()) % 2 == 1
    _, wp = _inside(wp.cpu(), nan)
    _, sc = _inside(sc.cpu(), nan)
    _, sh = _inside(sh.cpu(), nan)
    obuf, out = _inside(torch.full((N, Hp, Wp, su.COUT), SENTINEL, dtype=su.DT[case["out"]]), SENTINEL)
    got = ops.stem_nchw(x, wp, sc, sh, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.clone()
    n = out.numel()
    assert bool((obuf[:GUARD] == SENTINEL).all()) and bool((obuf[GUARD + n:] == SENTINEL).all()), "a write outside the output"
    ref = su.reference(case["shape"])
    ratio = su.ratio(ref, out.cpu())
    print("STEMSTAT " + json.dumps(dict(case=case["id"], ratio=round(ratio, 4))))
    assert ratio <= 1.0, f"{case['id']}: error / bound = {ratio}"
    ops.stem_nchw(x, wp, sc, sh, out=out)
    bits = torch.int16 if out.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(out.view(bits), first.view(bits)), "a second call differs"


def test_a_case_has_several_tiles_and_a_ragged_last_tile_on_each_axis(ops):
    found = []
    for N, Cin, H, W in su.SHAPES:
        p = ops.stem_plan(N, Cin, H, W)
        Hp, Wp = su.out_hw(H, W)
        if Hp > p["tile_h"] and Wp > p["tile_w"] and Hp % p["tile_h"] and Wp % p["tile_w"]:
            found.append((N, Cin, H, W))
    assert found, "no shape has two or more tiles with a ragged last tile along each axis"


def test_pack_weight_image_and_folded_batchnorm(ops):
    g = torch.Generator().manual_seed(13)
    for Cin in (1, 3, 4):
        kp = ops.stem_packed_k(Cin)
        assert kp % 32 == 0 and kp >= 49 * Cin
        w = torch.randn(64, Cin, 7, 7, generator=g)
        gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
        mean, var, eps = torch.randn(64, generator=g), torch.rand(64, generator=g) + 0.01, 1e-5
        wp, scale, shift = ops.stem_pack_weight(*[t.cuda() for t in (w, gamma, beta, mean, var)], eps)
        assert wp.dtype == torch.bfloat16 and tuple(wp.shape) == (64, kp)
        # whatever the order: every weight once, RNE, and zeros in the padding
        a = wp.cpu().float()
        for co in (0, 17, 63):
            want = torch.cat([w[co].reshape(-1).bfloat16().float(), torch.zeros(kp - 49 * Cin)]).sort()[0]
            assert torch.equal(a[co].sort()[0], want)
        sc = gamma.double() / torch.sqrt(var.double() + eps)
        sh = beta.double() - mean.double() * sc
        assert bool(((scale.cpu().double() - sc).abs() <= su.U * sc.abs() * (1 + 1e-6)).all())
        assert bool(((shift.cpu().double() - sh).abs() <= su.U * sh.abs() + 2.0 ** -50 * (beta.abs() + (mean * sc).abs())).all())
    assert ops.stem_packed_k(1) != ops.stem_packed_k(3)


def test_argument_errors_come_back_as_errors(ops):
    def pack(Cout=64, Cin=3):
        o = torch.ones(Cout, device="cuda")
        return ops.stem_pack_weight(torch.zeros(Cout, Cin, 7, 7, device="cuda"), o, o.clone(), o.clone(), o.clone())

    wp, sc, sh = pack()
    ops.stem_nchw(torch.zeros(2, 3, 9, 8, device="cuda"), wp, sc, sh)
    with pytest.raises(RuntimeError, match="1, 3 or 4 input channels"):
        pack(Cin=2)
    with pytest.raises(RuntimeError, match="writes 64 channels"):
        pack(Cout=32)
    with pytest.raises(RuntimeError, match="1, 3 or 4 input channels"):
        ops.stem_nchw(torch.zeros(2, 2, 9, 8, device="cuda"), wp, sc, sh)
    with pytest.raises(RuntimeError, match="1, 3 or 4 input channels"):
        ops.stem_plan(2, 2, 9, 8)
    with pytest.raises(RuntimeError, match="1, 3 or 4 input channels"):
        ops.stem_packed_k(5)
    # fp32 x [1, 3, 16, 16] = 768 floats and an fp32 out [1, 4, 4, 64] = 1024 floats that starts inside it
    buf = torch.zeros(2048, device="cuda")
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.stem_nchw(buf[:768].view(1, 3, 16, 16), wp, sc, sh, out=buf[512:1536].view(1, 4, 4, 64))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.stem_nchw(torch.zeros(1, 3, 16, 16, device="cuda"), wp, sc, sh, out=buf[1:1025].view(1, 4, 4, 64))
    torch.cuda.synchronize()
