"""-m gpu: the parity-mode NHWC convolution of csrc/conv_f32.hip at the operator level, against the two fp64 references of
tests/conv_f32_util.py (bounds, cases and their reasons: that module; tests/test_conv_f32_ref_cpu.py shows without a device that
the element-wise bound refuses every indexing mutant and the 1e-6 cap every arithmetic mutant).  Reached through
avf_conv2d_nhwc_f32x3; every case first asserts with avf_conv_plan - the launcher's own decision - the tile it names, and the
file as a whole that both tiles and all 8 (tile, residual, ReLU) instantiations were run.

Every operand is a view into a larger allocation: NaN around x, both weight images, scale, shift and the residual (a read outside
an operand poisons the output), a sentinel around the output that must be intact afterwards.  A second call returns the same
bits.  Each run prints a line "CONVF32STAT {json}" with its worst error / bound ratio against the exact product and its relative
Frobenius error against the emulated bf16x3 product."""
import json

import pytest
import torch

import conv_f32_util as fu
import conv_util as cu
from conv_util import GUARD, SENTINEL, _inside
from oracle.bf16x3 import split

pytestmark = pytest.mark.gpu

REACHED = set()


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


@pytest.mark.parametrize("case", fu.CASES, ids=[c["id"] for c in fu.CASES])
def test_conv_f32_matches_both_fp64_references(ops, case):
    N, H, W, Cin, Cout, k, s = case["shape_id"]
    plan = ops.conv_plan(N, H, W, Cin, Cout, k, s)
    assert plan["tile"] == case["tile"] and (plan["tile_m"], plan["tile_n"]) == cu.TILES[case["tile"]], plan
    inp = fu.inputs(case)
    Ho, Wo = cu.out_hw(H, W, k, s)
    nan = float("nan")
    w_hi, w_lo = [t.reshape(Cout, -1).bfloat16() for t in split(inp["w"])]  # exact: both pieces hold bf16 values
    _, x = _inside(inp["x"], nan)
    _, w_hi = _inside(w_hi, nan)
    _, w_lo = _inside(w_lo, nan)
    _, scale = _inside(inp["scale"], nan)
    _, shift = _inside(inp["shift"], nan)
    res = None if inp["res"] is None else _inside(inp["res"], nan)[1]
    obuf, out = _inside(torch.full((N, Ho, Wo, Cout), SENTINEL), SENTINEL)
    got = ops.conv2d_nhwc_f32(x, (w_hi, w_lo), scale, shift, k, s, residual=res, relu=case["relu"], out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.clone()
    n = out.numel()
    assert bool((obuf[:GUARD] == SENTINEL).all()) and bool((obuf[GUARD + n:] == SENTINEL).all()), "a write outside the output"
    exact, emulated = fu.reference(case)
    host = out.cpu().reshape(-1, Cout)
    ratio, err = fu.ratio(host, exact), fu.rel_fro(host, emulated)
    print("CONVF32STAT " + json.dumps(dict(case=case["id"], ratio=round(ratio, 4), rel_fro_emulated=float(f"{err:.3e}"))))
    assert ratio <= 1.0, f"{case['id']}: error / bound = {ratio}"
    assert err <= fu.CAP, f"{case['id']}: relative Frobenius error against the bf16x3 emulation {err}"
    ops.conv2d_nhwc_f32(x, (w_hi, w_lo), scale, shift, k, s, residual=res, relu=case["relu"], out=out)
    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), "a second call differs"
    REACHED.add((plan["tile"], case["res"], case["relu"]))


def test_every_tile_and_instantiation_was_reached():
    want = {(t, r, a) for t in (0, 1) for r, a in fu.COMBOS}
    assert REACHED == want and len(want) == 8, sorted(want - REACHED, key=str)


def test_pack_weight_split_layout_and_folded_batchnorm(ops):
    g = torch.Generator().manual_seed(11)
    for Cout, Cin, k in ((48, 32, 3), (16, 96, 1)):
        w = torch.randn(Cout, Cin, k, k, generator=g)
        gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
        mean, var, eps = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.01, 1e-5
        (w_hi, w_lo), scale, shift = ops.conv_pack_weight_f32(*[t.cuda() for t in (w, gamma, beta, mean, var)], eps)
        hi, lo = split(w.permute(0, 2, 3, 1).reshape(Cout, -1))
        for got, want in ((w_hi, hi), (w_lo, lo)):
            assert got.dtype == torch.bfloat16 and tuple(got.shape) == (Cout, k * k * Cin)
            assert torch.equal(got.cpu().view(torch.int16), want.bfloat16().view(torch.int16))
        assert float(lo.abs().max()) > 0
        sc = gamma.double() / torch.sqrt(var.double() + eps)
        sh = beta.double() - mean.double() * sc
        # fp64 arithmetic, then one rounding to fp32: U relative, plus the fp64 round-off of the cancelling difference
        assert bool(((scale.cpu().double() - sc).abs() <= cu.U * sc.abs() * (1 + 1e-6)).all())
        assert bool(((shift.cpu().double() - sh).abs() <= cu.U * sh.abs() + 2.0 ** -50 * (beta.abs() + (mean * sc).abs())).all())


def test_argument_errors_come_back_as_errors(ops):
    def conv(N=2, H=5, W=4, Cin=32, Cout=16, k=3, s=1, out=None, xt=None):
        x = torch.zeros(N, H, W, Cin, device="cuda") if xt is None else xt
        w = torch.zeros(Cout, k * k * Cin, dtype=torch.bfloat16, device="cuda")
        sc = torch.ones(Cout, device="cuda")
        return ops.conv2d_nhwc_f32(x, (w, w.clone()), sc, sc.clone(), k, s, out=out)

    conv()
    with pytest.raises(RuntimeError, match=r"Cin % 32 == 0"):
        conv(Cin=48)
    with pytest.raises(RuntimeError, match=r"Cout % 16 == 0"):
        conv(Cout=24)
    with pytest.raises(RuntimeError, match="kernel size 5"):
        conv(k=5, H=7, W=7)
    with pytest.raises(RuntimeError, match="stride 3"):
        conv(s=3)
    buf = torch.zeros(2 * 5 * 4 * 32 + 64, device="cuda")  # fp32 x, fp32 out of the same size, 64 floats apart
    x = buf[:2 * 5 * 4 * 32].view(2, 5, 4, 32)
    with pytest.raises(RuntimeError, match="overlaps"):
        conv(Cout=32, xt=x, out=buf[64:].view(2, 5, 4, 32))
    torch.cuda.synchronize()
