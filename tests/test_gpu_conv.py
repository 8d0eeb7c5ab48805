"""-m gpu: the NHWC implicit-GEMM convolution and the NHWC average pool of csrc/conv.hip at the operator level, element by
element against the fp64 reference of tests/conv_util.py (bounds, cases and their reasons: that module; tests/test_conv_ref_cpu.py
shows without a device that the bounds refuse every mutant).  Reached through avf_conv2d_nhwc / avf_avgpool_nhwc; every case first
asserts with avf_conv_plan - the launcher's own decision - the tile it names, and the file as a whole that both tiles and all 48
(tile, x type, out type, residual, ReLU) instantiations were run.

Every operand is a view into a larger allocation: NaN around x, w, scale, shift and the residual (a read outside an operand
poisons the output), a sentinel around the output that must be intact afterwards.  A second call returns the same bits.  Each
run prints a line "CONVSTAT {json}" with its worst error / bound ratio.

Worst error / bound ratios measured on an MI355X over the whole file: 0.023 with an fp32 output (the 128 x 64 tile; 0.012 on the
64 x 32 tile), 0.998 with a bf16 output (by construction: some element sits at a rounding tie, where a correct round-to-nearest errs
by the half ulp that is the bound), 0.13 for the average pool."""
import json

import pytest
import torch

import conv_util as cu
from conv_util import SENTINEL, _inside, _intact

pytestmark = pytest.mark.gpu

REACHED = set()


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


@pytest.mark.parametrize("case", cu.CASES, ids=[c["id"] for c in cu.CASES])
def test_conv_matches_fp64_reference(ops, case):
    N, H, W, Cin, Cout, k, s = case["shape_id"]
    plan = ops.conv_plan(N, H, W, Cin, Cout, k, s)
    assert plan["tile"] == case["tile"] and (plan["tile_m"], plan["tile_n"]) == cu.TILES[case["tile"]], plan
    inp = cu.inputs(case)
    Ho, Wo = cu.out_hw(H, W, k, s)
    nan = float("nan")
    _, x = _inside(inp["x"], nan)
    _, w = _inside(inp["w"].reshape(Cout, -1), nan)
    _, scale = _inside(inp["scale"], nan)
    _, shift = _inside(inp["shift"], nan)
    res = None if inp["res"] is None else _inside(inp["res"], nan)[1]
    obuf, out = _inside(torch.full((N, Ho, Wo, Cout), SENTINEL, dtype=cu.DT[case["out"]]), SENTINEL)
    got = ops.conv2d_nhwc(x, w, scale, shift, k, s, residual=res, relu=case["relu"], out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.clone()
    _intact(case["id"], obuf, out.numel())
    ref = cu.reference(case)
    ratio = cu._ratio(out.cpu().reshape(-1, Cout), ref["C"], cu.bound_for(ref, out.dtype))
    print("CONVSTAT " + json.dumps(dict(case=case["id"], ratio=round(ratio, 4))))
    assert ratio <= 1.0, f"{case['id']}: error / bound = {ratio}"
    ops.conv2d_nhwc(x, w, scale, shift, k, s, residual=res, relu=case["relu"], out=out)
    assert torch.equal(out.view(torch.int16 if out.dtype == torch.bfloat16 else torch.int32),
                       first.view(torch.int16 if out.dtype == torch.bfloat16 else torch.int32)), "a second call differs"
    REACHED.add((plan["tile"], case["x"], case["out"], case["res"], case["relu"]))


def test_every_tile_and_instantiation_was_reached():
    assert len(REACHED) == 48, sorted(set((t,) + c for t in (0, 1) for c in cu.COMBOS) - REACHED)


def test_pack_weight_layout_and_folded_batchnorm(ops):
    g = torch.Generator().manual_seed(11)
    for Cout, Cin, k in ((48, 32, 3), (16, 96, 1)):
        w = torch.randn(Cout, Cin, k, k, generator=g)
        gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
        mean, var, eps = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.01, 1e-5
        wp, scale, shift = ops.conv_pack_weight(*[t.cuda() for t in (w, gamma, beta, mean, var)], eps)
        assert wp.dtype == torch.bfloat16 and tuple(wp.shape) == (Cout, k * k * Cin)
        assert torch.equal(wp.cpu().float(), w.permute(0, 2, 3, 1).reshape(Cout, -1).bfloat16().float())  # one RNE rounding
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
        return ops.conv2d_nhwc(x, w, sc, sc.clone(), k, s, out=out)

    conv()
    with pytest.raises(RuntimeError, match=r"Cin % 32 == 0"):
        conv(Cin=48)
    with pytest.raises(RuntimeError, match=r"Cout % 16 == 0"):
        conv(Cout=24)
    with pytest.raises(RuntimeError, match="kernel size 5"):
        conv(k=5, H=7, W=7)
    with pytest.raises(RuntimeError, match="stride 3"):
        conv(s=3)
    with pytest.raises(RuntimeError, match="Cin % 32 == 0"):
        ops.conv_plan(2, 5, 4, 40, 16, 3, 1)
    buf = torch.zeros(2 * 5 * 4 * 32 + 64, device="cuda")  # fp32 x, fp32 out of the same size, 64 floats apart
    x = buf[:2 * 5 * 4 * 32].view(2, 5, 4, 32)
    with pytest.raises(RuntimeError, match="overlaps"):
        conv(Cout=32, xt=x, out=buf[64:].view(2, 5, 4, 32))
    with pytest.raises(RuntimeError, match=r"C % 4 == 0"):
        ops.avgpool_nhwc(torch.zeros(2, 4, 6, device="cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("HW,Cn,xd", cu.POOL_CASES)
def test_avgpool_matches_fp64_reference(ops, HW, Cn, xd):
    xc = cu.pool_inputs(HW, Cn, xd)
    _, x = _inside(xc, float("nan"))
    obuf, out = _inside(torch.full((xc.shape[0], Cn), SENTINEL), SENTINEL)
    ops.avgpool_nhwc(x, out=out)
    torch.cuda.synchronize()
    _intact("avgpool", obuf, out.numel())
    mean, b = cu.pool_reference(xc)
    ratio = cu._ratio(out.cpu(), mean, b)
    print("CONVSTAT " + json.dumps(dict(case=f"avgpool-{HW}-{Cn}-{xd}", ratio=round(ratio, 4))))
    assert ratio <= 1.0
