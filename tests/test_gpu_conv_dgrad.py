"""-m gpu: the data gradient of the NHWC implicit-GEMM convolution and the backward of the NHWC average pool (csrc/conv_dgrad.hip)
at the operator level, element by element against the fp64 reference of tests/conv_dgrad_util.py (bounds, cases and their
reasons: that module; tests/test_conv_dgrad_ref_cpu.py anchors the reference to torch.autograd and shows without a device that
the bounds refuse every mutant).  Reached through avf_conv2d_nhwc_dgrad / avf_avgpool_nhwc_bwd; every case first asserts with
avf_conv_dgrad_plan - the launcher's own decision - the tile it names, and the file as a whole that both tiles and all 32
(tile, gy type, out type, addend, gate) instantiations were run.

Every operand is a view into a larger allocation: NaN around gy, wt, the addend and the gate (a read outside an operand poisons
the output), a sentinel around the output that must be intact afterwards.  A second call returns the same bits.  Each run
prints a line "CONVDGRADSTAT {json}" with its worst error / bound ratio."""
import json

import pytest
import torch

import conv_dgrad_util as du
from conv_util import DT, SENTINEL, TILES, U, _inside, _intact, out_hw

pytestmark = pytest.mark.gpu

REACHED = set()


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("case", du.CASES, ids=[c["id"] for c in du.CASES])
def test_dgrad_matches_fp64_reference(ops, case):
    N, H, W, Cin, Cout, k, s = case["shape_id"]
    plan = ops.conv_dgrad_plan(N, H, W, Cin, Cout, k, s)
    assert plan["tile"] == case["tile"] and (plan["tile_m"], plan["tile_n"]) == TILES[case["tile"]], plan
    inp = du.inputs(case)
    nan = float("nan")
    _, gy = _inside(inp["gy"], nan)
    _, wt = _inside(inp["wt"].reshape(Cin, -1), nan)
    add = None if inp["addend"] is None else _inside(inp["addend"], nan)[1]
    gate = None if inp["gate"] is None else _inside(inp["gate"], nan)[1]
    obuf, out = _inside(torch.full((N, H, W, Cin), SENTINEL, dtype=DT[case["out"]]), SENTINEL)
    got = ops.conv2d_nhwc_dgrad(gy, wt, (H, W), k, s, addend=add, gate=gate, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.clone()
    _intact(case["id"], obuf, out.numel())
    ratio = du.ratio(out.cpu().reshape(-1, Cin), du.reference(case))
    print("CONVDGRADSTAT " + json.dumps(dict(case=case["id"], ratio=round(ratio, 4))))
    assert ratio <= 1.0, f"{case['id']}: error / bound = {ratio}"
    ops.conv2d_nhwc_dgrad(gy, wt, (H, W), k, s, addend=add, gate=gate, out=out)
    assert torch.equal(_bits(out), _bits(first)), "a second call differs"
    REACHED.add((plan["tile"], case["gy"], case["out"], case["add"], case["gate"]))


def test_every_tile_and_instantiation_was_reached():
    assert len(REACHED) == 32, sorted(set((t,) + c for t in (0, 1) for c in du.COMBOS) - REACHED)


def test_a_nan_gate_gives_zero(ops):
    gy = torch.randn(2, 3, 3, 32, device="cuda")
    wt = torch.randn(16, 9 * 32, device="cuda").bfloat16()
    gate = torch.full((2, 3, 3, 16), float("nan"), device="cuda")
    assert not bool(ops.conv2d_nhwc_dgrad(gy, wt, (3, 3), 3, 1, gate=gate, out_dtype=torch.float32).any())


def test_pack_helpers_are_one_rounding_of_the_scaled_transposed_weight(ops):
    from oracle.bf16x3 import split
    g = torch.Generator().manual_seed(13)
    for Cout, Cin, k in ((64, 48, 3), (32, 16, 1)):
        w = torch.randn(Cout, Cin, k, k, generator=g)
        gamma, var, eps = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.01, 1e-5
        scale = (gamma.double() / torch.sqrt(var.double() + eps)).float()
        want = (w * scale.view(-1, 1, 1, 1)).permute(1, 2, 3, 0).reshape(Cin, -1)  # fp32(w * scale) as [Cin, k, k, Cout]
        wt = ops.conv_pack_weight_dgrad(w.cuda(), gamma.cuda(), var.cuda(), eps)
        assert wt.dtype == torch.bfloat16 and tuple(wt.shape) == (Cin, k * k * Cout)
        assert torch.equal(_bits(wt.cpu()), _bits(want.bfloat16()))
        hi, lo = ops.conv_pack_weight_dgrad_f32(w.cuda(), gamma.cuda(), var.cuda(), eps)
        wh, wl = split(want)
        assert torch.equal(_bits(hi.cpu()), _bits(wh.bfloat16())) and torch.equal(_bits(lo.cpu()), _bits(wl.bfloat16()))


def test_argument_errors_come_back_as_errors(ops):
    def dgrad(N=2, H=5, W=4, Cin=16, Cout=32, k=3, s=1, out=None, gyt=None, **kw):
        Ho, Wo = out_hw(H, W, k, s)
        gy = torch.zeros(N, Ho, Wo, Cout, device="cuda") if gyt is None else gyt
        wt = torch.zeros(Cin, k * k * Cout, dtype=torch.bfloat16, device="cuda")
        return ops.conv2d_nhwc_dgrad(gy, wt, (H, W), k, s, out=out, **kw)

    dgrad()
    with pytest.raises(RuntimeError, match=r"Cout % 32 == 0"):
        dgrad(Cout=48)
    with pytest.raises(RuntimeError, match=r"Cin % 16 == 0"):
        dgrad(Cin=24)
    with pytest.raises(RuntimeError, match="kernel size 5"):
        ops.conv_dgrad_plan(2, 7, 7, 16, 32, 5, 1)
    with pytest.raises(RuntimeError, match="stride 3"):
        ops.conv_dgrad_plan(2, 7, 7, 16, 32, 3, 3)
    with pytest.raises(RuntimeError, match=r"Cout % 32 == 0"):
        ops.conv_dgrad_plan(2, 5, 4, 16, 40, 3, 1)
    with pytest.raises(RuntimeError, match="empty shape"):
        ops.conv_dgrad_plan(0, 5, 4, 16, 32, 3, 1)
    buf = torch.zeros(2 * 5 * 4 * 32 + 64, device="cuda")  # fp32 gy, fp32 out of the same size, 64 floats apart
    with pytest.raises(RuntimeError, match="overlaps"):
        dgrad(Cin=32, gyt=buf[:2 * 5 * 4 * 32].view(2, 5, 4, 32), out=buf[64:].view(2, 5, 4, 32))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        dgrad(out=torch.zeros(2 * 5 * 4 * 16 + 8, dtype=torch.bfloat16, device="cuda")[1:-7].view(2, 5, 4, 16))
    with pytest.raises(ValueError, match="gate must be"):   # addend and gate have out's type
        dgrad(gate=torch.zeros(2, 5, 4, 16, device="cuda"), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="gives a"):
        ops.conv2d_nhwc_dgrad(torch.zeros(2, 4, 4, 32, device="cuda"), torch.zeros(16, 288, dtype=torch.bfloat16, device="cuda"), (9, 9), 3, 2)
    with pytest.raises(RuntimeError, match=r"C % 8 == 0"):
        ops.avgpool_nhwc_bwd(torch.zeros(2, 12, device="cuda"), 4)
    with pytest.raises(ValueError, match="gate must be"):
        ops.avgpool_nhwc_bwd(torch.zeros(2, 16, device="cuda"), 4, gate=torch.zeros(2, 4, 16, device="cuda"),
                             out=torch.zeros(2, 4, 16, dtype=torch.bfloat16, device="cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("HW,Cn,od,gate", du.POOL_CASES)
def test_avgpool_backward_matches_fp64_reference(ops, HW, Cn, od, gate):
    dout_c, gate_c = du.pool_inputs(HW, Cn, od, gate)
    _, dout = _inside(dout_c, float("nan"))
    gt = None if gate_c is None else _inside(gate_c, float("nan"))[1]
    obuf, out = _inside(torch.full((dout_c.shape[0], HW, Cn), SENTINEL, dtype=DT[od]), SENTINEL)
    ops.avgpool_nhwc_bwd(dout, HW, gate=gt, out=out)
    torch.cuda.synchronize()
    _intact("avgpool_bwd", obuf, out.numel())
    ratio = du.pool_check("avgpool_bwd", out.cpu(), dout_c, HW, gate_c)
    print("CONVDGRADSTAT " + json.dumps(dict(case=f"avgpool_bwd-{HW}-{Cn}-{od}-gate{int(gate)}", ratio=round(ratio, 4))))
