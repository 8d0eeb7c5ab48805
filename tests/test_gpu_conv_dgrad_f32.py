"""-m gpu: the parity form of the convolution's data gradient (csrc/conv_dgrad_f32.hip: conv_dgrad_nhwc_kernel<ConvBf16x3>)
at the operator level on the shapes of tests/test_gpu_conv_dgrad.py, with the two checks of tests/conv_f32_util.py as
tests/conv_dgrad_util.py restates them: element by element against the exact fp64 product of the fp32 operands within the
derived bound, and relative Frobenius <= 1e-6 against the three-term emulation (oracle/bf16x3.py).  Every case first asserts
its tile with avf_conv_dgrad_plan; operands are NaN-surrounded views, the output sits inside a sentinel, a second call returns
the same bits, and all 8 (tile, addend, gate) instantiations are counted.  The weight images are oracle.bf16x3.split of the
fp32 wt (the pack helper is checked bitwise against that split in test_gpu_conv_dgrad.py).  Each run prints "CONVDGRADSTAT"."""
import json

import pytest
import torch

import conv_dgrad_util as du
from conv_util import SENTINEL, TILES, _inside, _intact
from oracle.bf16x3 import split

pytestmark = pytest.mark.gpu

REACHED = set()


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


@pytest.mark.parametrize("case", du.F32_CASES, ids=[c["id"] for c in du.F32_CASES])
def test_dgrad_f32_matches_exact_and_emulated_reference(ops, case):
    N, H, W, Cin, Cout, k, s = case["shape_id"]
    plan = ops.conv_dgrad_plan(N, H, W, Cin, Cout, k, s)
    assert plan["tile"] == case["tile"] and (plan["tile_m"], plan["tile_n"]) == TILES[case["tile"]], plan
    inp = du.inputs(case)
    nan = float("nan")
    _, gy = _inside(inp["gy"], nan)
    wh, wl = [_inside(t.reshape(Cin, -1).bfloat16(), nan)[1] for t in split(inp["wt_f32"])]
    add = None if inp["addend"] is None else _inside(inp["addend"], nan)[1]
    gate = None if inp["gate"] is None else _inside(inp["gate"], nan)[1]
    obuf, out = _inside(torch.full((N, H, W, Cin), SENTINEL), SENTINEL)
    got = ops.conv2d_nhwc_dgrad_f32(gy, (wh, wl), (H, W), k, s, addend=add, gate=gate, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.clone()
    _intact(case["id"], obuf, out.numel())
    exact, emulated = du.f32_reference(case)
    ratio, fro = du.ratio(out.cpu().reshape(-1, Cin), exact), du.rel_fro(out.cpu(), emulated)
    print("CONVDGRADSTAT " + json.dumps(dict(case=case["id"] + "-f32x3", ratio=round(ratio, 4), rel_fro_emulated=fro)))
    assert ratio <= 1.0, f"{case['id']}: error / bound = {ratio}"
    assert fro <= du.CAP, f"{case['id']}: relative Frobenius error against the emulated bf16x3 product = {fro}"
    ops.conv2d_nhwc_dgrad_f32(gy, (wh, wl), (H, W), k, s, addend=add, gate=gate, out=out)
    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), "a second call differs"
    REACHED.add((plan["tile"], case["add"], case["gate"]))


def test_every_tile_and_instantiation_was_reached():
    assert len(REACHED) == 8, REACHED


def test_argument_errors_come_back_as_errors(ops):
    gy = torch.zeros(2, 5, 4, 32, device="cuda")
    w = torch.zeros(16, 288, dtype=torch.bfloat16, device="cuda")
    ops.conv2d_nhwc_dgrad_f32(gy, (w, w.clone()), (5, 4), 3, 1)
    with pytest.raises(ValueError, match="gy must be"):
        ops.conv2d_nhwc_dgrad_f32(gy.bfloat16(), (w, w.clone()), (5, 4), 3, 1)
    with pytest.raises(RuntimeError, match=r"Cout % 32 == 0"):
        ops.conv2d_nhwc_dgrad_f32(torch.zeros(2, 5, 4, 16, device="cuda"), (w[:, :144].contiguous(), w[:, :144].contiguous()), (5, 4), 3, 1)
    torch.cuda.synchronize()
