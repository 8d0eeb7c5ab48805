"""CPU (no GPU needed): the fp64 reference of tests/stem_util.py is torch's conv 7x7 / 2 -> eval-mode BatchNorm -> ReLU ->
maxpool 3x3 / 2, its cases are not vacuous, and its element-wise bounds refuse every mutant - what tests/test_gpu_stem.py asserts of
the device bites.  halo_unmasked is invisible on the even conv maps (error / bound exactly 0 on (2, 3, 112, 112)): the odd shapes of
stem_util.SHAPES are there for it."""
import pytest
import torch
from torch.nn import functional as F

import stem_util as su

SHAPE_IDS = ["x".join(map(str, s)) for s in su.SHAPES]


@pytest.mark.parametrize("shape", su.SHAPES, ids=SHAPE_IDS)
def test_shape_is_not_vacuous(shape):
    su.guard(shape)


def test_the_cases_are_the_issue_list_in_every_type_combination():
    assert len(su.CASES) == 4 * len(su.SHAPES) == 36
    assert {(c["x"], c["out"]) for c in su.CASES} == {(a, b) for a in ("f32", "bf16") for b in ("f32", "bf16")}
    assert any(su.conv_hw(*s[2:])[0] % 2 and su.conv_hw(*s[2:])[1] % 2 for s in su.SHAPES)


@pytest.mark.parametrize("shape", su.SHAPES, ids=SHAPE_IDS)
def test_reference_is_torch_stem(shape):
    """fp64 torch ops on the bf16-rounded x give the reference to fp64 round-off; torch's own fp32 ops stay far inside the fp32
    bound and inside the bf16 one"""
    o = su.operands(shape)
    ref = su.reference(shape)
    xb = o["x"].bfloat16()
    want = F.conv2d(xb.double(), o["w"].double(), stride=2, padding=3) * o["scale"].double().view(1, -1, 1, 1) + o["shift"].double().view(1, -1, 1, 1)
    want = F.max_pool2d(F.relu(want), 3, 2, 1).permute(0, 2, 3, 1)
    assert tuple(want.shape) == (shape[0],) + su.out_hw(*shape[2:]) + (su.COUT,)
    assert float((ref["C"] - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
    y32 = F.conv2d(xb.float(), o["w"].float(), stride=2, padding=3) * o["scale"].view(1, -1, 1, 1) + o["shift"].view(1, -1, 1, 1)
    y32 = F.max_pool2d(F.relu(y32), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    assert su.ratio(ref, y32) <= 0.03
    assert su.ratio(ref, y32.bfloat16()) < 1.0


@pytest.mark.parametrize("case", su.CASES, ids=[c["id"] for c in su.CASES])
def test_bounds_pass_the_reference_and_refuse_every_mutant(case):
    shape, dt = case["shape"], su.DT[case["out"]]
    ref = su.reference(shape)
    assert su.ratio(ref, su.round_to(su.simulate(shape), dt)) <= 1.0
    for name, applies in su.MUTANTS.items():
        if applies(shape):
            r = su.ratio(ref, su.round_to(su.simulate(shape, name), dt))
            assert r > 1.0, (name, r)
        elif name == "halo_unmasked":
            assert torch.equal(su.simulate(shape, name), ref["C"]), name  # invisible on an even conv map


def test_halo_unmasked_is_invisible_on_the_video_frame():
    shape = (2, 3, 112, 112)
    assert not su.MUTANTS["halo_unmasked"](shape)
    assert su._ratio(su.simulate(shape, "halo_unmasked"), su.reference(shape)["C"], su.reference(shape)["bC"]) == 0.0


def test_every_mutant_applies_somewhere():
    for name, applies in su.MUTANTS.items():
        assert sum(applies(s) for s in su.SHAPES) >= 5, name
