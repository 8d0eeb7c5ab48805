"""CPU (no GPU needed): the fp64 reference of tests/stem_pool_util.py is torch's conv 7x7 / 2 -> eval-mode BatchNorm -> ReLU ->
max_pool2d(3, 2, padding=0, ceil_mode=True); avf_stem_out_hw (host only: the shape rule the launch acts on) is torch's output size
in both pool modes; and the element-wise bounds refuse the mutants of the new geometry - what tests/test_gpu_stem_pool.py asserts
of the device bites.  Unlike the pad-1 geometry, ``halo_unmasked`` shows on EVEN conv maps here, the 112 x 112 video frame included."""
import ctypes as C

import pytest
import torch
from torch.nn import functional as F

import stem_pool_util as sp
import stem_util as su

SHAPE_IDS = ["x".join(map(str, s)) for s in sp.SHAPES]


@pytest.mark.parametrize("shape", sp.SHAPES, ids=SHAPE_IDS)
def test_shape_is_not_vacuous(shape):
    sp.guard(shape)


def test_the_cases_are_the_issue_list_in_every_type_combination():
    assert sp.SHAPES == [(2, 3, 112, 112), (3, 3, 37, 29), (2, 4, 30, 45), (2, 1, 7, 5), (2, 4, 113, 111), (3, 3, 3, 4)]
    assert len(sp.CASES) == 4 * len(sp.SHAPES)
    assert {(c["x"], c["out"]) for c in sp.CASES} == {(a, b) for a in ("f32", "bf16") for b in ("f32", "bf16")}


@pytest.mark.parametrize("shape", sp.SHAPES, ids=SHAPE_IDS)
def test_reference_is_torch_stem_with_the_ceil_mode_pool(shape):
    o = su.operands(shape)
    ref = sp.reference(shape)
    xb = o["x"].bfloat16()
    want = F.conv2d(xb.double(), o["w"].double(), stride=2, padding=3) * o["scale"].double().view(1, -1, 1, 1) + o["shift"].double().view(1, -1, 1, 1)
    want = F.max_pool2d(F.relu(want), 3, 2, 0, ceil_mode=True).permute(0, 2, 3, 1)
    assert tuple(want.shape) == (shape[0],) + sp.out_hw(*shape[2:]) + (su.COUT,)
    assert float((ref["C"] - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
    y32 = F.conv2d(xb.float(), o["w"].float(), stride=2, padding=3) * o["scale"].view(1, -1, 1, 1) + o["shift"].view(1, -1, 1, 1)
    y32 = F.max_pool2d(F.relu(y32), 3, 2, 0, ceil_mode=True).permute(0, 2, 3, 1).contiguous()
    assert sp.ratio(ref, y32) <= 0.03
    assert sp.ratio(ref, y32.bfloat16()) < 1.0


def _lib_out_hw(lib, H, W, mode):
    out = [C.c_int(-1) for _ in range(4)]
    rc = lib.avf_stem_out_hw(H, W, mode, *[C.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


def test_stem_out_hw_is_torchs_output_size_in_both_modes():
    import avformer_amd as A
    lib = A._lib.load()
    w = torch.zeros(1, 1, 7, 7)
    conv = {L: F.conv2d(torch.zeros(1, 1, L, L), w, stride=2, padding=3).shape[-1] for L in range(3, 41)}
    pool = {0: {Lc: F.max_pool2d(torch.zeros(1, 1, Lc, Lc), 3, 2, 1).shape[-1] for Lc in set(conv.values())},
            1: {Lc: F.max_pool2d(torch.zeros(1, 1, Lc, Lc), 3, 2, 0, ceil_mode=True).shape[-1] for Lc in set(conv.values())}}
    for mode, name in ((A._lib.STEM_POOL_PAD1, "pad1"), (A._lib.STEM_POOL_CEIL, "ceil")):
        for H in range(3, 41):
            for W in range(3, 41):
                rc, got = _lib_out_hw(lib, H, W, mode)
                assert rc == 0 and got == (conv[H], conv[W], pool[mode][conv[H]], pool[mode][conv[W]]), (mode, H, W, got)
        assert A.ops.stem_out_hw(30, 37, pool=name) == (pool[mode][conv[30]], pool[mode][conv[37]])
    # a rectangular map through torch itself, once per mode
    assert tuple(F.max_pool2d(torch.zeros(1, 1, conv[28], conv[20]), 3, 2, 0, ceil_mode=True).shape[2:]) == A.ops.stem_out_hw(28, 20, "ceil") == (7, 5)
    assert tuple(F.max_pool2d(torch.zeros(1, 1, conv[28], conv[20]), 3, 2, 1).shape[2:]) == A.ops.stem_out_hw(28, 20) == (7, 5)
    assert A.ops.stem_out_hw(30, 45) == (8, 12) and A.ops.stem_out_hw(30, 45, "ceil") == (7, 11)


def test_stem_out_hw_refusals():
    import avformer_amd as A
    lib = A._lib.load()
    for H, W in ((2, 9), (9, 2), (1, 1)):
        assert _lib_out_hw(lib, H, W, A._lib.STEM_POOL_PAD1)[0] == 0         # the pad-1 pool takes any H, W >= 1
        with pytest.raises(RuntimeError, match="smaller than 2 x 2"):
            A.ops.stem_out_hw(H, W, pool="ceil")
        with pytest.raises(RuntimeError):                                     # as torch refuses that conv map
            F.max_pool2d(torch.zeros(1, 1, *su.conv_hw(H, W)), 3, 2, 0, ceil_mode=True)
    rc, _ = _lib_out_hw(lib, 9, 9, 2)
    assert rc != 0
    msg = lib.avf_last_error().decode()
    assert "AVF_STEM_POOL_PAD1" in msg and "AVF_STEM_POOL_CEIL" in msg
    with pytest.raises(ValueError, match="pad1.*ceil"):
        A.ops.stem_out_hw(9, 9, pool="floor")


@pytest.mark.parametrize("case", sp.CASES, ids=[c["id"] for c in sp.CASES])
def test_bounds_pass_the_reference_and_refuse_every_mutant(case):
    shape, dt = case["shape"], sp.DT[case["out"]]
    ref = sp.reference(shape)
    assert sp.ratio(ref, su.round_to(sp.simulate(shape), dt)) <= 1.0
    for name, applies in sp.MUTANTS.items():
        if applies(shape):
            r = sp.ratio(ref, su.round_to(sp.simulate(shape, name), dt))
            assert r > 1.0, (name, r)
        else:                                                 # invisible there (an odd conv map: the last window ends inside it)
            assert torch.equal(sp.simulate(shape, name), ref["C"]), name


def test_halo_unmasked_shows_on_the_video_frame():
    """the 56 x 56 conv map of a 112 x 112 frame is even: invisible in the pad-1 geometry (tests/test_stem_ref_cpu.py), visible here"""
    shape = (2, 3, 112, 112)
    assert sp.MUTANTS["halo_unmasked"](shape) and not su.MUTANTS["halo_unmasked"](shape)
    ref = sp.reference(shape)
    assert su._ratio(sp.simulate(shape, "halo_unmasked"), ref["C"], ref["bC"]) > 1.0


def test_every_mutant_applies_on_several_shapes():
    for name, applies in sp.MUTANTS.items():
        assert sum(applies(s) for s in sp.SHAPES) >= 3, name
