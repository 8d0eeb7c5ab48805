"""-m gpu: the second pool geometry of the fused ResNet stem (csrc/stem.hip, avf_stem_nchw_pool with AVF_STEM_POOL_CEIL: maxpool
3x3 / 2 / pad 0, ceil_mode - the stem of the VGGFace2 ResNet-50) at the operator level, element by element against the fp64
reference of tests/stem_pool_util.py (shapes and their reasons: that module; bounds: tests/stem_util.py;
tests/test_stem_pool_ref_cpu.py shows without a device that the bounds refuse the mutants of the new geometry).

As in tests/test_gpu_stem.py, x is a view at an ODD element offset inside a NaN-filled buffer (a read outside x poisons the
output), w / scale / shift sit between NaNs, the output between sentinels that must be intact afterwards (a canary behind
``out``, and one in front).  Mode 0 through the new entry returns the bits of avf_stem_nchw.  Each run prints a line
"STEMPOOLSTAT {json}" with its worst error / bound ratio.

Worst error / bound ratios measured on an MI355X over the whole file: 0.009 with an fp32 output, 0.987 with a bf16 output (by
construction: some element sits near a rounding tie, where a correct round-to-nearest errs by almost the half ulp that is the bound)."""
import json

import pytest
import torch

import stem_pool_util as sp
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
    """the packed image of the case's bf16 weights with scale / shift passed through the fold (gamma = scale, beta = shift, mean = 0,
    var = 1, eps = 0: exact)"""
    one, zero = torch.ones(su.COUT), torch.zeros(su.COUT)
    wp, sc, sh = ops.stem_pack_weight(*[t.cuda() for t in (inp["w"].float(), inp["scale"], inp["shift"], zero, one)], eps=0.0)
    assert torch.equal(sc.cpu(), inp["scale"]) and torch.equal(sh.cpu(), inp["shift"])
    return wp, sc, sh


@pytest.mark.parametrize("case", sp.CASES, ids=[c["id"] for c in sp.CASES])
def test_ceil_mode_stem_matches_fp64_reference(ops, case):
    N, Cin, H, W = case["shape"]
    inp = sp.inputs(case)
    Hp, Wp = sp.out_hw(H, W)
    assert ops.stem_out_hw(H, W, pool="ceil") == (Hp, Wp)
    nan = float("nan")
    wp, sc, sh = _packed(ops, inp)
    _, x = _inside(inp["x"], nan, shift=ODD)
    assert (x.data_ptr() // x.element_size()) % 2 == 1
    _, wp = _inside(wp.cpu(), nan)
    _, sc = _inside(sc.cpu(), nan)
    _, sh = _inside(sh.cpu(), nan)
    obuf, out = _inside(torch.full((N, Hp, Wp, su.COUT), SENTINEL, dtype=sp.DT[case["out"]]), SENTINEL)
    got = ops.stem_nchw(x, wp, sc, sh, out=out, pool="ceil")
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.clone()
    n = out.numel()
    assert bool((obuf[:GUARD] == SENTINEL).all()) and bool((obuf[GUARD + n:] == SENTINEL).all()), "a write outside the output"
    ref = sp.reference(case["shape"])
    ratio = sp.ratio(ref, out.cpu())
    print("STEMPOOLSTAT " + json.dumps(dict(case=case["id"], ratio=round(ratio, 4))))
    assert ratio <= 1.0, f"{case['id']}: error / bound = {ratio}"
    ops.stem_nchw(x, wp, sc, sh, out=out, pool="ceil")
    bits = torch.int16 if out.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(out.view(bits), first.view(bits)), "a second call differs"


def _raw(lib, name, x, wp, sc, sh, out, *mode):
    import avformer_amd as A
    _ptr, _stream, avf_dtype = A.ops._ptr, A.ops._stream, A.ops.avf_dtype
    N, Cin, H, W = x.shape
    return getattr(lib, name)(_ptr(x), avf_dtype(x.dtype), _ptr(wp), _ptr(sc), _ptr(sh), _ptr(out), avf_dtype(out.dtype), N, Cin, H, W,
                              *mode, _stream())


@pytest.mark.parametrize("shape,xd,od", [((2, 3, 112, 112), "f32", "bf16"), ((2, 4, 113, 111), "bf16", "f32")])
def test_mode_0_through_the_new_entry_is_avf_stem_nchw_bit_for_bit(ops, shape, xd, od):
    import avformer_amd as A
    lib = A._lib.load()
    inp = su.inputs(dict(shape=shape, x=xd))
    wp, sc, sh = _packed(ops, inp)
    x = inp["x"].cuda()
    Hp, Wp = su.out_hw(*shape[2:])
    old = torch.full((shape[0], Hp, Wp, su.COUT), SENTINEL, dtype=su.DT[od], device="cuda")
    new = old.clone()
    assert _raw(lib, "avf_stem_nchw", x, wp, sc, sh, old) == 0
    assert _raw(lib, "avf_stem_nchw_pool", x, wp, sc, sh, new, A._lib.STEM_POOL_PAD1) == 0
    torch.cuda.synchronize()
    bits = torch.int16 if old.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(old.view(bits), new.view(bits))
    assert su.ratio(su.reference(shape), new.cpu()) <= 1.0
    assert torch.equal(ops.stem_nchw(x, wp, sc, sh, out_dtype=su.DT[od]).view(bits), old.view(bits))   # the default is mode 0


def test_the_two_refusals(ops):
    import avformer_amd as A
    lib = A._lib.load()
    o = torch.ones(64, device="cuda")
    wp, sc, sh = ops.stem_pack_weight(torch.zeros(64, 3, 7, 7, device="cuda"), o, o.clone(), o.clone(), o.clone())
    ops.stem_nchw(torch.zeros(2, 3, 3, 3, device="cuda"), wp, sc, sh, pool="ceil")          # the smallest shape the mode takes
    for H, W in ((2, 9), (9, 2)):                                                           # conv map 1 x 5 / 5 x 1
        x = torch.zeros(2, 3, H, W, device="cuda")
        ops.stem_nchw(x, wp, sc, sh)                                                        # mode 0 takes it
        with pytest.raises(RuntimeError, match="smaller than 2 x 2"):
            ops.stem_nchw(x, wp, sc, sh, pool="ceil")
        out = torch.full((2, 1, 3, 64), SENTINEL, dtype=torch.bfloat16, device="cuda")
        assert _raw(lib, "avf_stem_nchw_pool", x, wp, sc, sh, out, A._lib.STEM_POOL_CEIL) != 0
        assert "at least 3" in lib.avf_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())                                               # refused before any launch
    x = torch.zeros(2, 3, 9, 8, device="cuda")
    out = torch.full((2, 3, 2, 64), SENTINEL, dtype=torch.bfloat16, device="cuda")
    for mode in (2, -1):
        assert _raw(lib, "avf_stem_nchw_pool", x, wp, sc, sh, out, mode) != 0
        msg = lib.avf_last_error().decode()
        assert "AVF_STEM_POOL_PAD1" in msg and "AVF_STEM_POOL_CEIL" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="pad1.*ceil"):
        ops.stem_nchw(x, wp, sc, sh, pool="floor")
