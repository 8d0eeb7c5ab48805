"""-m gpu: the PARITY-MODE attention kernels, group-wise against fp64 (kit: tests/attn_parity_util.py; tests/test_attn_parity_ref_cpu.py
shows without a device that its bounds pass an independent restatement of each arithmetic and refuse the mutants).

csrc/attn_parity_kernel.hpp: attn_fwd_parity_kernel, attn_dq_parity_kernel, attn_dkv_parity_kernel for ParityBf16x3
(attn_f32x3.hip, dim_head 64) and ParityF32Mfma<32 | 64 | 128> (attn_f32_mfma.hip), through avf_attn_fwd / avf_attn_bwd on fp32.
B = 2, H = 3, distinct data per clip and head.  Every test sets the arithmetic (restored in `finally`), asserts with
avf_attn_parity_plan - answered by the predicates the dispatch switches on, asked about the pointers of the very call - which
family the call takes, launches on NaN-filled
outputs and a NaN-filled workspace (delta), twice, and compares the two bit for bit.  The forward (o, lse2) is held to the kit's
bounds, and so is the backward ON REFERENCE-MADE o AND lse2 (fp32 of the fp64 reference), so that a forward fault and a backward
fault cannot agree with each other; every random-operand case then runs the backward once more on the device's own o and lse2 -
what a layer runs - under the bounds widened by attn_parity_util.own_outputs_extra.  One PARITYSTAT line per case: the worst
error / bound per part and the group (clip, head, row block, column block) that gave it.

Lengths: the edges of the 16-row wave block, the 32-row streamed tile and the 64-row workgroup, odd tails for the
two-rows-per-thread staging of the bf16x3 tiles, and 385 keys = 13 tiles.  Nothing here goes through gpu_util.check."""
import json

import pytest
import torch

import attn_parity_util as P
from gpu_util import f32_arithmetic

pytestmark = pytest.mark.gpu

B, H = P.B_, P.H_
MAXIMA = {}   # family -> part -> (ratio, case, group)
TRAINED = {}  # family -> N -> dict(o, dqkv): worst relative Frobenius error per (clip, head)


@pytest.fixture(scope="module")
def A():
    """the package, and at the end of the module the PARITYMAX / PARITYTRAINED lines of whatever cases ran (PARITYSTAT_MAXIMA
    and TRAINED_SCALE of the kit were taken from those of a whole run; which families the case tables reach is asserted in
    tests/test_attn_parity_ref_cpu.py)"""
    import avformer_amd as A
    assert A.ops.device_ok()
    yield A
    print("PARITYMAX " + json.dumps({f: {p: dict(ratio=v[0], case=v[1], group=v[2]) for p, v in parts.items()}
                                     for f, parts in sorted(MAXIMA.items())}))
    print("PARITYTRAINED " + json.dumps(TRAINED))


def _note(family, c, stats):
    case = dict(dh=c.dh, N=c.N, regime=c.regime)
    print("PARITYSTAT " + json.dumps(dict(family=family, **case, **stats)))
    for part, s in stats.items():
        if "ratio" in s and s["ratio"] > MAXIMA.setdefault(family, {}).get(part, (-1.0,))[0]:
            MAXIMA[family][part] = (s["ratio"], case, s["group"])


def _run(A, c, setting, family, label=None, misaligned=False, own_outputs=True):
    """one case under `setting`: forward, backward on reference-made inputs, backward on the device's own outputs; every
    launch asserts plan == family from the pointers it launches with (attn_parity_util.assert_plan); the bounds are those of
    the arithmetic the family computes in (the vector kernels: "f32")"""
    arith = "f32" if family == "vec" else family
    label = label or family
    tag = f"{label}[{c.dh},{c.N},{c.regime}]"
    with f32_arithmetic(setting):  # (sets it; restores the previous one in its `finally`)
        assert A._lib.get_f32_arithmetic() == setting
        o, lse2 = P.run_forward(A, c.qkv, *c.dims, family, tag=tag + ":fwd", misaligned=misaligned)
        stats = dict(c.check_forward(tag + ":fwd", dict(o=o, lse2=lse2), arith))
        got = P.run_backward(A, c.qkv, c.o_in, c.lse2_in, c.d_o, *c.dims, family, tag=tag + ":bwd", misaligned=misaligned)
        stats.update(c.check_backward(tag + ":bwd", got, arith))
        if c.regime == "trained":
            fro = dict(o=P.head_errors(o, c.ref["o"]), dqkv=P.head_errors(torch.cat([got[p] for p in P.PARTS_BWD], -1),
                                                                          torch.cat([c.ref[p] for p in P.PARTS_BWD], -1)))
            stats["trained_rel_fro"] = {k: float(f"{v:.3e}") for k, v in fro.items()}
            TRAINED.setdefault(label, {})[c.N] = stats["trained_rel_fro"]
        if own_outputs and c.regime is None:
            own = P.run_backward(A, c.qkv, o, lse2, c.d_o, *c.dims, family, tag=tag + ":bwd_own", misaligned=misaligned)
            for part, s in c.check_backward(tag + ":bwd_own", own, arith, own_outputs=True).items():
                stats[part + "_own"] = s
    _note(label, c, stats)
    return stats


# ---------------------------------------------------------------------------------------------- random operands
@pytest.mark.parametrize("family,dh,N", P.RANDOM_CASES)
def test_random_operands(A, family, dh, N):
    """both families at dim_head 64 over every length, "f32" at dim_head 32 and 128 over the ragged ones: forward and backward
    under 2 x the emulation's error + the floor, lse2 under its tolerance, the sign statistic"""
    _run(A, P.case(N, dh), family, family, label=family if dh == 64 else f"{family}_dh{dh}")


@pytest.mark.parametrize("dh,N", P.OTHER_WIDTHS_UNDER_BF16X3)
def test_other_head_widths_under_the_bf16x3_setting(A, dh, N):
    """dim_head 32 and 128 have no bf16x3 kernels: under that setting the plan must say f32 MFMA, and the result is held to
    the "f32" bounds"""
    _run(A, P.case(N, dh), "bf16x3", "f32", label=f"f32_dh{dh}_under_bf16x3")


# ---------------------------------------------------------------------------------------------- score regimes
@pytest.mark.parametrize("family,dh,N,regime", P.REGIME_CASES)
def test_score_regimes(A, family, dh, N, regime):
    """alpha doing real work on every tile (ramp, small_steps), only on the first (descending), a far-negative maximum
    (very_negative: a padded key left unmasked at these ragged lengths would take all the weight), scores of hundreds of nats
    (huge) and trained-scale scores (trained) - under the worst-case bound, which needs no emulation"""
    _run(A, P.case(N, dh, regime), family, family, label=f"regime_{family}" if dh == 64 else f"regime_{family}_dh{dh}")


# ---------------------------------------------------------------------------------------------- fallbacks
def test_misaligned_qkv_falls_back_to_the_vector_kernels(A):
    """a qkv whose storage starts 4 bytes past a 16-byte boundary: the plan says vector kernels under either setting, and
    the result stays within the "f32" bounds (one lane per query, an fmaf chain: the same precision class)"""
    dh, N = P.MISALIGNED
    for setting in P.ARITHS:
        _run(A, P.case(N, dh), setting, "vec", label=f"vec_misaligned_under_{setting}", misaligned=True)


def test_prescaled_bf16_projection_is_not_planned_onto_a_parity_family(A):
    """the layer path of a masked bf16 stack hands attn_fwd_vec a bf16 projection with pre-scaled q: neither parity family may
    take it (their kernels would scale q again and read fp32), under either setting, masked or not"""
    L = A._lib
    for setting in P.ARITHS:
        with f32_arithmetic(setting):
            for dh in (32, 64, 128):
                for masked in (False, True):
                    assert P.parity_plan(A, dh, H, masked=masked, q_prescaled=True, dtype=L.BF16) == "vec", (setting, dh, masked)
                assert P.parity_plan(A, dh, H, q_prescaled=True) == "vec" and P.parity_plan(A, dh, H, dtype=L.BF16) == "vec"
    # (what such a call computes - the fp32-arithmetic kernels on bf16 storage - is held to fp64 by
    # tests/test_gpu_attn_bf16.py::test_fp32_arithmetic_under_a_mask and tests/test_gpu_mask_core.py)
