"""-m gpu: the UNMASKED bf16 attention kernels, group-wise against fp64 (kit: tests/attn_bf16_util.py; tests/test_attn_bf16_ref_cpu.py
shows without a device that its bounds pass a correct rounding and refuse the mutants).

csrc/attn_bf16.hip: attn_fwd_res_kernel<8 | 12 | 8,multi>, attn_fwd_bf16_kernel, attn_dq/dkv_bf16_kernel; csrc/attn_bwd_merged.hip: attn_bwd_m4_kernel<KB 1..4, RAGGED, MXO>.  B = 2, H = 3, distinct data per clip
and head.  Every case asserts with the plan query (ops.attn_plan, answered by the functions the launchers switch on) that it
runs the kernel it names, launches on NaN-filled outputs, twice, and compares the two bit for bit; the forward (o, lse2) is
held to the kit's bounds, and so is the backward ON REFERENCE-MADE o AND lse2 (bf16 / fp32 of the fp64 reference), so that a
forward fault and a backward fault cannot agree with each other.  One ATTNSTAT line per launch: the worst error / bound per
part and the group (clip, head, row block, column block) that gave it.  Nothing here goes through gpu_util.check."""
import json

import pytest
import torch

import attn_bf16_util as K
import oracle

pytestmark = pytest.mark.gpu

B, H = K.B_, K.H_
REACHED = set()  # ("fwd", kind), ("bwd", kind), ("bwd", "merged", KB, ragged), ("mx8", KB, ragged)
MAXIMA = {}      # family -> part -> (ratio, case, group)


@pytest.fixture(scope="module")
def A():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A


def _note(family, c, kernel, stats):
    case = dict(N=c.N, dh=c.dh, qs=c.qs, regime=c.regime)
    print("ATTNSTAT " + json.dumps(dict(family=family, kernel=kernel, **case, **stats)))
    for part, s in stats.items():
        if s["ratio"] > MAXIMA.setdefault(family, {}).get(part, (-1.0,))[0]:
            MAXIMA[family][part] = (s["ratio"], case, s["group"])


def _forward(A, c, family, kind):
    p = A.ops.attn_plan(c.N, c.dh, bool(c.qs))
    assert p["fwd"] == kind, (c.N, c.dh, c.qs, p)
    REACHED.add(("fwd", kind))
    tag = f"{family}[{c.N},{c.dh},qs{c.qs},{c.regime}]"
    o, lse2 = K.run_forward(A, c.qkv, *c.dims, c.qs, tag=tag)
    _note(family, c, "fwd:" + kind, c.check_forward(tag, dict(o=o, lse2=lse2), rounded_l=kind != "stream"))


def _backward(A, c, family, kind, kb=0, ragged=False, mx8=False):
    p = A.ops.attn_plan(c.N, c.dh, bool(c.qs))
    assert (p["bwd"], p["kb"], p["ragged"]) == (kind, kb, ragged), (c.N, c.dh, c.qs, p)
    REACHED.add(("bwd", kind, kb, ragged) if kind == "merged" else ("bwd", kind))
    tag = f"{family}[{c.N},{c.dh},qs{c.qs},{c.regime}]"
    got = K.run_backward(A, c.qkv, c.o_in, c.lse2_in, c.d_o, *c.dims, c.qs, mx8=mx8, tag=tag)
    _note(family, c, "bwd:" + kind + (f"<{kb},{int(ragged)}{',mx8' if mx8 else ''}>" if kind == "merged" else ""),
          c.check_backward(tag, got))
    return got


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("kind,N", [(k, N) for k, ns in K.FWD_QS.items() for N in ns])
def test_forward_prescaled_q(A, kind, N):
    """dim_head 64, pre-scaled q: the three head-resident builds at their edges (row groups of 32: 8 | 9 and 12 | 13 groups at
    256 | 257 and 384 | 385; the last resident length 576) and the streaming kernel behind them"""
    _forward(A, K.case(N, 64, 1), "fwd_" + kind, kind)


@pytest.mark.parametrize("dh,N", K.FWD_DH)
def test_forward_dim_head_32_and_128(A, dh, N):
    """the streaming kernel's other two builds (four waves of 32 rows; eight waves of 16 rows at dim_head 128)"""
    _forward(A, K.case(N, dh, 1), f"fwd_stream{dh}", "stream")


@pytest.mark.parametrize("dh,N,kind", K.FWD_RAW)
def test_forward_raw_q(A, dh, N, kind):
    """q as the projection leaves it: the kernels scale the scores themselves (one FMA per score)"""
    _forward(A, K.case(N, dh, 0), "fwd_raw_" + ("stream" if kind == "stream" else "res"), kind)


# ---------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("kb,N", [(kb, N) for kb, ns in K.BWD_MERGED.items() for N in ns])
def test_backward_merged(A, kb, N):
    """the default backward (dim_head 64, pre-scaled q, N <= 512): every KB at its first, a middle and its last length, ragged
    (padded keys masked, padded query rows copies of row N - 1) and full"""
    _backward(A, K.case(N, 64, 1), f"bwd_merged_kb{kb}", "merged", kb, N != 128 * kb)


@pytest.mark.parametrize("N", K.MXO_LENGTHS)
def test_backward_merged_mx8_form(A, N):
    """the MXO instantiation: dqkv bit-equal to the plain call's, the image that of the STORED tensor (oracle.mx8_quant)"""
    c = K.case(N, 64, 1)
    kb = (N + 127) // 128
    assert A._lib.load().avf_attn_bwd_emits_mx8(N, 64) == 1
    plain = _backward(A, c, f"bwd_merged_kb{kb}", "merged", kb, N != 128 * kb)
    mx = _backward(A, c, "bwd_merged_mx8", "merged", kb, N != 128 * kb, mx8=True)
    REACHED.add(("mx8", kb, N != 128 * kb))
    assert torch.equal(mx["dqkv"], plain["dqkv"]), "dqkv of the MX-FP8 form differs from the plain kernel's"
    q_ref, s_ref = oracle.mx8_quant(mx["dqkv"].float())
    assert torch.equal(mx["scales"], s_ref)
    assert torch.equal(mx["image"], q_ref)


@pytest.mark.parametrize("dh,N,qs", K.BWD_STREAM)
def test_backward_streaming(A, dh, N, qs):
    """delta + attn_dq_bf16 + attn_dkv_bf16: at dim_head 64 past the merged kernel's 512 tokens with pre-scaled q and at every
    length with raw q (from one ragged 64-row tile at 33 tokens), every length at 32 and 128"""
    _backward(A, K.case(N, dh, qs), f"bwd_stream{dh}" + ("" if qs else "_raw"), "stream")


# ---------------------------------------------------------------------------------------------- score regimes
@pytest.mark.parametrize("regime,N", K.REGIME_CASES)
def test_score_regimes(A, regime, N):
    """the rescale paths of the head-resident forward and the merged backward's exp2(s - lse2) far from zero, under the
    worst-case bound of three bf16 roundings; `very_negative` at 511 and 575 also holds the padded keys of the multi-pass
    build to their mask (past 512 tokens the backward is the streaming pair)"""
    c = K.case(N, 64, 1, regime)
    _forward(A, c, "regime_fwd", "res12" if N <= 384 else "res_multi")
    if N <= 512:
        kb = (N + 127) // 128
        _backward(A, c, "regime_bwd", "merged", kb, N != 128 * kb)
    else:
        _backward(A, c, "regime_bwd", "stream")


# ---------------------------------------------------------------------------------------------- fp32 arithmetic under a mask
def test_fp32_arithmetic_under_a_mask(A):
    """the one plan value no unmasked call reports: a masked bf16 layer at dim_head 32 runs the fp32-arithmetic kernels on
    bf16 storage.  With every token kept the result is the unmasked reference's (no rounding of P: well inside the bounds)"""
    c = K.case(40, 32, 1)
    p = A.ops.attn_plan(40, 32, True, masked=True)
    assert (p["fwd"], p["bwd"]) == ("f32", "f32") and not A.ops.attn_masked_on_mfma(40, 32)
    REACHED.update({("fwd", "f32"), ("bwd", "f32")})
    keep = torch.ones(B, 40, dtype=torch.uint8, device="cuda")
    q = c.qkv.cuda()
    o, lse2 = A.ops.attn_fwd_masked(q, keep, *c.dims, q_prescaled=True)
    _note("masked_f32", c, "fwd:f32", c.check_forward("masked_f32", dict(o=K.heads(o.cpu(), *c.dims), lse2=lse2.cpu()), rounded_l=False))
    dqkv = A.ops.attn_bwd_masked(q, K.packed(c.o_in).cuda(), c.d_o.cuda(), c.lse2_in.cuda(), keep, *c.dims, q_prescaled=True)
    dq, dk, dv = K.heads(dqkv.cpu(), *c.dims)
    _note("masked_f32", c, "bwd:f32", c.check_backward("masked_f32", dict(dq=dq, dk=dk, dv=dv)))


# ---------------------------------------------------------------------------------------------- coverage
def test_every_kernel_was_reached():
    """coverage by assertion: over this file the plan query has reported every forward and every backward value (runs last;
    needs the tests above to have run)"""
    want = {("fwd", k) for k in ("res8", "res12", "res_multi", "stream", "f32")}
    want |= {("bwd", k) for k in ("stream", "f32")}
    want |= {("bwd", "merged", kb, rg) for kb in (1, 2, 3, 4) for rg in (False, True)}
    want |= {("mx8", 1, False), ("mx8", 2, True), ("mx8", 2, False), ("mx8", 3, False)}
    assert want <= REACHED, sorted(want - REACHED, key=str)
    print("ATTNMAX " + json.dumps({f: {p: dict(ratio=v[0], case=v[1], group=v[2]) for p, v in parts.items()}
                                   for f, parts in sorted(MAXIMA.items())}))
