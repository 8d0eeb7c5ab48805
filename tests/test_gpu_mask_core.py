"""-m gpu: the masked attention core AS A BF16 LAYER RUNS IT (avf_attn_fwd_masked_qs / avf_attn_bwd_masked_qs: the same helper
picks the kernels for avf_layer_fwd / avf_layer_bwd), against the fp64 reference of tests/mask_attn_util.py.

dim_head 64 and up to 512 tokens: attn_fwd_res_kernel<8 | 12 | 8-multi, qs, mask> and attn_bwd_m4_kernel<KB = 1..4, ragged,
mask>; everything else: the fp32-arithmetic kernels of attn_f32.hip on bf16 storage with pre-scaled q.  B = 2, H = 2; clip 0
carries the named keep pattern, clip 1 a random one with token 0 dropped.  Errors are taken per ROW GROUP (kept tokens, dropped
tokens; all clips and clip 0 alone): a dropped query's output row is the mean of v and its norm about 1/sqrt(N) of a kept
row's, so a whole-tensor error cannot see it.  Caps: mask_attn_util (the project's own figures for these kernels; none comes
from what the kernels produce); tests/test_mask_attn_ref_cpu.py shows that bf16 rounding alone takes under a fifth of each.
The unmasked instantiations of the same kernels: tests/test_gpu_attn_bf16.py (16 x 16 groups against an emulation of the
rounding points, the backward on reference-made inputs)."""
import functools
import math

import pytest
import torch

import mask_attn_util as M
from gpu_util import DEV, check, rel_fro

pytestmark = pytest.mark.gpu

B, H = M.B_, M.H_


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


@functools.lru_cache(maxsize=None)
def _case(N, dh, pattern, regime=None, hidden=False):
    """operands and fp64 reference of one case, computed once (treated as read-only by every test)"""
    qkv, d_o, keep = M.case_inputs(N, dh, pattern, regime)
    if hidden:
        qkv = M.hide_dropped(qkv, keep, H, dh)
    return qkv, d_o, keep, M.reference(qkv, keep, B, N, H, dh, d_o)


def _run(ops, qkv, d_o, keep, N, dh):
    q, g, m = qkv.to(DEV), d_o.to(DEV), keep.to(DEV)
    o, lse2 = ops.attn_fwd_masked(q, m, B, N, H, dh, q_prescaled=True)
    dqkv = ops.attn_bwd_masked(q, o, g, lse2, m, B, N, H, dh, q_prescaled=True)
    torch.cuda.synchronize()
    return o.cpu(), lse2.cpu(), dqkv.cpu()


def _check(tag, out, ref, keep, N, dh, mfma, regime=False):
    o, lse2, dqkv = out
    I = H * dh
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse2).all()) and bool(torch.isfinite(dqkv.float()).all()), tag
    eo = M.grouped_errors(o, ref["o"], keep, {"o": slice(None)})
    eg = M.grouped_errors(dqkv, ref["dqkv"], keep, {"dqkv": slice(None)} if regime else M.grad_parts(H, dh))
    kept_q = keep[:, None, :].expand(B, H, N)
    lse_err = float((lse2[kept_q].double() - ref["lse2"][kept_q]).abs().max()) if bool(keep.any()) else 0.0
    print(tag, {f"{p}:{g}": f"{k} {e:.3e}" for (p, g), (k, e) in sorted({**eo, **eg}.items())}, f"lse2 kept max |err| {lse_err:.3e}")
    M.assert_grouped(tag, eo, M.CAP_O, check)
    M.assert_grouped(tag, eg, M.CAP_DQKV_REGIME if regime else M.CAP_GRAD, check)
    # a dropped query passes no gradient to q, and a dropped key receives none into k: exactly
    rows = ~keep.reshape(-1)
    assert bool((dqkv[rows][:, :2 * I].float() == 0).all()), f"{tag}: dq / dk of a dropped token is not exactly 0"
    if mfma and bool(rows.any()):  # the contract the merged backward relies on (attn_bf16.hip, at attn_fwd_res_kernel)
        torch.testing.assert_close(lse2[~kept_q], torch.full_like(lse2[~kept_q], math.log2(N)), rtol=1e-5, atol=0.0)
    if bool(keep.any()):
        torch.testing.assert_close(lse2[kept_q], ref["lse2"][kept_q].float(), **(M.LSE_TOL_REGIME if regime else M.LSE_TOL))


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("N,pattern", M.CASES_MFMA)
def test_mfma_lengths_and_patterns(ops, N, pattern):
    """every tile edge of the two kernels (32-row query groups, 64-key tiles; forward builds change at 256 | 257 and 384 | 385,
    the backward's KB at 128 | 129, 256 | 257, 384 | 385) x every keep pattern that fits, token 0 dropped, tiles without a kept
    key and wholly dropped clips among them"""
    assert ops.attn_masked_on_mfma(N, 64)
    qkv, d_o, keep, ref = _case(N, 64, pattern)
    _check(f"mcore[{N},{pattern}]", _run(ops, qkv, d_o, keep, N, 64), ref, keep, N, 64, mfma=True)


# ---------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("N,dh,pattern", M.CASES_VEC)
def test_fallback_boundary_and_prescaled_vector_path(ops, N, dh, pattern):
    """past 512 tokens and at dim_head 32 / 128 the layer runs the fp32-arithmetic kernels with pre-scaled q (they document no
    lse2 for a dropped query: finite)"""
    assert not ops.attn_masked_on_mfma(N, dh)
    qkv, d_o, keep, ref = _case(N, dh, pattern)
    _check(f"mcore_vec[{N},{dh},{pattern}]", _run(ops, qkv, d_o, keep, N, dh), ref, keep, N, dh, mfma=False)


# ---------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("N,regime,pattern", M.CASES_REGIME)
def test_score_regimes_under_a_mask(ops, N, regime, pattern):
    """the rescale paths of the masked forward (12-wave and multi-pass builds; KB 3 and 4): the first finite score a row sees
    may be far below zero and may arrive in a later tile"""
    assert ops.attn_masked_on_mfma(N, 64)
    qkv, d_o, keep, ref = _case(N, 64, pattern, regime)
    _check(f"mcore_reg[{N},{regime},{pattern}]", _run(ops, qkv, d_o, keep, N, 64), ref, keep, N, 64, mfma=True, regime=True)


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("N,pattern", M.CASES_HIDDEN)
def test_dropped_tokens_cannot_be_seen(ops, N, pattern):
    """q and k of every dropped token replaced by x * 40 + 7: discarded scores reach thousands of nats, far above any kept
    row's lse - a kernel that forms exp2(s - lse2) before discarding it makes inf * 0.  Nothing may change, bit for bit."""
    assert ops.attn_masked_on_mfma(N, 64)
    qkv, d_o, keep, ref = _case(N, 64, pattern)
    qkv2, _, _, ref2 = _case(N, 64, pattern, None, True)
    assert ref2["max_discarded"] > 1e3
    a = _run(ops, qkv, d_o, keep, N, 64)
    b = _run(ops, qkv2, d_o, keep, N, 64)
    _check(f"mcore_hid[{N},{pattern}]", b, ref2, keep, N, 64, mfma=True)
    for name, x, y in zip(("o", "lse2", "dqkv"), a, b):
        assert torch.equal(x, y), f"{name} depends on the q / k of dropped tokens: max |diff| {(x.float() - y.float()).abs().max():.3e}"
    _check(f"mcore[{N},{pattern}]", a, ref, keep, N, 64, mfma=True)


# ---------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("N", M.LENGTHS_ALL_KEPT)
def test_all_kept_equals_no_mask(ops, N):
    """an all-ones keep against the unmasked kernels on the same operands: two bf16 roundings apart (4e-3, the figure of
    test_gemm_bf16_nt), lse2 within 1e-4"""
    qkv, d_o, keep, _ = _case(N, 64, "all_kept")
    keep = torch.ones_like(keep)
    o, lse2, dqkv = _run(ops, qkv, d_o, keep, N, 64)
    q = qkv.to(DEV)
    o_u, lse_u = ops.attn_fwd(q, B, N, H, 64, q_prescaled=True)
    dqkv_u = ops.attn_bwd(q, o_u, d_o.to(DEV), lse_u, B, N, H, 64, q_prescaled=True)
    check(f"mcore_allkept[{N}]:o", rel_fro(o, o_u), 4e-3)
    check(f"mcore_allkept[{N}]:dqkv", rel_fro(dqkv, dqkv_u), 4e-3)
    torch.testing.assert_close(lse2, lse_u.cpu(), atol=1e-4, rtol=0.0)
