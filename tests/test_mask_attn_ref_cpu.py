"""No GPU: the masked-attention test kit of tests/mask_attn_util.py is shown to be right and to bite.  Its fp64 reference agrees
with the oracle's masked attention (the code the g13 goldens validate); every mask builder produces what its name says; for
every case of tests/test_gpu_mask_core.py the reference merely ROUNDED to bf16 stays within a fifth of every cap, in every row
group (so a cap is never spent on the format alone); the reference cannot see the q and k of a dropped token; and the grouped
error catches a fault that lives in the dropped rows only, which a whole-tensor error does not."""
import math

import pytest
import torch

import mask_attn_util as M
import oracle

B, H = M.B_, M.H_


def _keep_of(pattern, N, seed=3):
    return M.make_keep(pattern, B, N, seed)


# ---------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("N,dh,pattern", [(40, 64, "random30"), (130, 64, "all_kept"), (70, 32, "last_only"), (33, 128, "random30")])
def test_reference_agrees_with_the_oracle(N, dh, pattern):
    """the oracle pads its mask with a leading True, so token 0 is kept here"""
    qkv, d_o = M.make_operands(B, N, H, dh, seed=N + dh)
    keep = _keep_of(pattern, N)
    keep[:, 0] = True
    ref = M.reference(qkv, keep, B, N, H, dh, d_o)
    I = H * dh
    x = qkv.double()
    x[:, :I] = x[:, :I] / (M.LOG2E / math.sqrt(dh))
    x.requires_grad_(True)
    o = oracle.attention_forward(x.view(B, N, 3 * I), torch.eye(3 * I, dtype=torch.float64), None, None, H, mask=keep[:, 1:])
    o.reshape(B * N, I).backward(d_o.double())
    torch.testing.assert_close(ref["o"], o.detach().reshape(B * N, I), atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(ref["dqkv"], x.grad, atol=1e-12, rtol=1e-12)


def test_reference_rows_of_dropped_and_kept_queries():
    N, dh = 70, 64
    qkv, d_o = M.make_operands(B, N, H, dh, seed=5)
    keep = _keep_of("token0_dropped", N)
    ref = M.reference(qkv, keep, B, N, H, dh, d_o)
    I = H * dh
    v = qkv.double()[:, 2 * I:].view(B, N, I)
    o = ref["o"].view(B, N, I)
    dq, dk, dv = [t.view(B, N, I) for t in ref["dqkv"].split(I, dim=-1)]
    torch.testing.assert_close(o[~keep], v.mean(1, keepdim=True).expand(B, N, I)[~keep], atol=1e-13, rtol=1e-12)
    assert bool((dq[~keep] == 0).all()) and bool((dk[~keep] == 0).all())
    # a dropped key receives d_o / N from every dropped query and nothing else
    g = d_o.double().view(B, N, I)
    share = (g * (~keep)[:, :, None]).sum(1, keepdim=True) / N
    torch.testing.assert_close(dv[~keep], share.expand(B, N, I)[~keep], atol=1e-13, rtol=1e-12)
    # lse2 of a kept query: log2 of the sum over the kept keys
    q = qkv.double()[:, :I].view(B, N, H, dh)[0, :, 0]           # (pre-scaled: the dot product is the log2-domain score)
    k = qkv.double()[:, I:2 * I].view(B, N, H, dh)[0, :, 0]
    i = int(keep[0].nonzero()[0])
    s2 = (k[keep[0]] @ q[i])
    assert float(ref["lse2"][0, 0, i]) == pytest.approx(float(torch.log2(torch.exp2(s2).sum())), rel=1e-12)


# ---------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("N", [1, 2, 65, 129, 324, 512])
def test_builders_produce_what_their_names_say(N):
    for name in M.patterns_for(N):
        keep = _keep_of(name, N)
        assert keep.shape == (B, N) and keep.dtype == torch.bool
        m = keep[0]
        assert not keep[1, 0], "clip 1 drops token 0"
        if name == "all_kept":
            assert bool(m.all())
        elif name == "none_kept":
            assert not bool(m.any())
        elif name == "token0_dropped":
            assert not m[0]
        elif name == "last_only":
            assert m.nonzero().flatten().tolist() == [N - 1]
        elif name == "one_in_the_middle":
            assert m.nonzero().flatten().tolist() == [N // 2]
        elif name == "alternating":
            assert m.tolist() == [i % 2 == 1 for i in range(N)]
        elif name == "first_tile_dropped":   # the 64-key tile 0 holds no kept key, a later one does
            assert not bool(m[:64].any()) and bool(m[64:].any())
        elif name == "middle_tile_dropped":  # tile 1 holds none, tiles 0 and 2 do
            assert not bool(m[64:128].any()) and bool(m[:64].any()) and bool(m[128:].any())
    assert ("first_tile_dropped" in M.patterns_for(N)) == (N > 64)
    assert ("middle_tile_dropped" in M.patterns_for(N)) == (N > 128)


def test_random30_drops_about_30_percent():
    keep = M.make_keep("random30", 8, 512, seed=1)
    assert 0.25 < float((~keep).float().mean()) < 0.35


def test_the_case_lists_are_what_the_gpu_file_is_meant_to_run():
    assert len(M.CASES_MFMA) == sum(len(M.patterns_for(N)) for N in M.LENGTHS_MFMA)
    assert {p for N, p in M.CASES_MFMA if N == 512} == set(M.PATTERNS)
    assert {p for N, p in M.CASES_MFMA if N == 64} == set(M.PATTERNS) - {"first_tile_dropped", "middle_tile_dropped"}
    assert all(M.fits(p, N) for N, r, p in M.CASES_REGIME) and all(M.fits(p, N) for N, p in M.CASES_HIDDEN)
    assert len(M.CASES_VEC) == 21 and len(M.CASES_REGIME) == 24 and len(M.CASES_HIDDEN) == 8


# ---------------------------------------------------------------------------------------------- caps against the format
def _rounded_reference_within_a_fifth(tag, N, dh, pattern, regime=None):
    qkv, d_o, keep = M.case_inputs(N, dh, pattern, regime)
    ref = M.reference(qkv, keep, B, N, H, dh, d_o)
    assert torch.isfinite(ref["o"]).all() and torch.isfinite(ref["dqkv"]).all()
    rnd = lambda t: t.to(torch.bfloat16)
    M.assert_grouped(tag, M.grouped_errors(rnd(ref["o"]), ref["o"], keep, {"o": slice(None)}), M.CAP_O / 5)
    if regime is None:
        M.assert_grouped(tag, M.grouped_errors(rnd(ref["dqkv"]), ref["dqkv"], keep, M.grad_parts(H, dh)), M.CAP_GRAD / 5)
    else:
        M.assert_grouped(tag, M.grouped_errors(rnd(ref["dqkv"]), ref["dqkv"], keep, {"dqkv": slice(None)}), M.CAP_DQKV_REGIME / 5)


@pytest.mark.parametrize("N", M.LENGTHS_MFMA)
def test_rounded_reference_is_within_a_fifth_of_the_caps_mfma_cases(N):
    for n, p in M.CASES_MFMA:
        if n == N:
            _rounded_reference_within_a_fifth(f"a[{N},{p}]", N, 64, p)


def test_rounded_reference_is_within_a_fifth_of_the_caps_other_cases():
    for N, dh, p in M.CASES_VEC:
        _rounded_reference_within_a_fifth(f"b[{N},{dh},{p}]", N, dh, p)
    for N, r, p in M.CASES_REGIME:
        _rounded_reference_within_a_fifth(f"c[{N},{r},{p}]", N, 64, p, r)
    for N, p in M.CASES_HIDDEN:
        _rounded_reference_within_a_fifth(f"d[{N},{p}]", N, 64, p)


def test_rounded_reference_figures_of_one_case():
    """B = 2, N = 130, H = 2, 30 % dropped with a dropped first tile: about 1.6e-3 in all four groups of o and dv"""
    N, dh = 130, 64
    qkv, d_o, keep = M.case_inputs(N, dh, "first_tile_dropped")
    ref = M.reference(qkv, keep, B, N, H, dh, d_o)
    e = M.grouped_errors(ref["o"].to(torch.bfloat16), ref["o"], keep, {"o": slice(None)})
    e.update(M.grouped_errors(ref["dqkv"].to(torch.bfloat16), ref["dqkv"], keep, {"dv": M.grad_parts(H, dh)["dv"]}))
    for part in ("o", "dv"):
        for grp in ("kept", "dropped"):
            kind, v = e[(part, grp)]
            assert kind == "rel" and 1.2e-3 < v < 2.0e-3, (part, grp, v)


# ---------------------------------------------------------------------------------------------- dropped tokens cannot be seen
@pytest.mark.parametrize("N,pattern", M.CASES_HIDDEN)
def test_reference_is_bit_invariant_under_the_q_and_k_of_dropped_tokens(N, pattern):
    dh = 64
    qkv, d_o, keep = M.case_inputs(N, dh, pattern)
    a = M.reference(qkv, keep, B, N, H, dh, d_o)
    b = M.reference(M.hide_dropped(qkv, keep, H, dh), keep, B, N, H, dh, d_o)
    I = H * dh
    flat = keep.reshape(-1)
    assert torch.equal(a["o"], b["o"])
    assert torch.equal(a["dqkv"][:, 2 * I:], b["dqkv"][:, 2 * I:])
    assert torch.equal(a["dqkv"][flat], b["dqkv"][flat])
    assert bool((b["dqkv"][~flat][:, :2 * I] == 0).all())
    kept_q = keep[:, None, :].expand(B, H, N)
    assert torch.equal(a["lse2"][kept_q], b["lse2"][kept_q])
    # ... although the discarded scores tower over everything a kept row sees
    assert b["max_discarded"] > 1e3 and float(a["lse2"][kept_q].max()) / M.LOG2E < 20.0, (b["max_discarded"], a["lse2"][kept_q].max())


# ---------------------------------------------------------------------------------------------- the grouped error bites
def test_grouped_error_sees_what_a_whole_tensor_error_hides():
    """every dropped query's output row wrong by 5 % in every element, under peaked attention (a kept row has about the norm
    of one v row, a dropped one 1/sqrt(N) of it): the whole-tensor error stays under 1e-2, the dropped group's is 0.05"""
    N, dh = 324, 64
    qkv, d_o, keep = M.case_inputs(N, dh, "random30", "ramp")
    ref = M.reference(qkv, keep, B, N, H, dh, d_o)
    wrong = ref["o"].clone()
    wrong[~keep.reshape(-1)] *= 1.05
    whole = float((wrong - ref["o"]).norm() / ref["o"].norm())
    assert whole < 1e-2, whole
    errs = M.grouped_errors(wrong, ref["o"], keep, {"o": slice(None)})
    assert errs[("o", "kept")][1] == 0.0 and errs[("o", "dropped")][1] == pytest.approx(0.05), errs
    with pytest.raises(AssertionError, match="o:dropped"):
        M.assert_grouped("t", errs, M.CAP_O)


def test_grouped_error_zero_reference_and_empty_groups():
    N, dh = 40, 64
    qkv, d_o, keep = M.case_inputs(N, dh, "last_only")
    ref = M.reference(qkv, keep, B, N, H, dh, d_o)
    errs = M.grouped_errors(ref["dqkv"], ref["dqkv"], keep, M.grad_parts(H, dh))
    assert errs[("dq", "dropped")] == ("abs", 0.0) and errs[("dk", "dropped")] == ("abs", 0.0)
    assert errs[("dq", "kept0")] == ("abs", 0.0)       # clip 0 keeps one key: p = 1, dS = 0
    assert errs[("dv", "kept0")] == ("rel", 0.0)
    leaky = ref["dqkv"].clone()
    leaky[~keep.reshape(-1), :H * dh] = 0.02
    with pytest.raises(AssertionError, match="reference is 0"):
        M.assert_grouped("t", M.grouped_errors(leaky, ref["dqkv"], keep, M.grad_parts(H, dh)), M.CAP_GRAD)
    nan = ref["dqkv"].clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        M.assert_grouped("t", M.grouped_errors(nan, ref["dqkv"], keep, M.grad_parts(H, dh)), M.CAP_GRAD)
    all_kept = M.make_keep("all_kept", 1, N)
    assert set(M.row_groups(all_kept)) == {"kept", "kept0"}
    assert set(M.row_groups(M.make_keep("none_kept", 1, N))) == {"dropped", "dropped0"}


# ---------------------------------------------------------------------------------------------- the dispatch predicate (host code)
def test_case_lists_sit_on_the_intended_side_of_the_dispatch():
    """avf_attn_masked_on_mfma is pure host code: every (a) / (c) / (d) / (e) length runs the masked MFMA kernels, every (b) shape
    the fp32-arithmetic ones, and the boundary is 512 | 513 at dim_head 64"""
    import avformer_amd as A
    A._build.build()
    on = A.ops.attn_masked_on_mfma
    assert all(on(N, 64) for N in M.LENGTHS_MFMA + M.LENGTHS_ALL_KEPT)
    assert all(on(N, 64) for N, _, _ in M.CASES_REGIME) and all(on(N, 64) for N, _ in M.CASES_HIDDEN)
    assert not any(on(N, dh) for N, dh in M.SHAPES_VEC)
    assert on(512, 64) and not on(513, 64) and not on(512, 32) and not on(512, 128)
