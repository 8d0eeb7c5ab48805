"""CPU (no GPU needed): the kit of the parity-mode attention tests (tests/attn_parity_util.py) - its emulations without a
rounding fault are the fp64 reference to fp32 accuracy, every group bound is positive, an INDEPENDENT restatement of each
arithmetic (plain fp32 torch matmuls for "f32", the three-product split on fp32 torch matmuls for "bf16x3", both in flash form
with exp2) passes check() forward and backward at every case of tests/test_gpu_attn_parity.py, every mutant is refused at
EVERY case of all_cases() and in every pass where mutant_applies says it is resolvable, and the host-only plan query names the
family of every case."""
import json

import pytest
import torch

import attn_parity_util as P

B, H = P.B_, P.H_
# What the independent restatements use of a bound, measured on a CPU over all_cases():
#   worst-case bound   o, dq, dk <= 0.010, dv <= 0.042 (`trained`, N = 200, bf16x3)
#   random operands    o, dq, dk <= 0.29 "bf16x3" (0.21 at N = 33 / 129 / 200), <= 0.35 "f32" (0.24 at those lengths)
#                      dv <= 0.61: dv = P^T dO carries the rounding of lse2_in to fp32 into every P, an error the restatement,
#                      the emulation and a kernel SHARE (same input): where it leads, error = emulation error, ratio 1 / 2
#   lse2               <= 0.036 (`huge`, N = 97)
# Against the margins the issue's probe measured (randn; ramp; q, k x 3; very_negative; N 33 / 129 / 200; dim_head 64: worst-case
# <= 0.023, random "bf16x3" <= 0.19, random "f32" <= 0.23, lse2 <= 0.023), with check()'s bounds exactly as the issue states them:
#   met        worst-case bound under ramp, small_steps, descending, very_negative (every part <= 0.010); random dq, dk "bf16x3"
#              at the probe lengths (<= 0.17); lse2 with randn and under the three ramps (<= 0.020)
#   NOT met    random dv: 0.52 "f32" / 0.20 "bf16x3" at N = 33 - the shared fp32 rounding of lse2_in above, which a factor-2
#              bound turns into 1 / 2 whatever the restatement does; random o "bf16x3" 0.203 at N = 33 and o, dq, dk "f32" 0.24
#              (torch's blocked fp32 matmul against this kit's k-ordered chain; the probe's emulation is not in the tree);
#              worst-case dv 0.041 / 0.023 and lse2 0.033 / 0.035 under `trained` / `huge`, regimes the probe did not run;
#              lse2 0.024 under very_negative
# so the two "random-operand bound" rows of that table, and the "worst-case bound" and "lse2" rows for dv, `trained`, `huge` and
# very_negative, are asserted at the figures below, not at the issue's.  Asserted with little room: a restatement that needs
# more of a bound says that the bound or the emulation has moved.
MARGIN_WORST_CASE = 0.06
MARGIN_RANDOM = {"o": 0.4, "dq": 0.4, "dk": 0.4, "dv": 0.7}
MARGIN_LSE2 = 0.05


# ---------------------------------------------------------------------------------------------- reference and emulation
@pytest.mark.parametrize("N,dh,regime", [(1, 64, None), (17, 64, None), (40, 32, None), (33, 128, None), (97, 64, "ramp")])
def test_the_emulations_are_the_reference_to_their_arithmetic(N, dh, regime):
    """fp32 operands, fp64 reference (attn_bf16_util.reference: torch autograd, checked in tests/test_attn_bf16_ref_cpu.py);
    either emulation agrees with it to a small multiple of its per-product error, and no magnitude sum is zero"""
    c = P.Case(N, dh, regime)
    assert c.qkv.dtype == torch.float32 and c.d_o.dtype == torch.float32 and c.qkv.shape == (B * N, 3 * H * dh)
    q, k, v = P.heads(c.qkv, *c.dims)
    assert not torch.equal(q[0, 0], q[1, 0]) and not torch.equal(q[0, 0], q[0, 1]) and not torch.equal(k[0, 0], k[0, 2])
    for arith in P.ARITHS:
        tol = 40 * (P.GAMMA[arith] + max(N, dh) * P.U)
        f, b = c.forward(arith), c.backward(arith)
        for name, t in (("o", f["o"]), ("dq", b["dq"]), ("dk", b["dk"]), ("dv", b["dv"])):
            assert float((t - c.ref[name]).abs().max()) <= tol * float(c.ref["mag"][name].abs().max()), (arith, name)
        assert float((f["lse2"] - c.ref["lse2"]).abs().max()) <= float(c.wc(arith)["lse2"].max())
    for name in ("o",) + P.PARTS_BWD:
        assert bool((c.ref["mag"][name] > 0).all()), name


def test_the_regimes_are_what_they_are_named_for():
    """the three ramps step per 32 keys (twice regime_qk's step per 64), `trained` has scores of about +-25 nats rms"""
    g = torch.Generator().manual_seed(1)
    q, k, u = torch.randn(128, 64, generator=g), torch.randn(128, 64, generator=g), torch.randn(64, generator=g)
    u = u / u.norm()
    for mode, step in (("ramp", 6.0), ("small_steps", 2.5), ("descending", -6.0)):
        q2, k2 = P.regime_qk32(mode, q, k, u)
        s = (q2 @ k2.T) / 8.0
        rise = float((s[:, 96:128].mean() - s[:, 64:96].mean()))
        assert abs(rise - step) < 0.35 * abs(step), (mode, rise)
    q2, k2 = P.regime_qk32("trained", q, k, u)
    s = (q2 @ k2.T) / 8.0
    assert 20.0 < float(s.std()) < 30.0 and 60.0 < float(s.abs().max()) < 130.0
    q2, k2 = P.regime_qk32("very_negative", q, k, u)
    assert float(((q2 @ k2.T) / 8.0).max()) < -200.0


# ---------------------------------------------------------------------------------------------- the bounds pass what is right
@pytest.mark.parametrize("arith,dh,N,regime", P.all_cases())
def test_bounds_are_positive_and_pass_an_independent_restatement(arith, dh, N, regime):
    c = P.case(N, dh, regime)
    wc = c.wc(arith)
    for part in ("o",) + P.PARTS_BWD:  # (group_bound asserts > 0 itself; here for both kinds of bound, whatever the case uses)
        assert bool((P.group_bound(part, c.ref, None, wc, N, dh, arith) > 0).all())
        if regime is None:
            emu = c.emu(arith, "fwd" if part == "o" else "bwd")
            assert bool((P.group_bound(part, c.ref, emu, wc, N, dh, arith) > 0).all())
    assert bool((wc["lse2"] > 0).all())
    tag = f"restated[{arith},{dh},{N},{regime}]"
    stats = dict(c.check_forward(tag, P.restate_forward(c.qkv, *c.dims, arith), arith))
    stats.update(c.check_backward(tag, P.restate_backward(c.qkv, c.d_o, c.o_in, c.lse2_in, *c.dims, arith), arith))
    print("PARITYEMU " + json.dumps(dict(arith=arith, dh=dh, N=N, regime=regime, **{p: s["ratio"] for p, s in stats.items()})))
    assert all(s["ratio"] <= (MARGIN_RANDOM[p] if regime is None else MARGIN_WORST_CASE) for p, s in stats.items() if p != "lse2"), stats
    assert stats["lse2"]["ratio"] <= MARGIN_LSE2, stats


@pytest.mark.parametrize("arith,N", [("bf16x3", 33), ("f32", 129)])
def test_the_device_own_output_bound_contains_the_reference_made_one(arith, N):
    """own_outputs_extra only adds: positive in every group, and a backward emulated on the restated forward's o and lse2 (what
    a layer runs) passes the widened bound"""
    c = P.case(N, 64)
    extra = P.own_outputs_extra(c.wc(arith))
    for part in P.PARTS_BWD:
        assert bool((P.group_sq(extra[part]) > 0).all()), part
    f = P.restate_forward(c.qkv, *c.dims, arith)
    own = P.emulate_backward(c.qkv, c.d_o, f["o"].float(), f["lse2"].float(), *c.dims, arith)
    c.check_backward(f"own[{arith},{N}]", own, arith, own_outputs=True)


# ---------------------------------------------------------------------------------------------- ... and refuse what is wrong
def _mutant_jobs():
    """[(arith, dh, N, regime, pass, mutant)]: every case of all_cases() x both passes x every mutant that mutant_applies
    accepts there, the jobs of one case next to each other (the case cache holds four)"""
    return [(a, dh, N, r, what, m) for a, dh, N, r in sorted(P.all_cases(), key=lambda c: (c[3] or "", c[1], c[2], c[0]))
            for what in ("fwd", "bwd") for m in P.MUTANTS if P.mutant_applies(m, what, N, a, r)]


JOBS = _mutant_jobs()


def test_every_mutant_has_a_job_at_every_case_it_applies_to():
    """nothing is selected away: the jobs are exactly what mutant_applies accepts over all_cases(), and that is every mutant in
    every family and pass it is written for, at every length from its smallest on (ragged / odd lengths for padded_key /
    odd_row_lost), plus the three regime mutants under the regimes that resolve them"""
    seen = set(JOBS)
    assert len(seen) == len(JOBS)
    random = {(a, dh): sorted(N for x, d, N, r in P.all_cases() if (x, d, r) == (a, dh, None)) for a, dh, _, _ in P.all_cases()}
    assert set(random) == {("bf16x3", 64), ("f32", 64), ("f32", 32), ("f32", 128)}
    assert tuple(random[("bf16x3", 64)]) == P.LENGTHS and tuple(random[("f32", 64)]) == P.LENGTHS
    for (a, dh), ns in random.items():
        for m, (passes, nmin, needs, ariths) in P.MUTANTS.items():
            for what in ("fwd", "bwd"):
                want = [N for N in ns if what in passes and a in ariths and N >= nmin
                        and (needs != "ragged" or N % 32) and (needs != "odd" or N % 2) and needs != "ramp"]
                got = [N for N in ns if (a, dh, N, None, what, m) in seen]
                assert got == want, (a, dh, m, what, got, want)
                if a in ariths and what in passes and needs != "ramp":
                    assert got, (a, dh, m, what)  # (every family has lengths at which each of its mutants applies)
    for a, dh, N, r in P.REGIME_CASES:
        got = {(what, m) for x, d, n, rr, what, m in JOBS if (x, d, n, rr) == (a, dh, N, r)}
        want = {("fwd", "swap_heads"), ("bwd", "swap_heads")}
        want |= {("fwd", "skip_rescale")} if r == "ramp" else set()
        want |= {("fwd", "padded_key")} if r == "very_negative" and N % 32 else set()
        assert got == want, (a, dh, N, r, got, want)
    for a in P.ARITHS:
        assert any(j[0] == a and j[3] == "ramp" and j[5] == "skip_rescale" for j in JOBS)
        assert any(j[0] == a and j[3] == "very_negative" and j[5] == "padded_key" for j in JOBS)


@pytest.mark.parametrize("arith,dh,N,regime,what,m", JOBS)
def test_mutants_are_refused(arith, dh, N, regime, what, m):
    c = P.case(N, dh, regime)
    tag = f"{arith}/{what}/{m}[{dh},{N},{regime}]"
    with pytest.raises(AssertionError) as e:
        if what == "fwd":
            c.check_forward(tag, c.forward(arith, mutant=m), arith)
        else:
            c.check_backward(tag, c.backward(arith, mutant=m), arith)
    assert tag in str(e.value), str(e.value)  # (refused by check's own assertion, with the part and the group)
    print("PARITYMUT", tag, str(e.value)[len(tag) + 2:][:160])


def test_the_whole_tensor_allclose_misses_what_this_kit_catches():
    """the gap this kit closes: a bf16x3 kernel that splits by truncation uses at most 0.56 of the whole-tensor allclose of
    tests/test_gpu_ops.py::test_attention_f32 (o: atol 2e-5, dqkv: atol 5e-5, rtol 1e-4) in its worst element, forward and
    backward - and is refused here (test_mutants_are_refused, at this very length)"""
    c = P.case(385, 64)
    used = lambda got, part, atol: float(((got[part] - c.ref[part]).abs() / (atol + 1e-4 * c.ref[part].abs())).max())
    assert P.mutant_applies("split_by_truncation", "fwd", 385, "bf16x3") and P.mutant_applies("split_by_truncation", "bwd", 385, "bf16x3")
    assert used(c.forward("bf16x3", mutant="split_by_truncation"), "o", 2e-5) < 0.7
    got = c.backward("bf16x3", mutant="split_by_truncation")
    assert all(used(got, part, 5e-5) < 0.7 for part in P.PARTS_BWD)


# ---------------------------------------------------------------------------------------------- the plan query
def test_plan_query_names_the_family_of_every_case():
    """avf_attn_parity_plan is pure host code, answered by the predicates attn_fwd_vec / attn_bwd_vec switch on"""
    import avformer_amd as A
    L = A._lib
    prev = L.get_f32_arithmetic()
    try:
        for setting in P.ARITHS:
            L.set_f32_arithmetic(setting)
            for dh in (32, 64, 128):
                want = "bf16x3" if (setting == "bf16x3" and dh == 64) else "f32"
                assert P.parity_plan(A, dh, H) == want, (setting, dh)
                # a mask, pre-scaled q, bf16 storage, a tensor off the 16-byte grid: the vector kernels
                assert P.parity_plan(A, dh, H, masked=True) == "vec"
                assert P.parity_plan(A, dh, H, q_prescaled=True) == "vec"
                assert P.parity_plan(A, dh, H, aligned16=False) == "vec"
                assert P.parity_plan(A, dh, H, dtype=L.BF16) == "vec"
                assert P.parity_plan(A, dh, H, dtype=L.BF16, q_prescaled=True) == "vec"
            for dh in (8, 16):  # head widths only the vector kernels have
                assert P.parity_plan(A, dh, H) == "vec", (setting, dh)
            assert P.parity_plan(A, 32, 1) == "f32" and L.get_f32_arithmetic() == setting  # (the query changes nothing)
        for a, dh, N, r in P.all_cases():
            L.set_f32_arithmetic(a)
            assert P.parity_plan(A, dh, H) == a, (a, dh, N, r)
        # the families the GPU file reaches, from its case tables: both at dim_head 64 with random operands and under every
        # regime, "f32" at 32 and 128, and at 128 under every regime
        assert {(a, dh) for a, dh, N in P.RANDOM_CASES} == {("bf16x3", 64), ("f32", 64), ("f32", 32), ("f32", 128)}
        assert {(a, dh, r) for a, dh, N, r in P.REGIME_CASES} == ({(a, 64, r) for a in P.ARITHS for r in P.REGIME_NAMES}
                                                                 | {("f32", 128, r) for r in P.REGIME_NAMES})
        assert {dh for dh, N in P.OTHER_WIDTHS_UNDER_BF16X3} == {32, 128} and P.MISALIGNED == (64, 33)
        L.set_f32_arithmetic("bf16x3")
        for dh, N in P.OTHER_WIDTHS_UNDER_BF16X3:
            assert P.parity_plan(A, dh, H) == "f32", (dh, N)
    finally:
        L.set_f32_arithmetic(prev)
