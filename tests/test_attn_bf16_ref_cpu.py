"""CPU (no GPU needed): the kit of the unmasked bf16 attention tests (tests/attn_bf16_util.py) - its fp64 reference is torch
autograd, its groups partition every tensor, its bounds pass a correct bf16 rounding in two associations at every case of
tests/test_gpu_attn_bf16.py and refuse every mutant at the smallest and the largest length of each kernel family, and the
host-only plan query names the kernel each case was written for."""
import json

import pytest
import torch
import torch.nn.functional as F

import attn_bf16_util as K

B, H = K.B_, K.H_


# ---------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("N,dh,qs", [(1, 64, 1), (17, 64, 1), (40, 32, 0), (33, 128, 1)])
def test_reference_equals_torch_autograd_and_the_closed_form(N, dh, qs):
    c = K.Case(N, dh, qs)
    q, k, v = [t.clone().requires_grad_(True) for t in K.heads(c.proj, B, N, H, dh)]
    o = F.scaled_dot_product_attention(q, k, v)  # fp64, scale dh^-1/2
    g = K.heads(c.d_o.double(), B, N, H, dh)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), g)
    for name, t in (("o", o.detach()), ("dq", dq), ("dk", dk), ("dv", dv)):
        torch.testing.assert_close(c.ref[name], t, rtol=1e-11, atol=1e-12, msg=lambda m: f"{name}: {m}")
    # the emulations without their rounding points are the reference again, in either association
    for assoc in ("normalised", "unnormalised"):
        f = c.forward(assoc, rounding=False)
        torch.testing.assert_close(f["o"], c.ref["o"], rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(f["lse2"], c.ref["lse2"], rtol=1e-12, atol=1e-12)
        b = K.emulate_backward(c.proj, c.d_o, c.ref["o"], c.ref["lse2"], *c.dims, assoc=assoc, rounding=False)
        for name in K.PARTS_BWD:
            torch.testing.assert_close(b[name], c.ref[name], rtol=1e-10, atol=1e-12, msg=lambda m: f"{name}: {m}")
    for name in ("o",) + K.PARTS_BWD:  # a magnitude dominates its sum and is positive everywhere
        assert bool((c.ref["mag"][name] > 0).all()) and bool((c.ref["mag"][name] >= c.ref[name].abs() * (1 - 1e-12)).all()), name
    if N == 1:
        assert float(c.ref["dq"].abs().max()) == 0.0 and float(c.ref["dk"].abs().max()) == 0.0


def test_prescaled_operands_stand_for_the_same_projection():
    """the fp64 projection undoes the factor of the stored q' exactly: q' = proj_q * c to fp64 rounding, k and v untouched"""
    qkv, d_o, proj = K.make_operands(B, 20, H, 64, 5, qs=1)
    I = H * 64
    c = K.LOG2E / 8.0
    torch.testing.assert_close(proj[:, :I] * c, qkv[:, :I].double(), rtol=1e-15, atol=0.0)
    assert torch.equal(proj[:, I:], qkv[:, I:].double())
    raw = K.make_operands(B, 20, H, 64, 5, qs=0)
    assert torch.equal(raw[2], raw[0].double()) and torch.equal(raw[1], d_o)
    a, b = K.heads(proj, B, 20, H, 64)[0], K.heads(proj, B, 20, H, 64)[1]
    assert not torch.equal(a[0, 0], a[1, 0]) and not torch.equal(a[0, 0], a[0, 1]) and not torch.equal(b[0, 0], b[0, 2])


# ---------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("N", [1, 7, 8, 15, 16, 17, 23, 24, 33, 129, 577])
@pytest.mark.parametrize("dh", [32, 128])
def test_groups_partition_every_tensor(N, dh):
    ids = K.group_ids(B, H, N, dh)
    rb, nblk = K.row_blocks(N)
    assert ids.shape == (B, H, N, dh)
    n_groups = B * H * nblk * (dh // 16)
    assert sorted(ids.unique().tolist()) == list(range(n_groups))  # every element in exactly one group, none empty
    rows = torch.bincount(rb, minlength=nblk)
    assert int(rows.sum()) == N and int(rows.max()) <= 23 and (N < 8 or int(rows.min()) >= 8)
    assert N < 16 or bool((rows[:-1] == 16).all())
    x = torch.randn(B, H, N, dh, generator=torch.Generator().manual_seed(N))
    want = torch.zeros(n_groups, dtype=torch.float64).index_add_(0, ids.reshape(-1), x.double().reshape(-1) ** 2)
    torch.testing.assert_close(K.group_sq(x).reshape(-1), want, rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------------------------------------- the bounds pass what is right
def _rounded_l(N, dh):
    return dh == 64 and N <= 576  # the head-resident forward (attn_bf16.hip: use_resident)


@pytest.mark.parametrize("N,dh,qs,regime", K.all_cases())
def test_clean_emulations_pass(N, dh, qs, regime):
    """the clean emulation and the comparison association (unnormalised P against the row maximum, divided by l afterwards;
    dS from the rounded P) at every case of the GPU file"""
    c = K.case(N, dh, qs, regime)
    rl = _rounded_l(N, dh)
    stats = {}
    for assoc in ("normalised", "unnormalised"):
        f = c.forward(assoc, rounded_l=rl)
        stats[assoc] = dict(c.check_forward(f"{assoc}[{N},{dh},{qs},{regime}]", f, rl))
        stats[assoc].update(c.check_backward(f"{assoc}[{N},{dh},{qs},{regime}]", c.backward(assoc)))
    print("ATTNEMU " + json.dumps(dict(N=N, dh=dh, qs=qs, regime=regime, **{a: {p: s["ratio"] for p, s in st.items()}
                                                                             for a, st in stats.items()})))
    if regime is None:  # the clean emulation sits at 1 / 2 by construction; the comparison passed check() above: o stays below
        # 0.55, dq and dk - which here carry one rounding MORE than any kernel, dS from the rounded P - reach 0.95 at N = 576
        assert all(s["ratio"] <= 0.5 + 1e-9 for p, s in stats["normalised"].items() if p != "lse2")
        assert stats["unnormalised"]["o"]["ratio"] <= 0.7
    else:  # the worst case of three roundings is far above what round-to-nearest does on average
        assert all(s["ratio"] <= 0.15 for p, s in stats["unnormalised"].items() if p != "lse2")


# ---------------------------------------------------------------------------------------------- ... and refuse what is wrong
# kernel family -> (dim_head, qs, its lengths in the GPU file, l sums the rounded P)
FAMILIES_FWD = {
    **{f"fwd_{k}": (64, 1, ns, k != "stream") for k, ns in K.FWD_QS.items()},
    "fwd_stream32": (32, 1, tuple(N for dh, N in K.FWD_DH if dh == 32), False),
    "fwd_stream128": (128, 1, tuple(N for dh, N in K.FWD_DH if dh == 128), False),
    "fwd_raw_res": (64, 0, tuple(N for dh, N, k in K.FWD_RAW if k != "stream"), True),
}
FAMILIES_BWD = {
    **{f"bwd_merged_kb{kb}": (64, 1, ns) for kb, ns in K.BWD_MERGED.items()},
    "bwd_stream64_qs_res_fwd": (64, 1, K.BWD_STREAM64_RES_FWD[1]),
    "bwd_stream64_raw_res_fwd": (64, 0, K.BWD_STREAM64_RES_FWD[0]),
    "bwd_stream64_qs": (64, 1, (577, 640, 641)), "bwd_stream64_raw": (64, 0, (577, 640, 641)),
    "bwd_stream32": (32, 1, tuple(N for dh, N in K.FWD_DH if dh == 32)),
    "bwd_stream128": (128, 1, tuple(N for dh, N in K.FWD_DH if dh == 128)),
}


def _mutant_jobs():
    """{(N, dh, qs, regime): [(pass, mutant, rounded_l, family)]}: every mutant at the smallest and the largest length of each
    family at which it applies; skip_rescale under `ramp`, and padded_key past N = 129 under `very_negative`, at the regime
    lengths"""
    jobs = {}
    for what, fams in (("fwd", FAMILIES_FWD), ("bwd", FAMILIES_BWD)):
        for fam, spec in fams.items():
            dh, qs, ns = spec[:3]
            rl = spec[3] if what == "fwd" else True
            for m in K.MUTANTS:
                ok = [N for N in ns if K.mutant_applies(m, what, N, None, rl)]
                for N in sorted({min(ok), max(ok)} if ok else ()):
                    jobs.setdefault((N, dh, qs, None), []).append((what, m, rl, fam))
    for r, N in K.REGIME_CASES:
        for m in ("skip_rescale", "padded_key"):
            if K.mutant_applies(m, "fwd", N, r):
                jobs.setdefault((N, 64, 1, r), []).append(("fwd", m, True, f"regime_{r}"))
    return jobs


JOBS = _mutant_jobs()


def test_every_mutant_has_a_job_in_every_family_it_applies_to():
    seen = {(fam, m) for js in JOBS.values() for _, m, _, fam in js}
    for fam in FAMILIES_FWD:
        for m in ("drop_key", "swap_heads", "truncate"):
            assert (fam, m) in seen, (fam, m)
    for fam in FAMILIES_BWD:
        for m in ("drop_key", "drop_query", "last_row_lse", "dq_stale_slice", "delta_stale_slice", "swap_heads", "truncate"):
            assert (fam, m) in seen, (fam, m)
    assert {("regime_ramp", "skip_rescale"), ("regime_very_negative", "padded_key")} <= seen
    # padded_key with random operands: the short head-resident lengths and every streaming family
    assert {("fwd_res8", "padded_key"), ("fwd_stream", "padded_key"), ("fwd_stream32", "padded_key"),
            ("fwd_stream128", "padded_key"), ("fwd_raw_res", "padded_key")} <= seen


@pytest.mark.parametrize("N,dh,qs,regime", sorted(JOBS, key=lambda c: (c[3] or "", c[1], c[2], c[0])))
def test_mutants_are_refused(N, dh, qs, regime):
    c = K.case(N, dh, qs, regime)
    for what, m, rl, fam in JOBS[(N, dh, qs, regime)]:
        tag = f"{fam}/{m}[{N},{dh},{qs},{regime}]"
        with pytest.raises(AssertionError) as e:
            if what == "fwd":
                c.check_forward(tag, c.forward("normalised", mutant=m), rl)
            else:
                c.check_backward(tag, c.backward("normalised", mutant=m))
        assert tag in str(e.value), str(e.value)  # (refused by check's own assertion, with the part and the group)
        print("ATTNMUT", tag, str(e.value)[len(tag) + 2:][:160])


def test_the_whole_tensor_norm_misses_what_the_groups_catch():
    """the gap this kit closes: one key of 512 dropped for one 16-row block of one head leaves the whole-tensor error of o
    inside every cap of tests/test_gpu_ops.py (1e-2 and up) and inside 3 x the error of a correct kernel, which is what its
    calibrated bound allows - and moves its group to several times the bound here"""
    c = K.case(512, 64, 1)
    clean, mut = c.forward("unnormalised"), c.forward("unnormalised", mutant="drop_key")
    rel = lambda t: float((t - c.ref["o"]).norm() / c.ref["o"].norm())
    assert rel(clean["o"]) < rel(mut["o"]) < min(3 * rel(clean["o"]), 1e-2)
    r = K.group_ratio(mut["o"], c.ref["o"], c.emu_fwd["o"], c.ref["mag"]["o"], 512, 64)
    assert float(r.max()) > 4.0 and float(K.group_ratio(clean["o"], c.ref["o"], c.emu_fwd["o"], c.ref["mag"]["o"], 512, 64).max()) < 0.7


# ---------------------------------------------------------------------------------------------- the plan query
def test_plan_query_names_the_kernel_of_every_case():
    """avf_attn_plan is pure host code: the lengths of the GPU file reach the kernels they were chosen for"""
    import avformer_amd as A
    plan = A.ops.attn_plan
    for kind, ns in K.FWD_QS.items():
        for N in ns:
            assert plan(N, 64, True)["fwd"] == kind, (kind, N)
    for dh, N in K.FWD_DH:
        assert plan(N, dh, True)["fwd"] == "stream" and plan(N, dh, True)["bwd"] == "stream", (dh, N)
    for dh, N, kind in K.FWD_RAW:
        assert plan(N, dh, False)["fwd"] == kind, (dh, N, kind)
    for kb, ns in K.BWD_MERGED.items():
        for N in ns:
            p = plan(N, 64, True)
            assert (p["bwd"], p["kb"], p["ragged"]) == ("merged", kb, N != 128 * kb), (kb, N, p)
    for N in K.MXO_LENGTHS:
        assert plan(N, 64, True)["bwd"] == "merged" and A._lib.load().avf_attn_bwd_emits_mx8(N, 64) == 1
    for dh, N, qs in K.BWD_STREAM:
        assert plan(N, dh, bool(qs))["bwd"] == "stream", (dh, N, qs)
    # under a mask: what avf_attn_masked_on_mfma says, the merged kernel's masked (ragged) instantiation
    for N, dh in ((1, 64), (128, 64), (512, 64), (513, 64), (40, 32), (130, 128)):
        p = plan(N, dh, True, masked=True)
        if A.ops.attn_masked_on_mfma(N, dh):
            assert p["fwd"].startswith("res") and (p["bwd"], p["ragged"]) == ("merged", True), (N, dh, p)
        else:
            assert (p["fwd"], p["bwd"]) == ("f32", "f32"), (N, dh, p)
    assert plan(64, 64, False, masked=True) == dict(fwd="f32", bwd="f32", kb=0, ragged=False)  # (a mask needs pre-scaled q there)
    with pytest.raises(RuntimeError, match="dim_head"):
        plan(16, 48, True)
