"""CPU (no GPU needed): the argument that tests/test_gpu_small_layer.py means something.

The kit of tests/small_layer_util.py is held against itself: (1) its hand-written fp64 forward / backward is the oracle's autograd;
(2) the inputs make the attention core and both branches count; (3) the bf16-rounded model of layer_small.hip keeps a third of every
cap, whole-tensor and grouped, so a correct kernel has room; (4) every named fault, injected into the fp64 reference, breaks at least
one asserted quantity by 1.5 x its cap, so a wrong kernel has none; (5) on the default-init inputs of test_transformer_vs_oracle two
of those faults pass - the reason for the gains."""
import ctypes

import pytest
import torch

import avformer_amd as A
import small_layer_util as U

MARGIN = 1.5
LIB = A.ops._lib  # the binding ops itself calls through (a second import of the package under its alias leaves A._lib another module)


@pytest.fixture(scope="module")
def runs():
    """per case: inputs, masks, fp64 reference, input figures, the rounded model's grouped errors (computed once, never changed)"""
    out = {}
    for case in U.CASES:
        sd, x = U.make_inputs(case)
        drop = U.cpu_drop_factors(case)
        st = {}
        ref = U.model(case, sd, x, drop, stats=st)
        fused = U.model(case, sd, x, drop, rounded=True)
        perop = U.model(case, sd, x, drop, rounded=True, round_dh=True)
        out[case] = dict(sd=sd, x=x, drop=drop, ref=ref, stats=st, err=U.grouped_errors(*fused, ref),
                         variant=U.grouped_errors(*perop, fused))
    return out


def test_case_table_covers_what_the_kernels_are_built_for():
    triples = {(D, 32 * H, M) for B, N, D, H, M, L, p, gs in U.CASES}
    assert triples == {(d, i, m) for d in (128, 256) for i in (128, 256) for m in (128, 256)}
    assert {c[1] for c in U.CASES} == {1, 2, 7, 12, 13, 15, 16}
    for n in (2, 12, 15, 16):
        assert any(c[1] == n and c[2] > 32 * c[3] for c in U.CASES), f"N={n} on a triple with D > inner"
        assert any(c[1] == n and c[2] < 32 * c[3] for c in U.CASES), f"N={n} on a triple with D < inner"
    assert {c[0] for c in U.CASES} == {1, 3, 130}
    assert sum(c[5] == 2 for c in U.CASES) >= 3 and any(c[5] == 2 and c[6] > 0 for c in U.CASES)
    assert {c[6] for c in U.CASES} == {0.0, 0.25}
    assert {c[7] for c in U.CASES} == {"bf16", "f32"} and all(c[7] == "f32" for c in U.CASES if c[6] > 0)
    assert any(c[6] == 0 and c[7] == "f32" for c in U.CASES)
    assert len(set(U.CASES)) == len(U.CASES) and len({U.case_seed(c) for c in U.CASES}) == len(U.CASES)
    assert max(c[0] * c[1] for c in U.CASES) == 130 * 16


def test_every_case_is_eligible_for_the_fused_kernels():
    """avf_layer_small_path is pure host code: 7 for every case, whatever the gradient stream"""
    for B, N, D, H, M, L, p, gs in U.CASES:
        for stream in (0, 1):
            cfg = LIB.LayerCfg(B, N, D, H, 32, M, LIB.BF16, 1, 1e-5, 0.0, 0, 0, 0, None, stream, 0, 0, 0, 0, None)
            assert A.ops.layer_small_path(cfg) == 7, (B, N, D, H, M)


def test_small_path_query_edges():
    """the neighbours the dispatch refuses (pure host code; the GPU test runs them on the per-operator path)"""
    path = A.ops.layer_small_path
    mk = lambda N=16, D=256, H=8, dh=32, M=256, dt=LIB.BF16, rs=0, mask=None, mx=0: LIB.LayerCfg(
        3, N, D, H, dh, M, dt, 1, 1e-5, 0.0, 0, 0, 0, None, 1 if dt == LIB.BF16 else 0, mx, rs, 0, 0, mask)
    assert path(mk()) == 7
    assert path(mk(N=17)) == 0
    assert path(mk(H=4, dh=64)) == 0
    assert path(mk(D=512)) == 0 and path(mk(D=384)) == 0 and path(mk(M=512)) == 0 and path(mk(H=16)) == 0
    assert path(mk(rs=1)) == 0
    assert path(mk(dt=LIB.F32)) == 0
    assert path(mk(mx=1)) == 0
    keep = (ctypes.c_uint8 * 48)(*([1] * 48))
    assert path(mk(mask=ctypes.cast(keep, ctypes.c_void_p))) == 0
    assert path(mk(dh=48)) == 0  # an invalid configuration is no path at all


@pytest.mark.parametrize("case", [c for c in U.CASES if c[0] <= 3], ids=U.case_id)
def test_fp64_model_is_the_oracles_autograd(case):
    """with rounding off the hand-written forward / backward IS oracle.transformer_forward + autograd (so the faults are injected
    into the very reference the GPU test uses, and the rounded model differs from it by its roundings alone)"""
    sd, x = U.make_inputs(case)
    drop = U.cpu_drop_factors(case)
    e = U.grouped_errors(*U.model(case, sd, x, drop), U.reference_autograd(case, sd, x, drop))
    assert max(e.values()) < 1e-12, e


def test_inputs_make_every_phase_count(runs):
    for case, r in runs.items():
        for l, s in r["stats"].items():
            tag = f"{U.case_id(case)} layer {l}: {s}"
            if case[1] >= 7:
                assert U.PMAX_RANGE[0] <= s["pmax"] <= U.PMAX_RANGE[1], tag
            assert U.BRANCH_RANGE[0] <= s["attn"] <= U.BRANCH_RANGE[1], tag
            assert U.BRANCH_RANGE[0] <= s["mlp"] <= U.BRANCH_RANGE[1], tag


def test_rounded_model_keeps_a_third_of_every_cap(runs):
    """headroom: whole-tensor and grouped errors of the rounded model are at most cap / BOUND_FACTOR in every case"""
    for case, r in runs.items():
        for kind, v in r["err"].items():
            assert v <= U.CAPS[kind] / U.BOUND_FACTOR, f"{U.case_id(case)} {kind}: model {v:.3e}, cap {U.CAPS[kind]:.3e}"


def test_model_figures_are_the_recorded_ones(runs):
    """the tables of small_layer_util.py are what the model gives here: each recorded figure is the worst case's, rounded up"""
    for table, field in ((U.MODEL_WORST, "err"), (U.MODEL_VARIANT_DIFF, "variant")):
        for kind, rec in table.items():
            worst = max(r[field].get(kind, 0.0) for r in runs.values())
            assert 0.9 * rec <= worst <= rec, f"{field} {kind}: recorded {rec:.4e}, recomputed {worst:.4e}"
    for kind, whole in U.GROUP_OF.items():
        assert U.CAPS[kind] == min(U.BOUND_FACTOR * U.MODEL_WORST[kind], 2 * U.WHOLE_CAPS[whole])
        assert U.BOUND_FACTOR * U.MODEL_WORST[kind] <= 2 * U.WHOLE_CAPS[whole], kind  # no group cap had to be clipped
    for r in runs.values():  # the two variants share the forward bit for bit
        assert r["variant"]["y.whole"] == 0.0
        for kind in ("g.whole:zero", "g.block:zero", "g.qkv_part:zero"):
            assert r["err"].get(kind, 0.0) == 0.0


# fault -> the cases it applies to (a fault of a path is looked for on a case of that path)
FAULT_CASES = {
    "pad_keys": lambda c: 7 <= c[1] < 16,
    "scale_10pct": lambda c: c[1] >= 7,
    "copy_last_row": lambda c: c[1] >= 7,
    "head0_reads_head1_k": lambda c: c[1] >= 7,
    "bwd_lse_shift": lambda c: c[1] >= 7,
    "site1_next_row": lambda c: c[6] > 0,
    "handoff_mask_missing": lambda c: c[5] == 2 and c[6] > 0,
    "db1_last_clip": lambda c: c[0] == 3,
    "ln2_last_clip": lambda c: c[0] == 3,
    "ln1_last_clip": lambda c: c[0] == 3,
}


def _worst_ratio(errs, caps=None):
    caps = caps or U.CAPS
    return max((v / caps[k], k) for k, v in errs.items())


@pytest.mark.parametrize("fault", U.FAULTS)
def test_fault_breaks_a_cap(runs, fault):
    """each fault, injected into the fp64 reference, exceeds at least one asserted cap by MARGIN on a case it applies to"""
    assert set(FAULT_CASES) == set(U.FAULTS)
    cases = [c for c in U.CASES if FAULT_CASES[fault](c) and c[0] <= 3]
    assert cases
    best = (0.0, None, None)
    for case in cases:
        r = runs[case]
        got = U.model(case, r["sd"], r["x"], r["drop"], faults=(fault,))
        ratio, kind = _worst_ratio(U.grouped_errors(*got, r["ref"]))
        best = max(best, (ratio, kind, U.case_id(case)))
    print(f"{fault}: {best[0]:.2f} x cap of {best[1]} on {best[2]}")
    assert best[0] >= MARGIN, best
    if fault == "bwd_lse_shift":  # a backward-only fault leaves the forward alone
        assert torch.equal(got[0], r["ref"][0])


def test_default_init_hides_the_attention_core():
    """why the gains: with the inputs of test_transformer_vs_oracle (init_transformer_state weights, B=6, N=12, D=256, H=8, M=256,
    one layer) the softmax is nearly uniform (median largest probability 0.13) and the attention branch a tenth of its residual.
    A score scale off by 10 % then stays under EVERY whole-tensor cap (y 3.4e-3 / dx 5.1e-3 / worst matrix gradient 2.8e-2 / worst
    vector gradient 3.4e-2 against 1.5e-2 / 3e-2 / 4e-2 / 6e-2), and a last attention row copied from its neighbour stays under the
    caps of y and dx (1.39e-2 / 1.44e-2) - the forward and the input gradient are blind to it; only a whole-tensor weight gradient
    (0.11) sees it.  At the gains of small_layer_util.py the same two faults on the same shape exceed a cap by MARGIN or more."""
    case = (6, 12, 256, 8, 256, 1, 0.0, "bf16")
    sd, x = U.make_inputs(case, default_init=True)
    ref = U.model(case, sd, x)
    st = {}
    U.model(case, sd, x, stats=st)
    assert st[0]["pmax"] < 0.2 and st[0]["attn"] < 0.2
    whole = {}
    for fault in ("scale_10pct", "copy_last_row"):
        e = U.grouped_errors(*U.model(case, sd, x, faults=(fault,)), ref)
        whole[fault] = {k: v for k, v in e.items() if k.endswith(".whole")}
        print(fault, {k: f"{v:.2e}" for k, v in whole[fault].items()})
    assert all(v < U.WHOLE_CAPS[k] for k, v in whole["scale_10pct"].items()), whole
    assert all(whole["copy_last_row"][k] < U.WHOLE_CAPS[k] for k in ("y.whole", "dx.whole")), whole
    assert whole["copy_last_row"]["g.whole"] > U.WHOLE_CAPS["g.whole"]
    sd, x = U.make_inputs(case)
    ref = U.model(case, sd, x)
    for fault in ("scale_10pct", "copy_last_row"):
        ratio, kind = _worst_ratio(U.grouped_errors(*U.model(case, sd, x, faults=(fault,)), ref))
        assert ratio >= MARGIN, (fault, ratio, kind)
