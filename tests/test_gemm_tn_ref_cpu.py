"""No device: the fp64 reference and the element-wise bound of tests/gemm_tn_util.py pass an honest fp32 computation of the
weight-gradient GEMM (one float32 matmul per split-K slab, folded in fp32) on every data family, and refuse every mutant a subtly
wrong TN kernel or fold would produce (the list in that module).  And the launcher's own plan queries (avf_gemm_tn_group_plan,
avf_gemm_tn_plan: host code) confirm that the case table of tests/test_gpu_gemm_tn.py reaches the variants it names, keep the
planner's invariants over a sweep, and pin the plan of the project's own layer shapes."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_tn_util as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N = 136, 72  # a 128-row tile and a ragged second one; a ragged column tile
KS = (8, 72, 320, 448, 2568)
SS = (1, 2, 3, 5, 9, 32)


def _seed(K, family):
    return 5000 + 10 * K + G.FAMILIES.index(family)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_honest_chain_stays_inside_the_bound(family):
    """worst error / bound over K x S here: normal 0.08, wide 0.25, cancel 0.05 - the bound leaves a correct kernel most of
    itself; "int" is exact"""
    worst = 0.0
    for K in KS:
        a, b = G.make_operands(K, M, N, _seed(K, family), family)
        ref, mag = G.products(a, b)
        for S in SS:
            r = G.check(f"{family}/K={K}/S={S}", G.chain(a, b, S), ref, mag, K, S, family)
            worst = max(worst, r)
    print(f"chain {family}: worst error / bound {worst:.4f}")
    assert worst <= 0.5, worst  # not tuned to this very chain: half of the bound is spare
    if family == "int":
        assert worst == 0.0


def test_int_family_is_exact_by_construction():
    """|sum| <= 64 K stays below 2^24 for every K of the GPU file, so fp32 holds every partial sum"""
    assert 64 * 8192 < 2 ** 24
    a, b = G.make_operands(2568, M, N, 1, "int")
    assert float(a.float().abs().max()) == 8.0 and float(b.float().abs().max()) == 8.0
    assert torch.equal(a.float(), a.float().round())


# (K, S, output shape) each mutant is tried at: K = 320 in S = 4 slabs of 128 rows runs 2, 2, 1, 0 K-steps (a dead slab)
MUTANT_CASES = {
    "kstep_dropped": [(320, S, (M, N)) for S in (1, 2, 3, 5)] + [(72, 1, (M, N))],
    "slab_dropped": [(320, 2, (M, N)), (320, 5, (M, N)), (448, 3, (M, N))],
    "slab_twice": [(320, 2, (M, N)), (320, 5, (M, N)), (448, 3, (M, N))],
    "dead_slab_nan": [(320, 4, (M, N)), (320, 9, (M, N))],
    "cols_swapped": [(320, 1, (M, N)), (320, 3, (M, N))],
    "tile_transposed": [(320, 1, (136, 136)), (320, 3, (136, 136))],
    "float4_sentinel": [(320, 1, (M, N)), (72, 1, (M, N))],
    "row_k_included": [(320, 1, (M, N)), (320, 3, (M, N)), (72, 1, (M, N))],
    "bf16_accumulate": [(320, 1, (M, N)), (320, 3, (M, N))],
}


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("name", G.MUTANTS)
def test_every_mutant_fails(name, family):
    for K, S, (m, n) in MUTANT_CASES[name]:
        a, b = G.make_operands(K, m, n, _seed(K, family) + m, family)
        ref, mag = G.products(a, b)
        what = f"{name}/{family}/K={K}/S={S}"
        G.check(what, G.chain(a, b, S), ref, mag, K, S, family)  # the same case unmutated passes
        with pytest.raises(AssertionError, match="error / bound above 1"):
            G.check(what, G.chain(a, b, S, mutant=name), ref, mag, K, S, family)


def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(G.MUTANTS)


# ------------------------------------------------------------------------------------------------
# the launcher's own plan, asked in a child process per switch setting (AVF_TN_BIG / _XCD are read once per process)
_PLAN_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import avformer_amd as A
import gemm_tn_util as G
ops = A.ops
name = sys.argv[1]
out = dict(rows=[], sweep=[], single=[], layers={})
def ask(shapes, K, sp):
    if sp is None:
        os.environ.pop("AVF_TN_SPLITS", None)
    else:
        os.environ["AVF_TN_SPLITS"] = str(sp)
    return ops.gemm_tn_group_plan(shapes, K)
for group, K, sp, want in G.CHILDREN[name][1]:
    out["rows"].append([group, K, sp, ask(G.GROUPS[group], K, sp)])
sweep_groups = dict(G.GROUPS, ONE=[(8, 8)], D512=[(1536, 512), (1024, 512), (512, 1024), (512, 512)],
                    D768=[(2304, 768), (1536, 768), (768, 1536), (768, 768)], RAGGED=[(1000, 136), (264, 520), (8, 8)])
for gname, shapes in sweep_groups.items():
    for K in (64, 128, 192, 256, 320, 448, 512, 576, 1024, 2048, 2112, 4096, 10368, 16384, 50176):
        for sp in (None, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 33):
            out["sweep"].append([gname, sum(m * n for m, n in shapes), K, sp, ask(shapes, K, sp)])
os.environ.pop("AVF_TN_SPLITS", None)
if name == "default":
    for (m, n, k), want in G.SINGLE:
        out["single"].append([[m, n, k], ops.gemm_tn_plan(m, n, k)])
    out["layers"]["d512"] = ops.gemm_tn_group_plan(sweep_groups["D512"], 10368)
    out["layers"]["d768"] = ops.gemm_tn_group_plan(sweep_groups["D768"], 16384)
    out["layers"]["d768_2112"] = ops.gemm_tn_group_plan(sweep_groups["D768"], 2112)
print("PLANS " + json.dumps(out))
"""
_plans = {}


def _child_plans(name):
    if name not in _plans:
        env = dict(os.environ, AVF_TUNING="1", **G.CHILDREN[name][0])
        for k in ("AVF_TN_BIG", "AVF_TN_XCD", "AVF_TN_SPLITS"):
            if k not in G.CHILDREN[name][0]:
                env.pop(k, None)
        r = subprocess.run([sys.executable, "-c", _PLAN_CHILD, name], capture_output=True, text=True, env=env, cwd=REPO, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("PLANS ")][-1]
        _plans[name] = json.loads(line[6:])
    return _plans[name]


@pytest.mark.parametrize("name", sorted(G.CHILDREN))
def test_case_table_plans_to_the_variants_it_names(name):
    rows = _child_plans(name)["rows"]
    assert len(rows) == len(G.CHILDREN[name][1])
    for (group, K, sp, want), (_, _, _, plan) in zip(G.CHILDREN[name][1], rows):
        got = {k: plan[k] for k in want}
        assert got == want, (name, group, K, sp, plan)
        assert plan["kchunk"] == G.split_kchunk(K, plan["S"]), (name, group, K, sp, plan)


def test_heuristic_rows_are_unforced():
    """fold_group_kernel<2 .. 8> and the 256 x 128 tile with S = 8 are reached by the heuristic itself"""
    rows = [(g, K, sp, w) for g, K, sp, w in G.CHILDREN["default"][1] if sp is None]
    assert {w["fold"] for _, _, _, w in rows} >= {-1, 2, 3, 4, 5, 6, 7, 8}
    assert any(w["big"] == 1 and w["S"] == 8 and w["xcd_groups"] == 1 for _, _, _, w in rows)


@pytest.mark.parametrize("name", sorted(G.CHILDREN))
def test_plan_invariants_over_a_sweep(name):
    for gname, elems, K, sp, p in _child_plans(name)["sweep"]:
        what = (name, gname, K, sp, p)
        assert p["kchunk"] % 64 == 0 and p["kchunk"] > 0, what
        assert p["S"] * p["kchunk"] >= K, what
        assert p["blocks"] >= p["tiles"] * p["S"], what
        assert p["blocks"] < p["tiles"] * p["S"] + 8, what  # the XCD-aware orders round up to 8 equal runs: by less than 8
        # an unsplit launch stores straight to C and needs no workspace; a split one needs S slabs of every output
        assert p["workspace_bytes"] >= (p["S"] * elems * 4 if p["S"] > 1 else 0), what
        assert sp is None or p["S"] == sp, what
        assert p["fold"] == (-1 if p["S"] == 1 else (p["S"] if p["S"] <= 8 else 0)), what
        assert p["waves"] == (8 if p["big"] else 4), what
        if not p["big"]:
            assert p["xcd_groups"] == 0 and p["blocks"] == p["tiles"] * p["S"], what
        else:
            assert p["xcd_groups"] == G.xcd_order(p["S"], name != "big_tile_major"), what


def test_case_table_reaches_every_variant():
    """what test_gpu_gemm_tn.py::test_every_variant_was_reached asserts after the runs, from the plans alone"""
    reached = set()
    for name in G.CHILDREN:
        for group, K, sp, plan in _child_plans(name)["rows"]:
            reached |= G.reached_by_group(plan, K)
    for (m, n, k), plan in _child_plans("default")["single"]:
        reached |= G.reached_by_single(plan, k)
    assert G.WANT <= reached, sorted(G.WANT - reached)
    # the K-steps per workgroup of the 256 x 128 rows, as the table states them
    big = {(g, K, sp): G.slab_steps(K, p["S"], p["kchunk"]) for g, K, sp, p in _child_plans("big")["rows"]}
    assert big[("R4", 320, 4)] == [2, 2, 1, 0] and big[("R4", 320, 1)] == [5] and big[("R4", 448, 1)] == [7]
    assert big[("R4", 448, 2)] == [4, 3] and big[("R4", 448, 3)] == [3, 3, 1]
    p = [p for g, K, sp, p in _child_plans("big")["rows"] if g == "SQ1024"][0]
    assert p["tiles"] == 32 and p["blocks"] == 288 and p["xcd_groups"] == -1  # more workgroups than the 256 slots


def test_single_problem_plans():
    for ((m, n, k), want), (_, plan) in zip(G.SINGLE, _child_plans("default")["single"]):
        assert plan == want, ((m, n, k), plan)
    m, n, k = 136, 264, 2568
    assert G.slab_steps(k, 10, 320) == [5] * 8 + [1, 0]  # the 8-row tail is a K-step of its own; the tenth slab is dead


def test_plans_of_the_layer_shapes_are_pinned():
    """the weight gradients of one layer at the benchmark's token counts: d = 512 over 32 x 324 = 10368 rows (C2), d = 768 over
    16 x 1024 = 16384 rows (C4) - and d = 768 at the 2112 rows of test_gpu_ops.py::test_gemm_tn_group, which run unsplit"""
    L = _child_plans("default")["layers"]
    assert L["d512"] == dict(big=1, waves=8, tiles=64, S=4, kchunk=2624, xcd_groups=2, blocks=256, fold=4,
                             workspace_bytes=4 * 4 * 512 * 4096)
    assert L["d768"] == dict(big=1, waves=8, tiles=144, S=3, kchunk=5504, xcd_groups=-1, blocks=432, fold=3,
                             workspace_bytes=4 * 3 * 768 * 6144)
    assert L["d768_2112"] == dict(big=1, waves=8, tiles=144, S=1, kchunk=2112, xcd_groups=8, blocks=144, fold=-1, workspace_bytes=0)
