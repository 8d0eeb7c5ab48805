"""-m gpu: every variant of the bf16 weight-gradient (TN) GEMM that csrc/gemm_bf16.hip can launch, element by element against the
fp64 reference of tests/gemm_tn_util.py (the bound (2 K + S) 2^-24 |A|^T |B| and its reasons: that module's docstring;
tests/test_gemm_tn_ref_cpu.py shows without a device that it bites and that the case table plans as stated).

kernel                                            reached by                                             rows (gemm_tn_util)
gemm_bf16_tn_kernel + fold_slabs_kernel           ops.gemm(trans_a=True, trans_b=False), S = 1, 3, 10, 32   SINGLE
gemm_bf16_tn_group_kernel (128 x 128, 4 waves)    ops.gemm_tn_group, S = 1 .. 9, fold <2 .. 8> unforced     CHILDREN["default"]
gemm_bf16_tn_group_big_kernel<3> (256 x 128)      AVF_TN_BIG=1 (and the heuristic's own pick), S = 1 .. 9:  CHILDREN["big"],
    runs of 0, 1, 2, 3, 4, 5 and 7 K-steps through the three-slot ring, xcd_groups 8, 4, 2, 1, -1;          CHILDREN["default"]
    tile-major ids with AVF_TN_XCD=0                                                                         CHILDREN["big_tile_major"]
fold_group_kernel<2 .. 8> and <0> (9 slabs)       every split row above

Every case asserts the launcher's own plan first (avf_gemm_tn_group_plan / avf_gemm_tn_plan), cycles the data families
"normal", "wide", "cancel", "int", reads operands that sit between NaN guard rows (the single-problem path also row-strided
views with 8 NaN pad columns), writes outputs that sit between sentinel guards (S = 1 of the single-problem path: ldc = N + 8),
takes the group's split-K workspace at exactly the queried size from a NaN-prefilled parent between sentinel guards, and checks:
every output finite, every element within the bound, "int" results equal to the fp64 product bit for bit, every guard intact, a
second call returning the same bits.  Each case prints a line "TNSTAT {json}" with its worst error / bound ratio.  The switches
AVF_TN_BIG / AVF_TN_XCD are read once per process: one child process per setting, one after the other, each
under its own time limit, none started after one that failed; a child saves what the device returned and this process checks it.

Worst error / bound ratios measured on an MI355X over the whole file (88 TNSTAT lines), per kernel and data family:
  kernel                                  normal   wide     cancel   int
  gemm_bf16_tn_kernel (+ fold_slabs)      0.054    0.101    0.006    exact     (the two at 8 x 8 x 8; 0.025 and below from K = 64 on)
  gemm_bf16_tn_group_kernel               0.0033   0.0072   0.0018   exact
  gemm_bf16_tn_group_big_kernel<3>        0.0023   0.0046   0.0012   exact
No kernel fault, guard hit, NaN or differing second call was found.  The device uses far less of the bound than the fp32
chain of the CPU test (0.08 / 0.25 / 0.05): the MFMA's 32-term sums and the long fp32 accumulation err far below their worst
case; the bound is the worst case of the number formats and stays as derived.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_tn_util as G

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR = 4  # guard rows on either side of an operand or an output
REACHED = set()
_child_failed = []  # the name of the first child that exited non-zero or ran out of time: no further child is started


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


def _seed(tag, i, j):
    return 100000 * tag + 100 * i + j


# ------------------------------------------------------------------------------------------------
# the single-problem path, in this process
def _in_nan(t, pad):
    """the operand t [K, X] on the device between NaN guard rows, with `pad` NaN columns per row (0: dense)"""
    K, X = t.shape
    buf = torch.full((K + 2 * GR, X + pad), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[GR:GR + K, :X]
    view.copy_(t)
    return view


def _guarded_out(M, N, pad):
    buf = torch.full((M + 2 * GR, N + pad), G.SENTINEL, dtype=F32, device="cuda")
    return buf, buf[GR:GR + M, :N]


def _guards_intact(buf, M, N):
    return bool((buf[:GR] == G.SENTINEL).all()) and bool((buf[GR + M:] == G.SENTINEL).all()) and bool((buf[:, N:] == G.SENTINEL).all())


@pytest.mark.parametrize("i", range(len(G.SINGLE)), ids=["%dx%dx%d" % s for s, _ in G.SINGLE])
def test_single_problem(ops, i):
    (M, N, K), want = G.SINGLE[i]
    plan = ops.gemm_tn_plan(M, N, K)
    assert plan == want, ((M, N, K), plan)
    REACHED.update(G.reached_by_single(plan, K))
    S = plan["S"]
    for f, family in enumerate(G.FAMILIES):  # (the shapes are small: every family on every one)
        _single_case(ops, M, N, K, plan, family, _seed(9, i, f))


def _single_case(ops, M, N, K, plan, family, seed):
    S = plan["S"]
    a, b = G.make_operands(K, M, N, seed, family)
    ref, mag = G.products(a, b)
    bits = None
    for pad in (0, 8):  # dense operands, then row-strided ones
        what = f"single[{M},{N},{K}]/S={S}/{family}/pad={pad}"
        a_dev, b_dev = _in_nan(a, pad), _in_nan(b, pad)
        got = []
        for _ in range(2):
            cbuf, cview = _guarded_out(M, N, 8 if S == 1 else 0)
            c = ops.gemm(a_dev, b_dev, trans_a=True, trans_b=False, out_dtype=F32, out=cview)
            torch.cuda.synchronize()
            assert c.data_ptr() == cview.data_ptr()
            assert _guards_intact(cbuf, M, N), what + ": a write outside the output"
            got.append(cview.cpu())
        assert bool(torch.isfinite(got[0]).all()), what + ": not finite (a read outside an operand, or a slab never written?)"
        assert torch.equal(got[0], got[1]), what + ": a second call differs"
        r = G.check(what, got[0], ref, mag, K, S, family)
        assert bits is None or torch.equal(bits, got[0]), what + ": strided operands give other bits than dense ones"
        bits = got[0]
        print("TNSTAT " + json.dumps(dict(kernel="single", shape=[M, N, K], S=S, kchunk=plan["kchunk"], family=family, pad=pad,
                                          ratio=round(r, 4))))


def test_split_path_refuses_a_strided_c_before_it_launches(ops):
    """gemm_bf16_tn with S > 1 folds into a dense C only: a row-strided C is refused BEFORE the GEMM kernel is enqueued - C and
    its surroundings keep their bytes - and the message names the entry point"""
    import avformer_amd as A
    M, N, K = 48, 40, 1000
    assert ops.gemm_tn_plan(M, N, K)["S"] == 3
    a, b = G.make_operands(K, M, N, 77, "normal")
    cbuf, cview = _guarded_out(M, N, 8)
    with pytest.raises(RuntimeError, match="gemm_bf16_tn: split-K path needs a dense C"):
        ops.gemm(a.cuda(), b.cuda(), trans_a=True, trans_b=False, out_dtype=F32, out=cview)
    assert A._lib.load().avf_last_error().startswith(b"gemm_bf16_tn:")
    torch.cuda.synchronize()
    assert bool((cbuf == G.SENTINEL).all()), "a refused call wrote to C"


# ------------------------------------------------------------------------------------------------
# the grouped kernels: one child process per switch setting
_CHILD = r"""
import os, sys, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import avformer_amd as A
import gemm_tn_util as G
ops = A.ops
name, tag = sys.argv[1], int(sys.argv[2])
GR, WG = %d, 64
NAN, SENT = float("nan"), G.SENTINEL
results = []
for i, (group, K, sp, want) in enumerate(G.CHILDREN[name][1]):
    if sp is None:
        os.environ.pop("AVF_TN_SPLITS", None)
    else:
        os.environ["AVF_TN_SPLITS"] = str(sp)
    shapes = G.GROUPS[group]
    plan = ops.gemm_tn_group_plan(shapes, K)
    assert {k: plan[k] for k in want} == want, (name, group, K, sp, plan)   # the plan first: nothing runs misplanned
    family = G.FAMILIES[i %% 4]
    pairs = []
    for j, (m, n) in enumerate(shapes):
        a, b = G.make_operands(K, m, n, 100000 * tag + 100 * i + j, family)
        dev = []
        for t in (a, b):   # dense, between NaN guard rows
            buf = torch.full((K + 2 * GR, t.shape[1]), NAN, dtype=torch.bfloat16, device="cuda")
            buf[GR:GR + K].copy_(t)
            dev.append(buf[GR:GR + K])
        pairs.append(tuple(dev))
    cbufs = [torch.empty((m + 2 * GR, n), dtype=torch.float32, device="cuda") for m, n in shapes]
    outs = [buf[GR:GR + m] for buf, (m, n) in zip(cbufs, shapes)]
    nws = plan["workspace_bytes"] // 4   # exactly what avf_gemm_tn_group_workspace_bytes promises
    assert plan["workspace_bytes"] %% 4 == 0 and (plan["S"] == 1 or nws >= plan["S"] * sum(m * n for m, n in shapes))
    wparent = torch.empty(WG + nws + WG, dtype=torch.float32, device="cuda")
    ws = wparent[WG:WG + nws]
    rec = dict(group=group, K=K, splits=sp, family=family, plan=plan, guards=True, ws_guards=True)
    got = []
    for call in range(2):
        for buf in cbufs:
            buf.fill_(SENT)
        wparent.fill_(SENT)
        ws.fill_(NAN)   # a slab folded without having been written shows as NaN in C
        ret = ops.gemm_tn_group(pairs, outs=outs, workspace=ws)
        torch.cuda.synchronize()
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(ret, outs))
        for buf, (m, n) in zip(cbufs, shapes):
            rec["guards"] &= bool((buf[:GR] == SENT).all()) and bool((buf[GR + m:] == SENT).all())
        rec["ws_guards"] &= bool((wparent[:WG] == SENT).all()) and bool((wparent[WG + nws:] == SENT).all())
        got.append([o.cpu() for o in outs])
    rec["outs"] = got[0]
    rec["same_bits"] = all(torch.equal(x, y) for x, y in zip(got[0], got[1]))
    results.append(rec)
os.environ.pop("AVF_TN_SPLITS", None)
torch.save(results, os.environ["AVF_TEST_OUT"])
""" % GR


@pytest.mark.parametrize("name", list(G.CHILDREN))
def test_group_child(name, tmp_path):
    if _child_failed:
        pytest.fail(f"not started: the child {_child_failed[0]!r} before it exited non-zero or ran out of time")
    env_extra, rows = G.CHILDREN[name]
    tag = list(G.CHILDREN).index(name)
    path = str(tmp_path / f"{name}.pt")
    env = dict(os.environ, AVF_TUNING="1", AVF_TEST_OUT=path, **env_extra)
    for k in ("AVF_TN_BIG", "AVF_TN_XCD", "AVF_TN_SPLITS"):
        if k not in env_extra:
            env.pop(k, None)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD, name, str(tag)], capture_output=True, text=True, env=env, cwd=REPO, timeout=240)
    except subprocess.TimeoutExpired:
        _child_failed.append(name)
        raise
    if r.returncode != 0:
        _child_failed.append(name)
    assert r.returncode == 0, f"child {name}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    results = torch.load(path)
    assert len(results) == len(rows)
    problems = []
    for i, ((group, K, sp, want), rec) in enumerate(zip(rows, results)):
        plan, family, shapes = rec["plan"], rec["family"], G.GROUPS[group]
        assert (rec["group"], rec["K"], rec["splits"]) == (group, K, sp) and {k: plan[k] for k in want} == want
        REACHED.update(G.reached_by_group(plan, K))
        what = f"{name}/{group}/K={K}/S={plan['S']}/{family}"
        worst = 0.0
        try:
            assert rec["guards"], what + ": a write outside an output"
            assert rec["ws_guards"], what + ": a write outside the workspace avf_gemm_tn_group_workspace_bytes promised"
            for j, ((m, n), c) in enumerate(zip(shapes, rec["outs"])):
                a, b = G.make_operands(K, m, n, _seed(tag, i, j), family)
                ref, mag = G.products(a, b)
                assert bool(torch.isfinite(c).all()), f"{what}[{j}]: not finite (a read of a guard row, or a slab folded unwritten?)"
                worst = max(worst, G.check(f"{what}[{j}]", c, ref, mag, K, plan["S"], family))
            assert rec["same_bits"], what + ": a second call differs"
        except AssertionError as e:  # every row is checked and reported before the test fails
            problems.append(str(e))
            worst = float("inf")
        print("TNSTAT " + json.dumps(dict(kernel=G.kernel_of(plan), child=name, group=group, K=K, S=plan["S"], kchunk=plan["kchunk"],
                                          xcd_groups=plan["xcd_groups"], fold=plan["fold"], blocks=plan["blocks"],
                                          steps=G.slab_steps(K, plan["S"], plan["kchunk"]), family=family, ratio=round(worst, 4))))
    assert not problems, "\n".join(problems)


def test_every_variant_was_reached():
    """coverage by assertion, from the plans the cases above saw: both group tiles, every fold
    code, every block order of the 256 x 128 tile, a dead slab on every kernel, runs of 0, 1, 2, 3, 4, 5 and >= 7 K-steps through
    the three-slot ring, S = 1, 3, 10 and 32 on the single-problem path (runs last; needs the tests above to have run)"""
    assert G.WANT <= REACHED, sorted(G.WANT - REACHED)
