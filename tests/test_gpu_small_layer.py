"""-m gpu: the short-sequence fused layer kernels (csrc/layer_small.hip) at the operator level, group-wise against fp64.

(a) every case of tests/small_layer_util.py - all eight (dim, inner, mlp) triples, 1..16 tokens, 1 / 3 / 130 clips, one and two
    layers, dropout, both gradient streams - on the fused kernels (avf_layer_small_path == 7), y / dx / every gradient against
    oracle.transformer_forward + autograd in fp64, per token row, per 16-column block, per 16-row / 16-column block and q / k / v
    part of the weight gradients; the caps are the project's whole-tensor caps and 3 x the bf16-rounded CPU model for the groups
    (tests/test_small_layer_ref_cpu.py shows that the model keeps a third of each and that every named fault breaks one);
(b) the eligibility edges: the neighbours the dispatch refuses, two of them run on the per-operator path;
(c) path against path: the same cases in three child processes with one tuning switch each (AVF_LAYER_SMALL=0: everything
    per-operator; AVF_LAYER_SMALL_BWD=0: per-operator backward reading the block the fused forward saved - the only check that
    block gets; AVF_LAYER_SMALL_ATT=0: backward B without the fused attention backward);
(d) bitwise repeatability (the per-clip partial rows are folded in a fixed order)."""
import os
import subprocess
import sys

import pytest
import torch

import avformer_amd as A
import small_layer_util as U
from gpu_util import check, rel_fro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = {c: i for i, c in enumerate(U.CASES)}


@pytest.fixture(scope="module")
def parent():
    """every case once in this process, on the default dispatch: case -> gpu_run's dict"""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for case in U.CASES:
            U.set_grad_stream(case, mp.setenv, lambda k: mp.delenv(k, raising=False))
            out[case] = U.gpu_run(case, IDX[case])
    return out


def _check_groups(tag, got, ref, caps, zero_tol=1e-12):
    for name, err in U.grouped_errors_detail(got["y"], got["dx"], got["grads"], ref, zero_tol).items():
        kind = name.split("|")[0]
        check(f"{tag}:{name}", err, caps[kind])


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_fused_layer_vs_fp64_groupwise(parent, case):
    B, N, D, H, M, L, p, gs = case
    r = parent[case]
    assert r["path"] == 7, f"{U.case_id(case)} is expected on the three fused kernels, avf_layer_small_path = {r['path']}"
    sd, x = U.make_inputs(case)
    drop = None
    if p > 0.0:
        assert r["seed"] != 0
        drop = U.device_drop_factors(case, r["seed"])
    ref = U.reference_autograd(case, sd, x, drop)
    assert all(torch.isfinite(v).all() for v in (r["y"], r["dx"], *r["grads"].values()))
    _check_groups(f"small_layer[{U.case_id(case)}]", r, ref, U.CAPS)
    if p > 0.0:  # the masks really changed the result
        assert rel_fro(ref[0], U.reference_autograd(case, sd, x, None)[0]) > 0.1


# ------------------------------------------------------------------------------------------------------------------ (b)
def _module(D, H, dh, M, **kw):
    return A.Transformer(D, 1, H, dh, M, compute_dtype="bf16", **kw)


def test_eligibility_edges():
    path = A.ops.layer_small_path
    for D in (128, 256):
        for H in (4, 8):
            for M in (128, 256):
                assert path(_module(D, H, 32, M)._cfg(3, 16)) == 7
    t = _module(256, 8, 32, 256)
    assert path(t._cfg(3, 1)) == 7
    assert path(t._cfg(3, 17)) == 0
    assert path(_module(256, 4, 64, 256)._cfg(3, 16)) == 0
    assert path(_module(512, 8, 32, 256)._cfg(3, 16)) == 0
    assert path(_module(384, 8, 32, 256)._cfg(3, 16)) == 0
    assert path(_module(256, 8, 32, 256, residual_dtype="bf16")._cfg(3, 16)) == 0
    keep = torch.ones(3, 16, dtype=torch.uint8, device="cuda")
    assert path(t._cfg(3, 16, keep=keep)) == 0
    assert path(A.Transformer(256, 1, 8, 32, 256, compute_dtype="f32")._cfg(3, 16)) == 0


@pytest.mark.parametrize("case", [(3, 17, 256, 8, 256, 1, 0.0, "bf16"), (3, 16, 384, 8, 256, 1, 0.0, "bf16")], ids=U.case_id)
def test_refused_neighbours_on_the_per_operator_path(monkeypatch, case):
    """one token / one width step past the fused kernels: the per-operator path, same inputs, the whole-tensor caps"""
    monkeypatch.delenv("AVF_GRAD_STREAM", raising=False)
    r = U.gpu_run(case, 100)
    assert r["path"] == 0
    sd, x = U.make_inputs(case)
    e = U.grouped_errors(r["y"], r["dx"], r["grads"], U.reference_autograd(case, sd, x))
    for kind, cap in U.WHOLE_CAPS.items():
        check(f"small_layer_neighbour[{U.case_id(case)}]:{kind}", e[kind], cap)


# ------------------------------------------------------------------------------------------------------------------ (c)
SWITCHES = {"AVF_LAYER_SMALL": 0, "AVF_LAYER_SMALL_BWD": 1, "AVF_LAYER_SMALL_ATT": 3}  # switch set to 0 -> avf_layer_small_path

CHILD = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import small_layer_util as U
U.child_main(sys.argv[1], int(sys.argv[2]))
'''


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """one child per switch, one at a time, each under its own time limit: switch -> directory of its results"""
    out = {}
    for switch, expect in SWITCHES.items():
        d = tmp_path_factory.mktemp(switch.lower())
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "AVF_GRAD_STREAM"}
        env.update(AVF_TUNING="1", **{switch: "0"})
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), str(d), str(expect)],
                           capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and "SMALL_LAYER_CHILD_OK" in r.stdout, f"{switch}=0: exit {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-3000:]
        out[switch] = d
    return out


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_path_against_path(parent, children, switch):
    """the fused kernels (this process) against the same cases with one stage switched back to the per-operator kernels.  Bounds
    (small_layer_util.PATH_BOUNDS): y 4e-3 per group where the forward differs (a single-pass softmax apart: results two bf16
    roundings apart) and bit-identical where it does not; gradients 3 x the difference between the rounded model's two variants
    (dh2 / dh1 kept in fp32 by the fused kernels, rounded to bf16 by the per-operator ones): dx 1.43e-2 whole / 2.06e-2 row /
    1.67e-2 column block, weight gradients 1.36e-2 whole / 2.74e-2 block / 1.59e-2 q-k-v part, vectors 1.40e-2."""
    for case in U.CASES:
        p_, c_ = parent[case], torch.load(os.path.join(children[switch], f"{IDX[case]}.pt"))
        tag = f"small_layer_path[{switch}=0][{U.case_id(case)}]"
        assert c_["path"] == SWITCHES[switch] and p_["path"] == 7
        assert c_["seed"] == p_["seed"], (f"{tag}: the child drew dropout seed {c_['seed']}, this process {p_['seed']} - the two "
                                          f"runs saw different masks and the comparison is void")
        if switch != "AVF_LAYER_SMALL":  # the same forward kernel on the same inputs
            assert torch.equal(c_["y"], p_["y"]), tag
        _check_groups(tag, c_, (p_["y"], p_["dx"], p_["grads"]), U.PATH_BOUNDS, zero_tol=U.ZERO_REF_MAX)


# ------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("case", [(130, 12, 128, 8, 256, 1, 0.25, "f32"), (3, 7, 256, 4, 256, 2, 0.0, "bf16")], ids=U.case_id)
def test_repeatable_bit_for_bit(parent, monkeypatch, case):
    """a second run of a case (130 per-clip partial rows under dropout; two layers on the bf16 stream) gives the same bits"""
    U.set_grad_stream(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    a, b = parent[case], U.gpu_run(case, IDX[case])
    assert a["seed"] == b["seed"] and b["path"] == 7
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["dx"], b["dx"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
