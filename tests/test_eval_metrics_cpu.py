"""CPU: the evaluation metrics (metrics.AccF1Metric / CCCMetric / EvalMetrics, the plain-torch path of the kernel in
csrc/eval_metrics.hip) against fixture G18 - the reference's own metric classes fed as train.py:150-155 feeds them -, against
sklearn called directly, and the properties the data-parallel use relies on: the statistics are additive.  Bounds:
eval_metrics_util's docstring."""
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import avformer_amd as A
from conftest import load_golden
from eval_metrics_util import (CASES, COUNT_TOL, MUTANTS, ORDER_TOL, assert_scores_match_fixture, check_scores, fixture_batches,
                               flat_scores, moment_magnitudes, random_batch, same)

G = load_golden("g18_eval_metrics")
M = A.metrics


def _accumulate(batches, loss=None):
    m = A.EvalMetrics()
    for out, labels in batches:
        m.update(out, labels, loss)
    return m


@pytest.mark.parametrize("case", CASES)
def test_g18_scores_match_the_reference(case):
    batches = fixture_batches(G, case)
    got = flat_scores(_accumulate(batches).scores())
    print(case, got)
    assert_scores_match_fixture(got, G, case)
    # the checker itself meets the fixture with the same bounds
    assert_scores_match_fixture(check_scores(batches), G, case)


@pytest.mark.parametrize("rows", [1, 2, 7, 64, 257, 4096])
def test_against_sklearn_directly(rows):
    from sklearn.metrics import accuracy_score, f1_score
    out, labels = random_batch(rows, 500 + rows)
    m = _accumulate([(out, labels)])
    got = flat_scores(m.scores())
    pred = torch.argmax(out[:, 12:19], 1).numpy()
    keep = labels["EX"].numpy() != 7
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if keep.any():
            assert same(got["ex_acc"], accuracy_score(labels["EX"].numpy()[keep], pred[keep]), COUNT_TOL)
            assert same(got["ex_f1"], f1_score(labels["EX"].numpy()[keep], pred[keep], average="macro"), COUNT_TOL)
        else:
            assert np.isnan(got["ex_acc"]) and np.isnan(got["ex_f1"])
        pa = np.round(torch.sigmoid(out[:, :12]).numpy())
        ya = labels["AU"].numpy()
        f1, correct = [], 0
        for u in range(12):
            k = ya[:, u] != -1
            f1.append(f1_score(ya[k, u], pa[k, u], average="binary") if k.any() else 0.0)
            correct += accuracy_score(ya[k, u], pa[k, u], normalize=False) if k.any() else 0
    assert same(got["au_f1"], np.mean(f1), COUNT_TOL)
    if (ya != -1).any():
        assert same(got["au_acc"], correct / (ya != -1).sum(), COUNT_TOL)
    ref = check_scores([(out, labels)])
    for k in ("ccc_v", "ccc_a", "va_score"):
        assert same(got[k], ref[k], 1e-10), (k, got[k], ref[k])


def test_merge_is_additive():
    out, labels = random_batch(1000, 77)
    whole = _accumulate([(out, labels)], loss=torch.tensor(0.5))
    parts = [_accumulate([(out[a:b], {k: v[a:b] for k, v in labels.items()})], loss=torch.tensor(0.5))
             for a, b in ((0, 1), (1, 300), (300, 1000))]
    merged = A.EvalMetrics()
    for p in parts:
        merged.merge(p)
    assert torch.equal(merged.state[:M.VA_MOMENTS], whole.state[:M.VA_MOMENTS])
    mom = merged.state[M.VA_MOMENTS:M.LOSS_SUM].reshape(2, 6)
    ref = whole.state[M.VA_MOMENTS:M.LOSS_SUM].reshape(2, 6)
    assert torch.equal(mom[:, 0], ref[:, 0])
    assert bool(((mom - ref).abs() <= ORDER_TOL * moment_magnitudes([(out, labels)])).all())
    assert float(merged.state[M.LOSS_SUM]) == 1.5 and float(merged.state[M.LOSS_STEPS]) == 3.0
    assert float(whole.state[M.LOSS_STEPS]) == 1.0 and float(merged.state[123:].abs().sum()) == 0.0
    for k, v in flat_scores(whole.scores()).items():
        assert same(flat_scores(merged.scores())[k], v, 1e-12), k
    assert abs(merged.avg_loss - 0.5) < 1e-15


def test_missing_labels_leave_their_slots_alone():
    out, labels = random_batch(50, 3)
    full = _accumulate([(out, labels)])
    for key, sl in (("EX", slice(M.EX_CONF, M.AU_STATS)), ("AU", slice(M.AU_STATS, M.VA_MOMENTS)), ("VA", slice(M.VA_MOMENTS, M.LOSS_SUM))):
        m = A.EvalMetrics()
        m.update(out, {k: v for k, v in labels.items() if k != key})
        assert float(m.state[sl].abs().sum()) == 0.0
        rest = torch.ones(128, dtype=torch.bool)
        rest[sl] = False
        assert torch.equal(m.state[rest], full.state[rest])


@pytest.mark.parametrize("case", ["eq", "mix", "exabs", "auedge"])
def test_single_metric_classes_agree_with_eval_metrics(case):
    batches = fixture_batches(G, case)
    ex, va, au, au_logits = A.AccF1Metric(ignore_index=7), A.CCCMetric(ignore_index=-5.0), A.MultiLabelAccF1(ignore_index=-1), A.MultiLabelAccF1()
    em = A.EvalMetrics()
    for i, (out, labels) in enumerate(batches):
        p = em.predict(out)
        assert torch.equal(p["EX"], torch.argmax(out[:, 12:19], 1)) and torch.equal(p["VA"], torch.tanh(out[:, 19:21]))
        assert torch.equal(p["AU"].float(), torch.round(torch.sigmoid(out[:, :12])))
        # numpy and tensors alike
        ex.update(p["EX"].numpy() if i % 2 else p["EX"], labels["EX"].numpy() if i % 2 else labels["EX"])
        va.update(y_pred=p["VA"].numpy() if i % 2 else p["VA"], y_true=labels["VA"])
        au.update(p["AU"].float(), labels["AU"])
        au_logits.update_from_logits(out, labels["AU"])
        em.update(out, labels)
    s = flat_scores(em.scores())
    assert same(ex.get()[0], s["ex_acc"], 1e-15) and same(ex.get()[1], s["ex_f1"], 1e-15)
    assert same(au.get()[0], s["au_acc"], 1e-15) and same(au.get()[1], s["au_f1"], 1e-15) and au_logits.get() == au.get()
    assert [same(a, b, 1e-15) for a, b in zip(va.get(), (s["ccc_v"], s["ccc_a"], s["va_score"]))] == [True] * 3
    assert same(em.total_score("ALL"), s["ex_score"] + s["au_score"] + s["va_score"], 1e-15) or np.isnan(s["ex_score"])
    assert same(em.total_score("VA"), s["va_score"], 0.0)
    ex.clear(), va.clear(), au.clear(), em.clear()
    assert float(em.state.abs().sum()) == 0.0
    with pytest.raises(RuntimeError):
        ex.get()


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checker_rejects_wrong_forms(mutant):
    """the fp64 checker is sharp enough to tell the reference's formulas from their nearest wrong forms: with the fixture's own
    bounds, each mutant fails on at least one G18 case (and the unmutated checker on none: test_g18_scores_match_the_reference)"""
    failed = []
    for case in CASES:
        try:
            assert_scores_match_fixture(check_scores(fixture_batches(G, case), mutant=mutant), G, case)
        except AssertionError:
            failed.append(case)
    print(mutant, "rejected on", failed)
    assert failed


def test_fixture_regenerates_and_keeps_out_of_the_band():
    for case in CASES:
        au = G[f"{case}.out"][..., :12]
        assert not bool(((au > 0) & (au < 2.0 ** -22)).any())
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "g18_eval_metrics.npz")) < 100 * 1024


def test_evaluate_runs_the_reference_loop_on_a_stand_in_model():
    class Stand(torch.nn.Module):
        task = "ALL"

        def forward(self, x):
            return x["rows"]

        def get_mt_loss(self, result, labels):
            assert not self.training and not torch.is_grad_enabled()
            return [result[:, 0].mean(), result[:, 1].mean(), result[:, 2].mean()]

        def get_va_loss(self, result, y):
            return result[:, 19].mean()

    batches = fixture_batches(G, "mix")
    model = Stand()
    metrics = A.EvalMetrics()
    scores = A.evaluate(model, [({"rows": o}, l) for o, l in batches], num_step=2, metrics=metrics)
    assert model.training
    ref = check_scores(batches[:2])
    for k, v in flat_scores(scores).items():
        if k in ref:
            assert same(v, ref[k], 1e-10), k
    want = np.mean([float(o[:, 0].mean() + o[:, 1].mean() + o[:, 2].mean()) for o, _ in batches[:2]])
    assert abs(metrics.avg_loss - want) < 1e-6 and float(metrics.state[M.LOSS_STEPS]) == 2.0
    A.evaluate(model, [({"rows": o}, l) for o, l in batches], num_step=10, task="VA", metrics=metrics)
    assert float(metrics.state[M.LOSS_STEPS]) == len(batches)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out, labels = random_batch(600, 91)
        a, b = (0, 250) if rank == 0 else (250, 600)          # unequal shares
        m = A.EvalMetrics()
        for s in range(a, b, 50):
            m.update(out[s:s + 50], {k: v[s:s + 50] for k, v in labels.items()}, torch.tensor(float(s)))
        m.all_reduce()
        q.put((rank, m.state.clone().numpy(), flat_scores(m.scores()), m.avg_loss))
    finally:
        dist.destroy_process_group()


def test_two_rank_all_reduce_gives_the_global_scores():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    out, labels = random_batch(600, 91)
    single = A.EvalMetrics()
    for s in range(0, 600, 50):
        single.update(out[s:s + 50], {k: v[s:s + 50] for k, v in labels.items()}, torch.tensor(float(s)))
    want = flat_scores(single.scores())
    for rank, state, got, avg in res:
        assert np.array_equal(state[:M.VA_MOMENTS], single.state[:M.VA_MOMENTS].numpy())
        for k, v in want.items():
            assert same(got[k], v, 1e-12), (rank, k)
        assert abs(avg - single.avg_loss) < 1e-12
    ref = check_scores([(out, labels)])
    for k in ref:
        assert same(want[k], ref[k], 1e-10), k
