"""-m gpu: the evaluation-metric kernels (csrc/eval_metrics.hip: one launch per validation batch into a 128-word fp64 state, one
launch from the state to the scores) and everything built on them.

Parity: fixture G18 - the reference's own metric classes - through the kernels.  The count slots of the state are bit-equal to
the plain-torch statistics taken on the CPU; the moment slots differ from them only through the device's tanhf, measured here in
fp32 ulps against CPU torch on the fixture's VA logits (TANH_ULPS) and propagated slot by slot (eval_metrics_util.moment_bounds);
the scores meet the fixture with the CPU bounds plus that term.  Sizes 1 .. 16 384 rows, three row strides, strided label
views, each task without labels, predictions only, guard words, bit-identical repeats, no host synchronisation, one launch per
update, a captured graph of forward + losses + update, and evaluate() on a small sformer against the host recipe."""
import gc
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from eval_metrics_util import (CASES, ORDER_TOL, assert_scores_match_fixture, ccc_tanh_term, check_scores, fixture_batches,
                               flat_scores, moment_bounds, random_batch, same, ulps_between)

pytestmark = pytest.mark.gpu

G = load_golden("g18_eval_metrics")
# max |tanhf on the device - torch.tanh on the CPU| over the VA logits of G18, in fp32 ulps of the CPU value (measured on an
# MI355X: 1.000; test_device_tanh_within_the_measured_ulps prints and pins it)
TANH_ULPS = 1.0
CNT = slice(0, 109)


def _cuda(labels):
    return {k: v.cuda() for k, v in labels.items()}


def _both(batches, loss=None):
    import avformer_amd as A
    dev, cpu = A.EvalMetrics(device="cuda"), A.EvalMetrics()
    for out, labels in batches:
        dev.update(out.cuda(), _cuda(labels), None if loss is None else loss.cuda())
        cpu.update_torch(out, labels, loss)
    return dev, cpu


def _assert_state(dev_state, cpu_state, batches, what):
    d, c = dev_state.cpu(), cpu_state.cpu()
    assert torch.equal(d[CNT], c[CNT]), f"{what}: count slots differ"
    dm, cm = d[109:121].reshape(2, 6), c[109:121].reshape(2, 6)
    assert torch.equal(dm[:, 0], cm[:, 0]), f"{what}: VA n differs"
    bound = moment_bounds(batches, TANH_ULPS)
    err = (dm - cm).abs()
    print(f"{what}: moment |err| max {float(err.max()):.3g}, worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3g}")
    assert bool((err <= bound).all()), (what, err, bound)
    assert torch.equal(d[121:], c[121:])


def test_device_tanh_within_the_measured_ulps():
    import avformer_amd as A
    x = torch.cat([G[f"{case}.out"].reshape(-1, 21) for case in CASES])
    got = A.EvalMetrics().predict(x.cuda())["VA"].cpu()
    u = ulps_between(got, torch.tanh(x[:, 19:21]))
    print(f"device tanhf against CPU torch.tanh on {x.shape[0] * 2} fixture logits: {u:.3f} ulps")
    assert u <= TANH_ULPS


@pytest.mark.parametrize("case", CASES)
def test_g18_through_the_kernel(case):
    import avformer_amd as A
    batches = fixture_batches(G, case)
    dev, cpu = _both(batches)
    _assert_state(dev.state, cpu.state, batches, case)
    vec = dev.scores_vector()
    host = A.metrics.scores_from_state(dev.state)
    for i, name in enumerate(A.metrics.SCORE_NAMES):
        assert same(vec[i], host[i], 1e-12), (case, name, float(vec[i]), float(host[i]))
    extra = ccc_tanh_term(cpu.state, moment_bounds(batches, TANH_ULPS))
    got = flat_scores(dev.scores())
    print(case, got, "ccc tanh term", extra)
    assert_scores_match_fixture(got, G, case, extra_ccc=extra)


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 16384])
def test_sizes_strides_and_predictions(rows):
    import avformer_amd as A
    for ld in (21, 24, 32):
        out, labels = random_batch(rows, 1000 + rows + ld, width=ld)
        wide = out.cuda()[:, :21]
        assert wide.stride() == (ld, 1)
        # labels as views into wider arrays
        au_w, va_w = torch.zeros(rows, 16), torch.zeros(rows, 4)
        au_w[:, 2:14], va_w[:, 1:3] = labels["AU"], labels["VA"]
        lab = {"EX": labels["EX"].cuda(), "AU": au_w.cuda()[:, 2:14], "VA": va_w.cuda()[:, 1:3]}
        assert lab["AU"].stride() == (16, 1) and lab["VA"].stride() == (4, 1)
        dev, cpu = A.EvalMetrics(device="cuda"), A.EvalMetrics()
        dev.update(wide, lab)
        cpu.update_torch(out[:, :21], labels)
        _assert_state(dev.state, cpu.state, [(out[:, :21], labels)], f"rows {rows} ld {ld}")
        ref = check_scores([(out[:, :21], labels)])
        got = flat_scores(dev.scores())
        extra = ccc_tanh_term(cpu.state, moment_bounds([(out[:, :21], labels)], TANH_ULPS))
        for k, v in ref.items():
            assert same(got[k], v, (1e-10 + extra) if "ccc" in k or k == "va_score" else 1e-12), (rows, ld, k, got[k], v)
        p = dev.predict(wide)
        assert torch.equal(p["EX"].cpu(), torch.argmax(out[:, 12:19], 1))
        assert torch.equal(p["AU"].cpu().float(), torch.round(torch.sigmoid(out[:, :12])))
        u = ulps_between(p["VA"], torch.tanh(out[:, 19:21]))
        print(f"rows {rows} ld {ld}: device tanhf against CPU torch.tanh {u:.3f} ulps")
        assert u <= TANH_ULPS


def test_null_labels_predict_only_and_guard_words():
    import avformer_amd as A
    rows = 300
    out, labels = random_batch(rows, 5)
    o, lab = out.cuda(), _cuda(labels)
    em = A.EvalMetrics()
    cfg = em._cfg()
    full = torch.zeros(128, dtype=torch.float64, device="cuda")
    A.ops.eval_update(o, lab["EX"], lab["AU"], lab["VA"], None, cfg, full)
    SENT = -777.0

    def guarded(n, dtype, fill):
        buf = torch.full((n + 32,), fill, dtype=dtype, device="cuda")
        return buf, buf[16:16 + n]

    # every buffer between guard words; the state starts from a recognisable value, so an untouched slot shows
    for skip, sl in ((None, None), ("EX", slice(0, 49)), ("AU", slice(49, 109)), ("VA", slice(109, 121))):
        sbuf, st = guarded(128, torch.float64, SENT)
        st.fill_(3.0)
        abuf, pa = guarded(rows * 12, torch.uint8, 99)
        ebuf, pe = guarded(rows, torch.int64, -9)
        vbuf, pv = guarded(rows * 2, torch.float32, SENT)
        ys = [None if skip == k else lab[k] for k in ("EX", "AU", "VA")]
        A.ops.eval_update(o, ys[0], ys[1], ys[2], None, cfg, st, pa.view(rows, 12), pe, pv.view(rows, 2))
        want = full + 3.0
        if sl is not None:
            want[sl] = 3.0
        err = (st - want).abs().cpu()
        assert float(err[CNT].max()) == 0.0 and float(err[121:].max()) == 0.0 and float(err.max()) < 1e-9, (skip, err)
        assert float(st[121]) == 3.0 and float(st[122]) == 3.0            # no loss given: the loss words are left alone
        for buf, fill in ((sbuf, SENT), (abuf, 99), (ebuf, -9), (vbuf, SENT)):
            assert bool((buf[:16] == fill).all()) and bool((buf[-16:] == fill).all()), skip
        assert torch.equal(pe.cpu(), torch.argmax(out[:, 12:19], 1))
        assert torch.equal(pa.view(rows, 12).cpu().float(), torch.round(torch.sigmoid(out[:, :12])))
        assert ulps_between(pv.view(rows, 2), torch.tanh(out[:, 19:21])) <= TANH_ULPS
    # state null: predictions only, each buffer on its own
    p = em.predict(o)
    abuf, pa = guarded(rows * 12, torch.uint8, 99)
    A.ops.eval_update(o, lab["EX"], lab["AU"], lab["VA"], None, cfg, None, pa.view(rows, 12))
    assert torch.equal(pa.view(rows, 12), p["AU"]) and bool((abuf[:16] == 99).all()) and bool((abuf[-16:] == 99).all())
    with pytest.raises(RuntimeError, match="neither a state nor a prediction"):
        A.ops.eval_update(o, lab["EX"], None, None, None, cfg, None)
    # the loss words
    st = torch.zeros(128, dtype=torch.float64, device="cuda")
    for v in (0.25, 1.5):
        A.ops.eval_update(o, None, None, None, torch.tensor(v, device="cuda"), cfg, st)
    assert float(st[121]) == 1.75 and float(st[122]) == 2.0 and float(st[:121].abs().sum()) == 0.0
    assert float(A.ops.eval_scores(st, cfg)[9]) == 0.875


def _sequence():
    return [random_batch(r, 40 + i) for i, r in enumerate((64, 257, 1000, 64, 4096, 1, 300, 2048))]


def test_same_sequence_gives_the_same_bits_and_never_synchronises():
    import avformer_amd as A
    seq = [(o.cuda(), _cuda(l)) for o, l in _sequence()]
    loss = torch.tensor(0.5, device="cuda")
    states = []
    for _ in range(2):
        m = A.EvalMetrics(device="cuda")
        for o, l in seq:
            m.update(o, l, loss)
        states.append(m.state.clone())
    assert torch.equal(states[0], states[1])
    m = A.EvalMetrics(device="cuda")
    m.update(*seq[0], loss)                                   # the first call builds the cfg struct
    m.clear()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for o, l in seq:
            m.update(o, l, loss)
        kept = m.state.clone()
        m.clear()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(kept, states[0]) and float(m.state.abs().sum()) == 0.0


def test_launch_counts():
    """one launch per update, one per scores: counted with the profiler as test_gpu_task_losses.py counts them"""
    import avformer_amd as A
    from torch.profiler import ProfilerActivity, profile
    out, labels = random_batch(256, 9)
    o, lab, loss = out.cuda(), _cuda(labels), torch.tensor(0.5, device="cuda")
    m = A.EvalMetrics(device="cuda")
    m.update(o, lab, loss)
    m.scores()
    torch.cuda.synchronize()

    def kernels(fn):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                and "Memset" not in e.name]
    ku = kernels(lambda: m.update(o, lab, loss))
    ks = kernels(lambda: m.scores())
    print(ku, ks)
    assert len(ku) == 1 and "eval_update_kernel" in ku[0], ku
    assert len(ks) == 1 and "eval_scores_kernel" in ks[0], ks


def _sformer_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 256, 7, 7, generator=g)
    y_ex = torch.randint(0, 8, (B,), generator=g)
    y_ex[0] = 2
    y_au = (torch.rand(B, 12, generator=g) > 0.5).float()
    y_au[1, 3] = -1
    y_va = torch.rand(B, 2, generator=g) * 2 - 1
    y_va[2] = -5.0
    return x, {"EX": y_ex, "AU": y_au, "VA": y_va}


def test_evaluate_on_sformer_matches_the_host_recipe():
    import avformer_amd as A
    from sklearn.metrics import accuracy_score, f1_score
    torch.manual_seed(0)
    m = A.build_model("sformer", task="ALL", task_losses="reference").cuda().train()
    data = [_sformer_inputs(16, 60 + i) for i in range(3)]
    batches = [({"clip": x.cuda()}, _cuda(l)) for x, l in data]
    metrics = A.EvalMetrics(device="cuda")
    scores = A.evaluate(m, batches, num_step=3, metrics=metrics)
    assert m.training
    # the reference's recipe on the host from the same outputs
    m.eval()
    with torch.no_grad():
        outs = [m(x).float().cpu() for x, _ in batches]
        losses = [float(sum(m.get_mt_loss(m(x), l))) for x, l in batches]
    m.train()
    host = [(o, l) for o, (_, l) in zip(outs, data)]
    ref = check_scores(host)
    cpu = A.EvalMetrics()
    for o, l in host:
        cpu.update_torch(o, l)
    extra = ccc_tanh_term(cpu.state, moment_bounds(host, TANH_ULPS))
    got = flat_scores(scores)
    print(got, ref, "avg_loss", metrics.avg_loss, np.mean(losses))
    for k, v in ref.items():
        assert same(got[k], v, (1e-10 + extra) if "ccc" in k or k == "va_score" else 1e-12), (k, got[k], v)
    pred = torch.cat([torch.argmax(o[:, 12:19], 1) for o in outs]).numpy()
    y = torch.cat([l["EX"] for _, l in data]).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert same(got["ex_acc"], accuracy_score(y[y != 7], pred[y != 7]), 1e-12)
        assert same(got["ex_f1"], f1_score(y[y != 7], pred[y != 7], average="macro"), 1e-12)
    assert abs(metrics.avg_loss - np.mean(losses)) <= 1e-6 * max(1.0, abs(np.mean(losses)))
    assert same(metrics.total_score("ALL", scores), got["ex_score"] + got["au_score"] + got["va_score"], 1e-15)


def test_captured_forward_losses_and_update_replay_to_the_eager_state():
    """ONE capture in this file's process (a second end-of-capture in one process has crashed the runtime before)"""
    import avformer_amd as A
    torch.manual_seed(0)
    B, k = 8, 3
    m = A.build_model("sformer", task="ALL", task_losses="reference").cuda().eval()
    data = [_sformer_inputs(B, 80 + i) for i in range(k)]
    x = {"clip": data[0][0].cuda()}
    labels = _cuda(data[0][1])

    def step(metrics):
        with torch.no_grad():
            out = m(x)
            ls = m.get_mt_loss(out, labels)
            metrics.update(out, labels, ls[0] + ls[1] + ls[2])

    def load(i):
        x["clip"].copy_(data[i][0])
        for key in labels:
            labels[key].copy_(data[i][1][key])

    eager = A.EvalMetrics(device="cuda")
    for i in range(k):
        load(i)
        step(eager)
    torch.cuda.synchronize()
    replayed = A.EvalMetrics(device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(replayed)
    torch.cuda.current_stream().wait_stream(side)
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(replayed)
    replayed.clear()
    for i in range(k):
        load(i)
        graph.replay()
    torch.cuda.synchronize()
    print("eager", flat_scores(eager.scores()), "replayed", flat_scores(replayed.scores()))
    assert torch.equal(replayed.state, eager.state) and float(eager.state[122]) == k
