"""FusedAdam's on-device step control (csrc/grad_control.hip): gradient clipping, learning-rate warm-up and the lr scale.
The comparison target is always torch on the same gradients: ``clip_grad_norm_`` + ``torch.optim.Adam`` (+ ``LambdaLR``)."""
import copy
import ctypes as C
import math

import pytest
import torch

from gpu_util import DEV, rel_fro
from test_gpu_optim import _models

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23   # one fp32 unit in the last place, relative: the norm is accumulated in fp64, only its final rounding is left
KW = dict(lr=3e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=1e-2)


def _batch(g, dims, B=3):
    Tv, Ta, D = dims
    return ({"clip": torch.randn(B, Tv, D, generator=g).to(DEV), "audio_features": torch.randn(B, Ta, D, generator=g).to(DEV)},
            (torch.rand(B, 12, generator=g) > 0.5).float().to(DEV))


def _backward(m, batch, labels):
    for p in m.parameters():
        p.grad = None
    m.get_au_loss(m(batch), labels).backward()


def _norm64(m):
    return math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in m.parameters() if p.grad is not None))


def _share_grads(ma, mb):
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        pb.grad = None if pa.grad is None else pa.grad.detach().clone()


def _assert_params_close(ma, mb, tag, bound=2e-6):
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert rel_fro(pa, pb) < bound, (tag, n, rel_fro(pa, pb))


def _clipped_steps(mode, dims, steps):
    """`steps` updates of FusedAdam(max_grad_norm = 0.25 x the first norm) and of clip_grad_norm_ + torch Adam on the same
    gradients; every step checks the norm, the untouched .grad tensors and the parameters"""
    A, ma, mb, shape = _models(mode, dims)
    g = torch.Generator().manual_seed(4)
    oa = ob = max_norm = None
    for it in range(steps):
        batch, labels = _batch(g, shape)
        _backward(ma, batch, labels)
        ref = _norm64(ma)
        if it == 0:
            max_norm = 0.25 * ref
            oa = A.optim.FusedAdam(ma, max_grad_norm=max_norm, **KW)
            ob = torch.optim.Adam(mb.parameters(), **KW)
        _share_grads(ma, mb)
        before = [None if p.grad is None else p.grad.clone() for p in ma.parameters()]
        torch.nn.utils.clip_grad_norm_(mb.parameters(), max_norm)
        oa.step()
        ob.step()
        for p, b in zip(ma.parameters(), before):   # the gradients in memory keep their unclipped values
            assert (p.grad is None and b is None) or torch.equal(p.grad, b)
        norm, coef = float(oa.grad_norm), float(oa.clip_coef)
        print(f"[{mode} {dims}] step {it}: norm {norm!r} fp64 {ref!r} rel {abs(norm - ref) / ref:.3e} coef {coef!r}")
        assert abs(norm - ref) / ref <= ULP, (it, norm, ref)
        assert coef < 0.5 if it == 0 else coef < 1.0, (it, coef)
        _assert_params_close(ma, mb, it)
    return A, ma, mb, oa, ob, batch


@pytest.mark.parametrize("mode,dims", [("f32", (64, 2, 2, 32, 96, 9, 7)), ("bf16", (64, 2, 2, 32, 96, 9, 7)),
                                       ("f32", (36, 1, 3, 16, 52, 5, 4))])   # widths 36 / 52: odd offsets in the bucket
def test_clipped_step_matches_clip_grad_norm_and_torch_adam(mode, dims):
    A, ma, mb, oa, ob, batch = _clipped_steps(mode, dims, 4)
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        sa, sb = oa.state[pa], ob.state[pb]
        assert float(sa["step"]) == float(sb["step"]) == 4.0
        assert rel_fro(sa["exp_avg"], sb["exp_avg"]) < 1e-5
        assert rel_fro(sa["exp_avg_sq"], sb["exp_avg_sq"]) < 1e-5
    if mode == "bf16":
        # the copies written by the clipped step are exactly what a fresh preparation pass produces
        st = ma.transformer
        assert st._lowp_ready
        kept = [b.clone() for b in st._lowp_bufs]
        st.refresh_weights()
        with torch.no_grad():
            ma(batch)
        for x, y in zip(kept, st._lowp_bufs):
            assert torch.equal(x, y)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_inactive_clipping_is_bitwise_the_unclipped_step(mode):
    A, ma, mb, shape = _models(mode)
    g = torch.Generator().manual_seed(6)
    oa = ob = None
    for it in range(3):
        batch, labels = _batch(g, shape)
        _backward(ma, batch, labels)
        if it == 0:
            oa = A.optim.FusedAdam(ma, max_grad_norm=1e6 * _norm64(ma), **KW)
            ob = A.optim.FusedAdam(mb, **KW)
        _share_grads(ma, mb)
        oa.step()
        ob.step()
        assert float(oa.clip_coef) == 1.0
        for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            assert torch.equal(pa, pb), (it, n)
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
        assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
    assert ob._ctl is None   # the default optimizer never built a control block


def test_default_step_makes_no_control_call(monkeypatch):
    """defaults and an untouched lr scale: neither avf_grad_control nor avf_adam_batch_control is called"""
    A, ma, _, shape = _models("bf16")
    from avformer_amd import _lib
    real = _lib.load()
    called = []

    class Spy:
        def __getattr__(self, name):
            if name in ("avf_grad_control", "avf_adam_batch_control"):
                called.append(name)
            return getattr(real, name)

    opt = A.optim.FusedAdam(ma, **KW)
    _backward(ma, *_batch(torch.Generator().manual_seed(2), shape))
    monkeypatch.setattr(_lib, "load", lambda *a, **k: Spy())
    opt.step()
    assert called == []
    opt.set_lr_scale(1.0)   # touching the scale switches the control block on
    opt.step()
    assert called == ["avf_grad_control", "avf_adam_batch_control"]


def test_warmup_and_lr_scale_match_lambda_lr():
    A, ma, mb, shape = _models("f32")
    oa = A.optim.FusedAdam(ma, n_warmup_steps=4, **KW)
    ob = torch.optim.Adam(mb.parameters(), **KW)
    scale = {"v": 1.0}
    sched = torch.optim.lr_scheduler.LambdaLR(ob, lambda s: min(1.0, (s + 1) / 4) * scale["v"])
    g = torch.Generator().manual_seed(7)
    for it in range(6):
        batch, labels = _batch(g, shape)
        _backward(ma, batch, labels)
        _share_grads(ma, mb)
        if it == 4:   # before step 5
            oa.set_lr_scale(0.1)
        oa.step()
        ob.step()
        if it == 3:
            scale["v"] = 0.1
        sched.step()
        assert float(oa._ctl[0]) == pytest.approx(min(1.0, (it + 1) / 4) * (0.1 if it >= 4 else 1.0), rel=1e-6)
        assert float(oa.grad_norm) == 0.0 and float(oa.clip_coef) == 1.0   # clipping is off
        _assert_params_close(ma, mb, it)
    # a 0-dim device tensor is taken as well
    oa.set_lr_scale(torch.tensor(0.25, device=DEV))
    assert float(oa._ctl[3]) == 0.25
    assert oa.state_dict()["param_groups"][0]["lr_scale"] == 0.25


def test_more_tensors_than_one_descriptor_table():
    """14 layers x 11 tensors + the loose ones > 143: the norm kernel and the Adam session both launch a second table"""
    dims = (16, 14, 1, 8, 16, 3, 2)
    A, ma, mb, oa, ob, _ = _clipped_steps("f32", dims, 2)
    assert sum(1 for p in ma.parameters() if p.grad is not None) > 143


# ---- the kernels through the C ABI --------------------------------------------------------------------------------------
def _raw(tensors, max_norm=1.0, n_warmup=0, step=None, scale=1.0, numel=None):
    """avf_grad_control on a hand-built list (None: a null pointer) -> the four control floats (CPU).  The workspace and the
    outputs are poisoned first: nothing may rely on a cleared buffer."""
    from avformer_amd import _lib
    lib = _lib.load()
    n = len(tensors)
    numel = numel or [5 if t is None else t.numel() for t in tensors]
    ptrs = (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tensors]) if n else None
    sizes = (C.c_int64 * n)(*numel) if n else None
    nbytes = lib.avf_grad_control_workspace_bytes(n, sizes)
    ws = torch.full((max(1, nbytes // 8),), float("nan"), dtype=torch.float64, device=DEV)
    ctl = torch.tensor([7.0, 7.0, 7.0, scale], dtype=torch.float32, device=DEV)
    st = None if step is None else torch.tensor([float(step)], dtype=torch.float32, device=DEV)
    _lib.check(lib.avf_grad_control(n, ptrs, sizes, max_norm, n_warmup, None if st is None else C.c_void_p(st.data_ptr()),
                                    C.c_void_p(ctl.data_ptr()), C.c_void_p(ws.data_ptr()) if nbytes else None,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "grad_control")
    torch.cuda.synchronize()
    return ctl.cpu()


def _check_raw(tensors, tag, max_norm=1.0):
    ctl = _raw(tensors, max_norm)
    ref = math.sqrt(sum(float(t.double().pow(2).sum()) for t in tensors if t is not None))
    norm, coef = float(ctl[2]), float(ctl[1])
    print(f"[{tag}] norm {norm!r} fp64 {ref!r} coef {coef!r}")
    assert abs(norm - ref) <= ULP * ref, (tag, norm, ref)
    want = float(torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (ctl[2] + 1e-6), max=1.0))   # torch's formula, fp32
    assert abs(coef - want) <= ULP * want, (tag, coef, want)
    assert float(ctl[0]) == 1.0 and float(ctl[3]) == 1.0
    return ctl


@pytest.mark.parametrize("numel", [1, 3, 4095, 4096, 4097, 12289])
def test_raw_single_tensor(numel):
    g = torch.Generator().manual_seed(numel)
    _check_raw([(3.0 * torch.randn(numel, generator=g)).to(DEV)], f"numel {numel}")


def test_raw_edges():
    g = torch.Generator().manual_seed(11)
    r = lambda n: (3.0 * torch.randn(n, generator=g)).to(DEV)
    buf = r(5001)
    assert buf.data_ptr() % 16 == 0
    _check_raw([buf[1:]], "4 bytes past a 16-byte boundary")              # second work item is misaligned as well
    _check_raw([buf[2:9], buf[3:4100]], "short and long views at odd offsets")
    _check_raw([r(100), None, r(4100)], "null pointer in the middle")
    _check_raw([r(7), torch.empty(0, device=DEV), r(9)], "zero-numel tensor")
    many = [r(1 + (i % 5)) for i in range(300)]                            # three descriptor tables
    _check_raw(many, "300 tensors")
    # count = 0 with clipping on: norm 0, multiplier 1
    ctl = _raw([], 1.0)
    assert float(ctl[2]) == 0.0 and float(ctl[1]) == 1.0
    # clipping off: nothing is read (count 0, no workspace), warm-up and scale still apply
    ctl = _raw([], 0.0, n_warmup=4, step=3, scale=0.5)
    assert ctl.tolist() == [0.375, 1.0, 0.0, 0.5]
    assert _raw([], -1.0, n_warmup=4, step=9, scale=0.5).tolist() == [0.5, 1.0, 0.0, 0.5]
    # the same input twice: the same bits
    t = [r(12289), buf[1:]]
    a, b = _raw(t, 0.5), _raw(t, 0.5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # NaN / inf follow torch: a NaN norm is a NaN multiplier (not swallowed by a min), an infinite norm gives 0
    bad = r(5000)
    bad[4321] = float("nan")
    ctl = _raw([bad], 1.0)
    assert math.isnan(float(ctl[1])) and math.isnan(float(ctl[2]))
    bad[4321] = float("inf")
    ctl = _raw([bad], 1.0)
    assert float(ctl[1]) == 0.0 and float(ctl[2]) == float("inf")


def test_non_finite_gradient_follows_torch():
    A, ma, mb, shape = _models("f32")
    oa = A.optim.FusedAdam(ma, max_grad_norm=1.0, **KW)
    ob = torch.optim.Adam(mb.parameters(), **KW)
    _backward(ma, *_batch(torch.Generator().manual_seed(9), shape))
    victim = max((p for p in ma.parameters() if p.grad is not None), key=lambda p: p.numel())
    victim.grad.view(-1)[17] = float("inf")
    _share_grads(ma, mb)
    torch.nn.utils.clip_grad_norm_(mb.parameters(), 1.0)
    oa.step()
    ob.step()
    assert float(oa.grad_norm) == float("inf") and float(oa.clip_coef) == 0.0
    bad = 0
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        fa, fb = torch.isfinite(pa), torch.isfinite(pb)
        assert torch.equal(fa, fb), n
        bad += int((~fa).sum())
        assert rel_fro(pa[fa], pb[fb]) < 2e-6, n
    assert bad == 1   # inf * 0 = NaN at the one element, plain arithmetic everywhere else
    # a NaN element: NaN norm, NaN multiplier
    victim.grad.view(-1)[17] = float("nan")
    oa.step()
    assert math.isnan(float(oa.clip_coef)) and math.isnan(float(oa.grad_norm))


def test_captured_step_follows_warmup_clipping_and_lr_scale():
    """GraphedTrainStep with clipping and a warm-up that is still running when the step is captured: every replay must be
    bitwise the eager twin's step - it is not if lr or the multiplier were baked in at capture"""
    import avformer_amd as A
    dims = (64, 2, 2, 32, 96, 9, 7)
    _, m_g, m_e, shape = _models("bf16", dims)

    def loss_fn(m, b):
        return m.get_au_loss(m({"clip": b["clip"], "audio_features": b["audio_features"]}), b["labels"])

    def batch(seed):
        b, labels = _batch(torch.Generator().manual_seed(seed), shape, B=4)
        return dict(b, labels=labels)

    probe = copy.deepcopy(m_e)
    loss_fn(probe, batch(1)).backward()
    max_norm = 0.25 * _norm64(probe)
    kw = dict(max_grad_norm=max_norm, n_warmup_steps=3, **KW)
    opt_g, opt_e = A.optim.FusedAdam(m_g, **kw), A.optim.FusedAdam(m_e, **kw)

    def eager(b):
        opt_e.zero_grad(set_to_none=True)
        loss_fn(m_e, b).backward()
        opt_e.step()

    gs = A.graphs.GraphedTrainStep(m_g, opt_g, loss_fn, batch(1), warmup=1)   # update 1 eager; replays are updates 2, 3, ...
    eager(batch(1))
    for i in range(6):
        if i == 5:
            opt_g.set_lr_scale(0.5)
            opt_e.set_lr_scale(0.5)
        b = batch(30 + i)
        gs(b)
        eager(b)
        torch.cuda.synchronize()
        for (n, p), q in zip(m_g.named_parameters(), m_e.parameters()):
            assert torch.equal(p, q), (i, n)
        assert torch.equal(opt_g._ctl, opt_e._ctl), i
        assert float(opt_g.clip_coef) < 1.0
        want = min(1.0, (i + 2) / 3) * (0.5 if i == 5 else 1.0)
        assert float(opt_g._ctl[0]) == pytest.approx(want, rel=1e-6), i
