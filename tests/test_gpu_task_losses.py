"""-m gpu: the fused EX / AU / VA loss kernel (csrc/task_loss.hip) and everything built on it.

Parity: value and gradient of every criterion - alone and fused - against fixture G17, i.e. against the reference's own
models/loss.py, within the project's bounds for a loss kernel (test_gpu_ops.py::test_au_loss_golden): loss atol 1e-6 / rtol
1e-5, gradient atol 1e-7 / rtol 1e-5; NaN and exact-zero results compared by kind.  Size and layout: 1, 255, 256, 257 and 4096
rows against the plain-torch restatement evaluated in fp64, same bounds; a strided, 24-wide row; zeros outside the blocks and in
the block of a task without labels; the fused call bit-identical to the three criteria called one by one.  Training: the
``sformer`` multi-task step backpropagates into both heads and the token section, contains no host synchronisation, and
replays from a captured graph to the eager values."""

import pytest
import torch

from conftest import load_golden
from task_loss_util import AU, CRITERIA, EX, GRAD_TOL, LOSS_TOL, VA, assert_same_kind_close, fixture_pairs, loss_and_grad

pytestmark = pytest.mark.gpu

G = load_golden("g17_task_losses")
# (EX criterion, AU criterion, VA weights, their fixture keys): the recipes of sformer and avformer
RECIPES = {"sformer": ("ce", "dice", (1.0, 1.0), "va11"), "avformer": ("focal", "aubce", (2.0, 1.0), "va21")}


def _mt(recipe):
    import avformer_amd as A
    ex, au, w, _ = RECIPES[recipe]
    return A.MultiTaskLoss(CRITERIA[ex]["make"](), CRITERIA[au]["make"](), A.CCCLoss(), w)


@pytest.mark.parametrize("case,name", fixture_pairs(G))
def test_criterion_alone_matches_the_reference(case, name):
    spec = CRITERIA[name]
    crit, y = spec["make"]().cuda(), G[f"{case}.{spec['label']}"].cuda()
    for form in ("rows", "alone"):
        if form not in spec:
            continue
        loss, grad = loss_and_grad(lambda o: spec[form](crit, o, y), G[f"{case}.out"].cuda())
        d = (grad[:, spec["cols"]].cpu() - G[f"{case}.{name}.dout"]).abs().nan_to_num(0).max()
        print(f"{case}.{name}.{form}: loss {float(loss):.9g} (fixture {float(G[f'{case}.{name}.loss']):.9g}), max |d grad| {float(d):.3g}")
        assert_same_kind_close(loss, G[f"{case}.{name}.loss"], f"{case}.{name}.{form} loss", **LOSS_TOL)
        assert_same_kind_close(grad[:, spec["cols"]], G[f"{case}.{name}.dout"], f"{case}.{name}.{form} gradient", **GRAD_TOL)
        rest = torch.ones(21, dtype=torch.bool)
        rest[spec["cols"]] = False
        assert float(grad[:, rest].abs().max()) == 0.0


@pytest.mark.parametrize("recipe", sorted(RECIPES))
@pytest.mark.parametrize("case", ["b16", "b64", "mix", "exign", "va1"])
def test_fused_three_match_the_reference(case, recipe):
    ex, au, _, va = RECIPES[recipe]
    mt = _mt(recipe)
    out = G[f"{case}.out"].cuda().requires_grad_(True)
    ls = mt(out, G[f"{case}.y_ex"].cuda(), G[f"{case}.y_au"].cuda(), G[f"{case}.y_va"].cuda())
    for k, (name, cols) in enumerate(((ex, EX), (au, AU), (va, VA))):
        (g,) = torch.autograd.grad(ls[k], out, retain_graph=True)
        print(f"{case}.{recipe}[{name}]: loss {float(ls[k]):.9g} (fixture {float(G[f'{case}.{name}.loss']):.9g})")
        assert_same_kind_close(ls[k], G[f"{case}.{name}.loss"], f"{case}.{name} fused loss", **LOSS_TOL)
        assert_same_kind_close(g[:, cols], G[f"{case}.{name}.dout"], f"{case}.{name} fused gradient", **GRAD_TOL)
        rest = torch.ones(21, dtype=torch.bool)
        rest[cols] = False
        assert float(g[:, rest].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["b64", "mix"])
@pytest.mark.parametrize("key,normalize", [("mt", False), ("mtn", True)])
def test_get_mt_loss_matches_the_reference_sformer(case, key, normalize):
    import avformer_amd as A
    m = A.build_model("sformer", task="ALL", task_losses="reference").cuda()
    labels = {"EX": G[f"{case}.y_ex"].cuda(), "AU": G[f"{case}.y_au"].cuda(), "VA": G[f"{case}.y_va"].cuda()}
    out = G[f"{case}.out"].cuda().requires_grad_(True)
    ls = m.get_mt_loss(out, labels, normalize=normalize)
    (3 * ls[0] + ls[1] + ls[2]).backward()
    print(f"{case}.{key}: {[float(l) for l in ls]} (fixture {G[f'{case}.{key}.loss'].tolist()})")
    assert_same_kind_close(torch.stack([l.detach() for l in ls]), G[f"{case}.{key}.loss"], f"{case}.{key} list", **LOSS_TOL)
    assert_same_kind_close(out.grad, G[f"{case}.{key}.dout"], f"{case}.{key} gradient", **GRAD_TOL)


def _random_batch(rows, seed, width=21):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(rows, width, generator=g)
    y_ex = torch.randint(0, 8, (rows,), generator=g)                 # 7 = ignored, one row in eight
    y_au = (torch.rand(rows, 12, generator=g) > 0.6).float()
    y_au[torch.rand(rows, generator=g) < 0.15] = -1                  # dropped rows
    y_au[:, 5][torch.rand(rows, generator=g) < 0.1] = -1             # unlabelled units inside kept rows
    y_va = torch.rand(rows, 2, generator=g) * 2 - 1
    y_va[torch.rand(rows, 2, generator=g) < 0.15] = -5.0
    if rows == 1:                                                    # one row: keep it valid for EX and AU
        y_ex[0], y_au[0, 0] = 3, 1.0
    return out, y_ex, y_au, y_va


@pytest.mark.parametrize("recipe", sorted(RECIPES))
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 4096])
@pytest.mark.parametrize("normalize", [False, True])
def test_sizes_against_the_fp64_restatement(rows, recipe, normalize):
    mt = _mt(recipe)
    out, y_ex, y_au, y_va = _random_batch(rows, 100 + rows)
    o64 = out.double().requires_grad_(True)
    ref = mt.forward_torch(o64, y_ex, y_au, y_va, normalize=normalize)
    og = out.cuda().requires_grad_(True)
    ls = mt(og, y_ex.cuda(), y_au.cuda(), y_va.cuda(), normalize=normalize)
    for k, cols in enumerate((EX, AU, VA)):
        (g,) = torch.autograd.grad(ls[k], og, retain_graph=True)
        g64 = torch.autograd.grad(ref[k], o64, retain_graph=True, allow_unused=True)[0] if ref[k].requires_grad else None
        g64 = torch.zeros_like(o64) if g64 is None else g64
        print(f"rows {rows} {recipe} normalize {normalize} [{k}]: loss {float(ls[k]):.9g} fp64 {float(ref[k]):.12g}  "
              f"max |d grad| {float((g.cpu().double() - g64).abs().max()):.3g} of {float(g64.abs().max()):.3g}")
        assert_same_kind_close(ls[k], ref[k], f"rows {rows} loss {k}", **LOSS_TOL)
        assert_same_kind_close(g, g64, f"rows {rows} gradient {k}", **GRAD_TOL)


def test_counts_and_all_dropped_au_rows():
    """counts = valid EX rows, AU labels != -1, VA labels != -5 (get_mt_loss(normalize=True), sformer.py:427-447); every AU
    row dropped gives NaN with a zero gradient, as the reference's mean over an empty selection"""
    import avformer_amd as A
    out, y_ex, y_au, y_va = _random_batch(300, 7)
    mt = _mt("sformer")
    losses, counts, grad = A.ops.task_loss(out.cuda(), y_ex.cuda(), y_au.cuda(), y_va.cuda(), mt._cfg(False))
    assert counts.tolist() == [float((y_ex != 7).sum()), float((y_au != -1).sum()), float((y_va != -5).sum())]
    for recipe in RECIPES:
        og = out.cuda().requires_grad_(True)
        l_au = _mt(recipe)(og, y_au=-torch.ones(300, 12).cuda())[1]
        l_au.backward()
        assert bool(torch.isnan(l_au)) and float(og.grad.abs().max()) == 0.0
        ref = _mt(recipe).forward_torch(out.double(), y_au=-torch.ones(300, 12))[1]
        assert bool(torch.isnan(ref))
    zero = _mt("avformer")(out.cuda(), y_ex.cuda().fill_(7), -torch.ones(300, 12).cuda(), torch.full((300, 2), -5.0).cuda(),
                           normalize=True)
    assert [float(z) for z in zero] == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_layout_strided_rows_null_labels_and_bit_identity(recipe):
    import avformer_amd as A
    ex, au, w, _ = RECIPES[recipe]
    mt = _mt(recipe)
    out, y_ex, y_au, y_va = _random_batch(77, 5, width=30)
    wide = out.cuda()[:, :24]                                        # 24 columns, rows 30 floats apart
    assert wide.stride() == (30, 1)
    ye, ya, yv = y_ex.cuda(), y_au.cuda(), y_va.cuda()
    cfg = mt._cfg(False)
    losses, counts, grad = A.ops.task_loss(wide, ye, ya, yv, cfg)
    l_c, c_c, grad_c = A.ops.task_loss(wide.contiguous(), ye, ya, yv, cfg)
    assert grad.shape == (77, 24) and grad.is_contiguous()
    assert torch.equal(losses, l_c) and torch.equal(grad, grad_c) and float(grad[:, 21:].abs().max()) == 0.0
    ref = mt.forward_torch(out[:, :24].double(), y_ex, y_au, y_va)
    for k in range(3):
        assert_same_kind_close(losses[k], ref[k], f"strided loss {k}", **LOSS_TOL)
    # a task without labels: loss 0, its block zero, the other blocks unchanged - bit for bit
    for off in range(3):
        lab = [ye, ya, yv]
        lab[off] = None
        l_o, _, g_o = A.ops.task_loss(wide, *lab, cfg)
        cols = (EX, AU, VA)[off]
        keep = torch.ones(24, dtype=torch.bool)
        keep[cols] = False
        assert float(l_o[off]) == 0.0 and float(g_o[:, cols].abs().max()) == 0.0
        assert torch.equal(g_o[:, keep], grad[:, keep]) and all(torch.equal(l_o[k], losses[k]) for k in range(3) if k != off)
    # the fused call against the three criteria called one by one, values and gradients
    crits = (CRITERIA[ex]["make"]().cuda(), CRITERIA[au]["make"]().cuda(), A.CCCLoss())
    og = out[:, :21].contiguous().cuda().requires_grad_(True)
    fused = mt(og, ye, ya, yv)
    (2.0 * fused[0] + 3.0 * fused[1] + 5.0 * fused[2]).backward()
    o1 = out[:, :21].contiguous().cuda().requires_grad_(True)
    # (an AULoss module called directly runs its own, older kernel - au_loss_kernel -; on the fused kernel it is the AU task alone)
    single = [crits[0].forward_rows(o1, ye), crits[1].forward_rows(o1, ya) if isinstance(crits[1], A.DiceAULoss) else mt(o1, y_au=ya)[1],
              crits[2].forward_rows(o1, yv, w)]
    (2.0 * single[0] + 3.0 * single[1] + 5.0 * single[2]).backward()
    assert all(torch.equal(a, b) for a, b in zip(fused, single)) and torch.equal(og.grad, o1.grad)
    # backward with one incoming gradient only: the other blocks are zero
    og.grad = None
    mt(og, ye, ya, yv)[1].backward()
    assert float(og.grad[:, 12:].abs().max()) == 0.0 and float(og.grad[:, :12].abs().max()) > 0.0


def _sformer_step(m, x, labels):
    """forward, get_mt_loss for normalize False and True, backward of train.py:147's weighting of both lists"""
    out = m(x)
    ls = m.get_mt_loss(out, labels, normalize=False) + m.get_mt_loss(out, labels, normalize=True)
    (3 * ls[0] + ls[1] + ls[2] + 3 * ls[3] + ls[4] + ls[5]).backward()
    return torch.stack([l.detach() for l in ls])


def test_sformer_multi_task_step_trains_and_replays_from_a_graph():
    import gc

    import avformer_amd as A
    torch.manual_seed(0)
    B = 8
    g = torch.Generator().manual_seed(3)
    x = {"clip": torch.randn(B, 256, 7, 7, generator=g).cuda()}
    y_ex = torch.randint(0, 8, (B,), generator=g)
    y_ex[0] = 2
    y_au = (torch.rand(B, 12, generator=g) > 0.5).float()
    y_au[1] = -1
    y_va = torch.rand(B, 2, generator=g) * 2 - 1
    y_va[2] = -5.0
    labels = {"EX": y_ex.cuda(), "AU": y_au.cuda(), "VA": y_va.cuda()}
    m = A.build_model("sformer", task="ALL", task_losses="reference").cuda().train()
    vals = _sformer_step(m, x, labels)
    assert bool(torch.isfinite(vals).all())
    grads = {n: p.grad for n, p in m.named_parameters()}
    for n in ("fc.3.weight", "fc.1.weight", "base_model.pos_embedding", "base_model.spatial_transformer.layers.0.0.fn.fn.to_qkv.weight"):
        assert grads[n] is not None and bool(torch.isfinite(grads[n]).all()) and float(grads[n].abs().sum()) > 0, n
    # task 'AU' routes the AU columns through au_head (sformer.py:382-384): the Dice + BCE gradient reaches it
    m_au = A.build_model("sformer", task="AU", task_losses="reference").cuda().train()
    _sformer_step(m_au, x, labels)
    g_au = [p.grad for n, p in m_au.named_parameters() if n.startswith("au_head.") and p.grad is not None]
    assert g_au and all(bool(torch.isfinite(t).all()) for t in g_au) and sum(float(t.abs().sum()) for t in g_au) > 0
    del m_au, g_au, grads

    # no host synchronisation inside get_mt_loss (forward and backward of the loss), normalize False and True
    m.eval()   # no dropout, BatchNorm on its running statistics: replay and eager compute the same thing
    out = m(x)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ls = m.get_mt_loss(out, labels, normalize=False) + m.get_mt_loss(out, labels, normalize=True)
        total = 3 * ls[0] + ls[1] + ls[2] + 3 * ls[3] + ls[4] + ls[5]
        (d_out,) = torch.autograd.grad(total, out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(d_out).all())
    del out, ls, total, d_out

    # one capture, one replay
    for p in m.parameters():
        p.grad = None
    eager = _sformer_step(m, x, labels).clone()
    eager_grad = m.fc[3].weight.grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for p in m.parameters():
            p.grad = None
        _sformer_step(m, x, labels)
    torch.cuda.current_stream().wait_stream(side)
    for p in m.parameters():
        p.grad = None
    gc.collect()   # nothing left over from earlier tests is released while the stream is capturing
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_vals = _sformer_step(m, x, labels)
    graph.replay()
    torch.cuda.synchronize()
    print(f"eager {eager.tolist()} replay {static_vals.tolist()}")
    assert torch.equal(static_vals, eager) and torch.equal(m.fc[3].weight.grad, eager_grad)


def test_launch_count_of_get_mt_loss():
    """one launch forward, one backward: counted with the profiler on the loss alone"""
    import avformer_amd as A
    from torch.profiler import ProfilerActivity, profile
    m = A.build_model("sformer", task="ALL", task_losses="reference").cuda()
    labels = {"EX": G["mix.y_ex"].cuda(), "AU": G["mix.y_au"].cuda(), "VA": G["mix.y_va"].cuda()}
    out = G["mix.out"].cuda().requires_grad_(True)
    for normalize in (False, True):
        ls = m.get_mt_loss(out, labels, normalize=normalize)       # warm-up
        torch.autograd.grad(ls, out, [torch.ones_like(l) for l in ls])
        g = [torch.ones_like(l) for l in ls]
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            ls = m.get_mt_loss(out, labels, normalize=normalize)
            torch.autograd.grad(ls, out, g)
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                   and "Memset" not in e.name]
        print(f"normalize {normalize}: {kernels}")
        assert len(kernels) == 2 and "task_loss_kernel" in kernels[0] and "task_loss_bwd_kernel" in kernels[1], kernels
