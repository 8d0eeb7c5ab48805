"""CPU (no GPU needed): the EX / AU / VA criteria and the multi-task loss against fixture G17, which holds what the
reference's models/loss.py computes (tests/golden/make_golden_task_losses.py).  The plain-torch form of every criterion
reproduces each case in fp32, and in fp64 it agrees with the fp32 fixture within the same bounds - the project's bounds for a
loss kernel (test_gpu_ops.py::test_au_loss_golden): loss atol 1e-6 / rtol 1e-5, gradient atol 1e-7 / rtol 1e-5.  The reference's
own fp32 results lie within 1e-7 (loss) and 3e-7 of the largest gradient of an fp64 run, so it stays inside them.  NaN and
exact-zero results are compared by kind.  Also: the registry builds the four models with the reference's criteria, and the C
entry point refuses bad layouts on the host, before anything is launched."""
import ctypes
import math

import pytest
import torch

import avformer_amd as A
from conftest import load_golden
from task_loss_util import (CASES, CRITERIA, GRAD_TOL, LOSS_TOL, assert_same_kind_close, fixture_pairs, loss_and_grad)

G = load_golden("g17_task_losses")


def test_fixture_holds_the_cases_of_the_issue():
    assert all(f"{c}.out" in G for c in CASES)
    assert G["b16.out"].shape == (16, 21) and G["b64.out"].shape == (64, 21) and G["mix.out"].shape == (64, 21)
    assert bool((G["exign.y_ex"] == 7).all())
    assert int((G["va1.y_va"][:, 0] != -5).sum()) == 1 and int((G["va1.y_va"][:, 1] != -5).sum()) == 1
    y = G["mix.y_au"]
    assert bool((G["mix.y_ex"] == 7).any()) and bool((y[:, 0] == -1).any()) and bool((G["mix.y_va"] == -5).any())
    assert bool(((y[:, 0] != -1) & (y[:, 1:] == -1).any(1)).any())   # -1 inside a kept row
    assert math.isnan(G["exign.ce.loss"]) and math.isnan(G["exign.focal.loss"])   # (0-dim entries load as floats)
    assert float(G["va1.va21.loss"]) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case,name", fixture_pairs(G))
def test_plain_torch_form_reproduces_the_reference(case, name, dtype):
    spec = CRITERIA[name]
    crit, y = spec["make"](), G[f"{case}.{spec['label']}"]
    loss, grad = loss_and_grad(lambda o: spec["torch"](crit, o, y), G[f"{case}.out"].to(dtype))
    print(f"{case}.{name}[{dtype}]: loss {float(loss):.9g} (fixture {float(G[f'{case}.{name}.loss']):.9g}), "
          f"max |d grad| {float((grad[:, spec['cols']] - G[f'{case}.{name}.dout']).abs().nan_to_num(0).max()):.3g}")
    assert_same_kind_close(loss, G[f"{case}.{name}.loss"], f"{case}.{name} loss", **LOSS_TOL)
    assert_same_kind_close(grad[:, spec["cols"]], G[f"{case}.{name}.dout"], f"{case}.{name} gradient", **GRAD_TOL)
    rest = torch.ones(21, dtype=torch.bool)
    rest[spec["cols"]] = False
    assert float(grad[:, rest].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", ["b64", "mix"])
@pytest.mark.parametrize("key,normalize", [("mt", False), ("mtn", True)])
def test_get_mt_loss_is_the_list_of_the_reference_sformer(case, key, normalize, dtype):
    """SpatialFormer.get_mt_loss (sformer.py:423-449) and the gradient of train.py:147's 3 ex + au + va; the default
    task_losses="plain" model serves get_mt_loss with the same criteria"""
    labels = {"EX": G[f"{case}.y_ex"], "AU": G[f"{case}.y_au"], "VA": G[f"{case}.y_va"]}
    for task_losses in ("reference", "plain"):
        m = A.build_model("sformer", task="ALL", task_losses=task_losses)
        out = G[f"{case}.out"].to(dtype).clone().requires_grad_(True)
        ls = m.get_mt_loss(out, labels, normalize=normalize)
        assert isinstance(ls, list) and len(ls) == 3
        (3 * ls[0] + ls[1] + ls[2]).backward()
        assert_same_kind_close(torch.stack([l.detach() for l in ls]), G[f"{case}.{key}.loss"], f"{case}.{key} list", **LOSS_TOL)
        assert_same_kind_close(out.grad, G[f"{case}.{key}.dout"], f"{case}.{key} gradient", **GRAD_TOL)


def test_normalize_with_a_count_of_zero_gives_a_zero_loss():
    m = A.build_model("avformer", task="ALL", task_losses="reference")
    out = G["exign.out"].clone().requires_grad_(True)
    labels = {"EX": G["exign.y_ex"], "AU": -torch.ones(16, 12), "VA": torch.full((16, 2), -5.0)}
    ls = m.get_mt_loss(out, labels, normalize=True)
    assert [float(l.detach()) for l in ls] == [0.0, 0.0, 0.0]
    (ls[0] + ls[1] + ls[2]).backward()
    assert float(out.grad.abs().max()) == 0.0


RECIPES = {"avformer": (A.FocalLoss_Ori, A.AULoss, (2.0, 1.0)), "sformer": (A.CrossEntropyEX, A.DiceAULoss, (1.0, 1.0)),
           "vformer": (A.CrossEntropyEX, A.AULoss, (2.0, 1.0)), "tformer": (A.CrossEntropyEX, A.AULoss, (2.0, 1.0))}


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_registry_builds_the_reference_criteria(name):
    m = A.build_model(name, task="ALL", task_losses="reference")
    ex, au, w = RECIPES[name]
    assert type(m.loss_EX) is ex and type(m.loss_AU) is au and type(m.loss_VA) is A.CCCLoss and m.loss_MT.va_weights == w
    assert m.loss_EX.ignore_index == 7 and hasattr(m, "get_mt_loss") and m.task == "ALL"
    plain = A.build_model(name, task="ALL")
    assert plain.task_losses == "plain" and type(plain.loss_AU) is A.AULoss and not hasattr(plain, "loss_EX")
    assert hasattr(plain, "get_mt_loss") and list(plain.state_dict()) == list(m.state_dict())
    with pytest.raises(ValueError):
        A.build_model(name, task="ALL", task_losses="other")
    # the weights of valence and arousal, and the EX objective, reach get_va_loss / get_ex_loss
    out, y_va, y_ex = G["mix.out"], G["mix.y_va"], G["mix.y_ex"]
    ccc = A.CCCLoss()
    want = w[0] * ccc(torch.tanh(out[:, 19]), y_va[:, 0]) + w[1] * ccc(torch.tanh(out[:, 20]), y_va[:, 1])
    torch.testing.assert_close(m.get_va_loss(out, y_va), want, **LOSS_TOL)
    assert_same_kind_close(m.get_ex_loss(out, y_ex), G["mix.focal.loss" if ex is A.FocalLoss_Ori else "mix.ce.loss"], "EX", **LOSS_TOL)
    if au is A.DiceAULoss:   # (AULoss itself has no CPU path: test_cabi_cpu.py::test_no_cpu_fallback)
        assert_same_kind_close(m.get_au_loss(out, G["mix.y_au"]), G["mix.dice.loss"], "AU", **LOSS_TOL)


def test_plain_setting_keeps_its_losses():
    m = A.build_model("sformer", task="EX")
    out, y_ex, y_va = G["b64.out"], G["b64.y_ex"], G["b64.y_va"]
    assert torch.equal(m.get_ex_loss(out, y_ex), torch.nn.functional.cross_entropy(out[:, 12:19], y_ex, ignore_index=7))

    def ccc(p, t):  # biased variances, every row
        return 1 - 2 * ((p - p.mean()) * (t - t.mean())).mean() / (p.var(unbiased=False) + t.var(unbiased=False) + (p.mean() - t.mean()) ** 2 + 1e-8)
    want = 2 * ccc(torch.tanh(out[:, 19]), y_va[:, 0]) + ccc(torch.tanh(out[:, 20]), y_va[:, 1])
    torch.testing.assert_close(m.get_va_loss(out, y_va), want, rtol=1e-6, atol=1e-6)


def test_constructor_arguments_follow_the_reference():
    f = A.FocalLoss_Ori(7, alpha=[1, 2, 3, 4, 5, 6, 7], gamma=1.5, ignore_index=7)
    assert f.gamma == 1.5 and f.smooth == 1e-4 and f.alpha.tolist() == [1, 2, 3, 4, 5, 6, 7] and f.reduction == "mean"
    with pytest.raises(RuntimeError):
        A.FocalLoss_Ori(7, alpha=[1, 2])
    with pytest.raises(ValueError):
        A.FocalLoss_Ori(5)
    assert A.CCCLoss().ignore == -5.0 and A.DiceAULoss().ignore == -1
    assert A.DiceAULoss().pos_weight == (1, 2, 1, 1, 1, 1, 1, 6, 6, 5, 1, 5)
    with pytest.raises(TypeError):
        A.MultiTaskLoss(loss_EX=torch.nn.CrossEntropyLoss())


def test_entry_point_checks_its_layout_on_the_host():
    """struct layout of the binding, and every refusal that protects the kernel's bounds - all before a launch"""
    A._build.build()
    lib = A._lib.load()
    assert lib.avf_sizeof_task_loss_cfg() == ctypes.sizeof(A._lib.TaskLossCfg)
    mt = A.MultiTaskLoss()
    cfg = mt._cfg(False)
    assert (cfg.ex_col, cfg.au_col, cfg.va_col, cfg.va_ncols, cfg.va_tanh) == (12, 0, 19, 2, 1)
    assert list(cfg.pos_weight) == [1, 1, 1, 1, 1, 1, 1, 3, 3, 3, 1, 2] and cfg.ex_ignore == 7 and cfg.va_ignore == -5.0
    p = ctypes.c_void_p(4096)  # never dereferenced: each call below is refused first

    def call(c, width=21, ld=21, rows=4, ld_au=12, ld_va=2):
        return lib.avf_task_loss(p, ld, p, p, ld_au, p, ld_va, ctypes.byref(c), rows, width, p, p, p, None)
    assert call(cfg, width=20, ld=20) != 0 and b"column block" in lib.avf_last_error()      # VA block beyond the row
    assert call(cfg, ld=20) != 0 and call(cfg, rows=0) != 0 and call(cfg, ld_au=11) != 0 and call(cfg, ld_va=1) != 0
    import copy
    bad = copy.copy(cfg)
    bad.ex_col = 10                                                                       # overlaps the AU block
    assert call(bad) != 0 and b"overlaps" in lib.avf_last_error()
    bad = copy.copy(cfg)
    bad.va_ncols = 3
    assert call(bad) != 0
    bad = copy.copy(cfg)
    bad.ex_mode = 5
    assert call(bad) != 0
    assert lib.avf_task_loss_bwd(p, p, p, p, ctypes.byref(cfg), 4, 20, p, None) != 0
