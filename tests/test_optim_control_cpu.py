"""CPU (no GPU needed): the host side of FusedAdam's gradient clipping / warm-up / lr-scale control - constructor validation,
the three C-ABI symbols in the binding, the knobs in param_groups (state_dict round trip) and the pure-host size query."""
import ctypes as C

import pytest
import torch

import avformer_amd as A


def _model():
    return A.SyntheticAVFormer(16, 1, 1, 8, 16, 3, 2, compute_dtype="f32")


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("-inf"), float("nan")])
def test_constructor_rejects_bad_max_grad_norm(bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        A.optim.FusedAdam(_model(), lr=1e-3, max_grad_norm=bad)


@pytest.mark.parametrize("bad", [-1, -100, 2.5])
def test_constructor_rejects_bad_n_warmup_steps(bad):
    with pytest.raises(ValueError, match="n_warmup_steps"):
        A.optim.FusedAdam(_model(), lr=1e-3, n_warmup_steps=bad)


def test_constructor_accepts_the_knobs_and_state_dict_carries_them():
    m = _model()
    opt = A.optim.FusedAdam(m, lr=1e-3, max_grad_norm=2.5, n_warmup_steps=7)
    for grp in opt.param_groups:
        assert grp["max_grad_norm"] == 2.5 and grp["n_warmup_steps"] == 7 and grp["lr_scale"] == 1.0
    opt.set_lr_scale(0.1)
    sd = opt.state_dict()
    assert all(abs(g["lr_scale"] - 0.1) < 1e-9 and g["max_grad_norm"] == 2.5 and g["n_warmup_steps"] == 7
               for g in sd["param_groups"])
    other = A.optim.FusedAdam(m, lr=1e-3)
    assert other.param_groups[0]["max_grad_norm"] is None and other.param_groups[0]["n_warmup_steps"] == 0
    assert not other._scaled
    other.load_state_dict(sd)
    assert other.param_groups[0]["max_grad_norm"] == 2.5 and other.param_groups[0]["n_warmup_steps"] == 7
    assert other._scaled and abs(other._lr_scale - 0.1) < 1e-9
    with pytest.raises(ValueError):
        opt.set_lr_scale(torch.ones(2))


def test_signatures_hold_the_three_new_symbols():
    S = A._lib.SIGNATURES
    assert S["avf_grad_control_workspace_bytes"][0] is C.c_size_t and len(S["avf_grad_control_workspace_bytes"][1]) == 2
    assert S["avf_grad_control"][0] is C.c_int and len(S["avf_grad_control"][1]) == 9
    assert S["avf_adam_batch_control"][0] is C.c_int and len(S["avf_adam_batch_control"][1]) == 1


def test_workspace_bytes_is_one_double_per_4096_elements():
    A._build.build()
    lib = A._lib.load()
    numel = [1, 4096, 4097, 0, 12289]
    arr = (C.c_int64 * len(numel))(*numel)
    assert lib.avf_grad_control_workspace_bytes(len(numel), arr) == 8 * (1 + 1 + 2 + 0 + 4)
    assert lib.avf_grad_control_workspace_bytes(0, None) == 0
    # the session call outside a session is an error, not a silent no-op
    assert lib.avf_adam_batch_control(None) != 0
    assert b"no batch is open" in lib.avf_last_error()
