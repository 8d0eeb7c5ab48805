"""CPU (no GPU needed): dim_head 128 is a configuration the layer accepts in every compute mode (bf16, mx8 forward, bf16
residual stream, f32), while head widths outside {32, 64, 128} stay rejected on the bf16 path with "dim_head" in the error;
and the CPU oracle matches the reference's Transformer at dim_head 128 (fixture G16)."""
import ctypes

import pytest
import torch

import avformer_amd as A
import oracle
from conftest import load_golden, split_golden


@pytest.fixture(scope="module")
def lib():
    A._build.build()
    return A._lib.load()


def _cfg(dim_head, dtype, heads=4, dim=512, mx8=False, resid16=False):
    c = A._lib.LayerCfg(8, 197, dim, heads, dim_head, 1024, dtype, 1, 1e-5, 0.0)
    c.mx8_fwd = 1 if mx8 else 0
    c.resid_bf16 = 1 if resid16 else 0
    return c


@pytest.mark.parametrize("mode", ["bf16", "mx8", "resid_bf16", "f32"])
def test_dim_head_128_sizes(lib, mode):
    dtype = A._lib.F32 if mode == "f32" else A._lib.BF16
    cfg = _cfg(128, dtype, mx8=mode == "mx8", resid16=mode == "resid_bf16")
    assert lib.avf_layer_saved_bytes(ctypes.byref(cfg)) > 0, lib.avf_last_error()
    assert lib.avf_layer_workspace_bytes(ctypes.byref(cfg)) > 0, lib.avf_last_error()
    if dtype == A._lib.BF16:
        assert lib.avf_layer_lowp_bytes(ctypes.byref(cfg)) > 0, lib.avf_last_error()
    else:
        assert lib.avf_layer_lowp_bytes(ctypes.byref(cfg)) == 0


def test_identity_to_out_dim_head_128_bf16(lib):
    cfg = A._lib.LayerCfg(2, 50, 128, 1, 128, 256, A._lib.BF16, 0, 1e-5, 0.0)  # heads == 1, dim_head == dim: nn.Identity
    assert lib.avf_layer_saved_bytes(ctypes.byref(cfg)) > 0, lib.avf_last_error()


@pytest.mark.parametrize("dim_head", [48, 96, 256])
def test_unsupported_dim_head_rejected_bf16(lib, dim_head):
    cfg = _cfg(dim_head, A._lib.BF16, heads=2)
    assert lib.avf_layer_saved_bytes(ctypes.byref(cfg)) == 0
    assert b"dim_head" in lib.avf_last_error()


def test_oracle_vs_reference_golden_dh128():
    """oracle.transformer_forward vs the reference's Transformer(64, 2, 2, 128, 128): y, dx and every weight gradient"""
    p, g, r = split_golden({**load_golden("g16_transformer_dh128"), **load_golden("g16_transformer_dh128_grads")})
    assert r["dim_head"] == 128
    x = r["x"].clone().requires_grad_(True)
    ps = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    y = oracle.transformer_forward(x, ps, r["depth"], r["heads"])
    y.pow(2).mean().backward()
    # the tolerances of test_oracle_golden.py
    torch.testing.assert_close(y.detach(), r["y"], atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(x.grad, r["dx"], atol=2e-5, rtol=1e-4)
    assert set(g) == set(p)
    for k in p:
        torch.testing.assert_close(ps[k].grad, g[k], atol=2e-5, rtol=1e-4, msg=k)
