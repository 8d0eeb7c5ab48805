"""-m gpu: dim_head 128 in every compute mode, forward and backward.

The attention core at dim_head 128: the bf16 streaming MFMA kernels (eight waves of 16 rows per workgroup), the fp32 matrix-pipe
kernels of the parity mode (in both of its arithmetics: the three-product bf16x3 attention is dim_head-64-only, so dim_head
128 runs on the f32-input MFMA kernels there too) and the fp32-arithmetic kernels of the masked calls (two lanes per row).
Then whole stacks in every mode against the reference fixture G16 (tests/golden/make_golden_dh128.py) and the CPU oracle,
dropout replay, determinism and graph capture."""
import math

import pytest
import torch

import oracle
from conftest import load_golden, split_golden
from gpu_util import (DEV, check_abs, check_rel, f32_arithmetic, hip_transformer_run, make_hip_transformer, max_abs,
                      oracle_transformer_run, rel_fro)

pytestmark = pytest.mark.gpu

SQ = lambda y: y.pow(2).mean()
DH = 128


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    A._lib.load()
    return A.ops


@pytest.fixture(params=["bf16x3", "f32"])
def f32_arith(request):
    with f32_arithmetic(request.param) as mode:
        yield mode


def _close(a, b, atol=2e-5, rtol=1e-4):
    torch.testing.assert_close(a.detach().float().cpu(), b.detach().float().cpu(), atol=atol, rtol=rtol)


# ---------------------------------------------------------------------------------------------- attention core
def _attn_ref(qkv, B, N, H, dh, d_o=None):
    """fp64 restatement of heads.py:222-237 on the packed projection."""
    I = H * dh
    qkv = qkv.double().clone().requires_grad_(True)
    q, k, v = qkv.view(B, N, 3 * I).split(I, dim=-1)
    sh = lambda t: t.reshape(B, N, H, dh).permute(0, 2, 1, 3)
    q, k, v = sh(q), sh(k), sh(v)
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    p = s.softmax(-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * N, I)
    lse2 = torch.logsumexp(s, dim=-1) * math.log2(math.e)
    dqkv = None
    if d_o is not None:
        o.backward(d_o.double())
        dqkv = qkv.grad
    return o.detach(), lse2.detach(), dqkv


def _prescale_q(qkv, H, dh):
    """bf16 projection with q' = bf16(q * log2(e)/sqrt(dh)) in the q columns, and the fp32 projection it stands for:
    (q'/c | k | v) exactly, so that the reference sees the very numbers the kernels see"""
    c = math.log2(math.e) / math.sqrt(dh)
    I = H * dh
    dev = qkv.float().clone()
    dev[:, :I] = (dev[:, :I] * c).to(torch.bfloat16).float()
    ref = dev.clone()
    ref[:, :I] = ref[:, :I] / c
    return dev.to(torch.bfloat16), ref


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 324, 513, 1024, 1031])
@pytest.mark.parametrize("B,H", [(2, 2), (1, 5)])
@pytest.mark.parametrize("qs", [False, True], ids=["raw_q", "prescaled_q"])
def test_attention_bf16_dh128(ops, N, B, H, qs):
    g = torch.Generator().manual_seed(12800 + N + 10 * H)
    qkv = torch.randn(B * N, 3 * H * DH, generator=g).to(torch.bfloat16)
    d_o = torch.randn(B * N, H * DH, generator=g).to(torch.bfloat16)
    ref_in = qkv.float()
    if qs:
        qkv, ref_in = _prescale_q(qkv, H, DH)
    o_ref, lse_ref, dqkv_ref = _attn_ref(ref_in, B, N, H, DH, d_o.float())
    o, lse2 = ops.attn_fwd(qkv.cuda(), B, N, H, DH, q_prescaled=qs)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse2).all()
    tag = f"attn_dh128[{B}x{N}x{H},qs{int(qs)}]"
    check_rel(tag + ":o", o, o_ref, 1e-2)
    _close(lse2, lse_ref.float(), atol=2e-2, rtol=1e-3)
    dqkv = ops.attn_bwd(qkv.cuda(), o, d_o.cuda(), lse2, B, N, H, DH, q_prescaled=qs)
    assert torch.isfinite(dqkv.float()).all()
    I = H * DH
    for name, sl in (("dq", slice(0, I)), ("dk", slice(I, 2 * I)), ("dv", slice(2 * I, 3 * I))):
        if N == 1 and name != "dv":  # a single key: p = 1, dS = 0 exactly -> dq = dk = 0 (no relative error to take)
            assert max_abs(dqkv[:, sl], dqkv_ref[:, sl]) < 1e-2
            continue
        check_rel(f"{tag}:{name}", dqkv[:, sl], dqkv_ref[:, sl], 2e-2)


@pytest.mark.parametrize("B,N,H", [(2, 7, 2), (1, 130, 3), (2, 324, 2)])
def test_attention_f32_dh128(ops, f32_arith, B, N, H):
    g = torch.Generator().manual_seed(B * 100 + N + DH)
    qkv = torch.randn(B * N, 3 * H * DH, generator=g)
    d_o = torch.randn(B * N, H * DH, generator=g)
    o_ref, lse_ref, dqkv_ref = _attn_ref(qkv, B, N, H, DH, d_o)
    o, lse2 = ops.attn_fwd(qkv.cuda(), B, N, H, DH)
    _close(o, o_ref.float())
    _close(lse2, lse_ref.float(), atol=1e-4)
    dqkv = ops.attn_bwd(qkv.cuda(), o, d_o.cuda(), lse2, B, N, H, DH)
    _close(dqkv, dqkv_ref.float(), atol=5e-5, rtol=1e-4)


@pytest.mark.parametrize("B,N,H", [(3, 40, 2), (2, 100, 1), (2, 65, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_masked_attention_core_dh128_vs_fp64(ops, B, N, H, dtype):
    g = torch.Generator().manual_seed(B * 100 + N)
    I = H * DH
    qkv = torch.randn(B * N, 3 * I, generator=g).to(dtype)
    d_o = torch.randn(B * N, I, generator=g).to(dtype)
    keep = torch.rand(B, N, generator=g) > 0.3
    keep[:, 0] = True
    keep[-1, 1:] = False  # one clip with every other token dropped
    o, lse2 = ops.attn_fwd_masked(qkv.to(DEV), keep.to(DEV), B, N, H, DH)
    dqkv = ops.attn_bwd_masked(qkv.to(DEV), o, d_o.to(DEV), lse2, keep.to(DEV), B, N, H, DH)
    # fp64 restatement with the -FLT_MAX fill of heads.py:225-232 on the same (storage-rounded) inputs
    x = qkv.double().requires_grad_(True)
    q, k, v = [t.reshape(B, N, H, DH).permute(0, 2, 1, 3) for t in x.split(I, dim=-1)]
    s = (q @ k.transpose(-1, -2)) * DH ** -0.5
    pair = keep[:, None, :, None] & keep[:, None, None, :]
    s = s.masked_fill(~pair, -torch.finfo(torch.float32).max)
    ref = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * N, I)
    ref.backward(d_o.double())
    tol = 1e-5 if dtype == torch.float32 else 1.2e-2
    tag = f"mask_attn_dh128[{B}x{N}x{H},{dtype}]"
    check_rel(tag + ":o", o, ref.detach().float(), tol)
    check_rel(tag + ":dqkv", dqkv, x.grad.float(), tol * 2)
    dq = dqkv.float().view(B, N, 3, H, DH)[:, :, 0]
    dk = dqkv.float().view(B, N, 3, H, DH)[:, :, 1]
    assert torch.all(dq[~keep.to(DEV)] == 0) and torch.all(dk[~keep.to(DEV)] == 0)


# ---------------------------------------------------------------------------------------------- stacks
def _state(D, L, H, M, seed):
    g = torch.Generator().manual_seed(seed)
    sd = oracle.init_transformer_state(D, L, H, DH, M, generator=g)
    for k in sd:  # non-trivial LayerNorm affine so dgamma/dbeta paths are exercised
        if k.endswith("norm.weight"):
            sd[k] = 1 + 0.1 * torch.randn(D, generator=g)
        if k.endswith("norm.bias"):
            sd[k] = 0.1 * torch.randn(D, generator=g)
    return sd, g


def _g16():
    return split_golden({**load_golden("g16_transformer_dh128"), **load_golden("g16_transformer_dh128_grads")})


def test_g16_f32_vs_reference_golden():
    p, g, r = _g16()
    t = make_hip_transformer(p, r["dim"], r["depth"], r["heads"], r["dim_head"], r["mlp_dim"], "f32")
    y, dx, grads = hip_transformer_run(t, r["x"], SQ)
    _close(y, r["y"], atol=5e-5, rtol=1e-3)
    _close(dx, r["dx"], atol=1e-6, rtol=1e-3)
    for k, v in g.items():
        _close(grads[k], v, atol=2e-6, rtol=2e-3)


def test_g16_bf16_vs_reference_golden():
    p, g, r = _g16()
    t = make_hip_transformer(p, r["dim"], r["depth"], r["heads"], r["dim_head"], r["mlp_dim"], "bf16")
    y, dx, grads = hip_transformer_run(t, r["x"], SQ)
    check_rel("golden_bf16[g16]:y", y, r["y"], 1.5e-2)
    check_rel("golden_bf16[g16]:dx", dx, r["dx"], 3e-2)
    for k, v in g.items():
        check_rel(f"golden_bf16[g16]:g.{k}", grads[k], v, 4e-2)


STACKS = {"d256_h2": (3, 77, 256, 2, 2, 512), "d768_h6": (2, 200, 768, 2, 6, 1536)}  # (B, N, D, L, H, M)


@pytest.mark.parametrize("cfg", list(STACKS))
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_transformer_dh128_vs_oracle(cfg, mode):
    B, N, D, L, H, M = STACKS[cfg]
    sd, g = _state(D, L, H, M, 123)
    x = torch.randn(B, N, D, generator=g)
    y_ref, dx_ref, g_ref = oracle_transformer_run(x, sd, L, H, SQ)
    t = make_hip_transformer(sd, D, L, H, DH, M, mode)
    y, dx, grads = hip_transformer_run(t, x, SQ)
    if mode == "f32":
        _close(y, y_ref, atol=5e-5, rtol=1e-3)
        _close(dx, dx_ref, atol=1e-6, rtol=1e-3)
        for k, v in g_ref.items():
            _close(grads[k], v, atol=3e-6, rtol=3e-3)
    else:
        tag = f"vs_oracle_dh128[{cfg}]"
        check_rel(tag + ":y", y, y_ref, 1.5e-2)
        check_rel(tag + ":dx", dx, dx_ref, 3e-2)
        for k, v in g_ref.items():
            check_rel(f"{tag}:g.{k}", grads[k], v, 4e-2)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_masked_stack_dh128_vs_oracle(mode):
    import avformer_amd as A
    B, N, D, H, M = 3, 40, 256, 2, 512
    sd, g = _state(D, 2, H, M, 77)
    x = torch.randn(B, N, D, generator=g)
    mask = torch.rand(B, N - 1, generator=g) > 0.3  # the reference's mask: one entry per token after the first
    mask[-1, 1:] = False
    mask[0] = True
    t = A.Transformer(D, 2, H, DH, M, compute_dtype=mode)
    t.load_state_dict(sd)
    t = t.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = t(xg, mask=mask.to(DEV))
    SQ(y).backward()
    xc = x.clone().requires_grad_(True)
    ps = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yc = oracle.transformer_forward(xc, ps, 2, H, mask=mask)
    SQ(yc).backward()
    grads = dict(t.named_parameters())
    if mode == "f32":
        _close(y, yc, atol=5e-5, rtol=1e-3)
        _close(xg.grad, xc.grad, atol=1e-6, rtol=1e-3)
        for k, p in ps.items():
            _close(grads[k].grad, p.grad, atol=2e-6, rtol=2e-3)
    else:
        tag = "mask_stack_dh128"
        check_rel(tag + ":y", y, yc.detach(), 1.5e-2)
        check_rel(tag + ":dx", xg.grad, xc.grad, 3e-2)
        for k, p in ps.items():
            check_rel(f"{tag}:g.{k}", grads[k].grad, p.grad, 4e-2)
    assert rel_fro(yc.detach(), oracle.transformer_forward(x, sd, 2, H)) > 1e-3  # the mask matters


def test_north_star_model_dh128():
    """the synthetic AV model at dim 512, 6 layers of 4 heads x 128, 196 + 128 tokens, B = 2: parity-mode logits and loss
    at the north-star tolerance, throughput-mode at the caps test_c3_c4_model_logits_and_loss_vs_oracle states"""
    import avformer_amd as A
    Tv, Ta, D, L, H, M, B = 196, 128, 512, 6, 4, 1024, 2
    torch.manual_seed(123)
    m32 = A.SyntheticAVFormer(D, L, H, DH, M, Tv, Ta, compute_dtype="f32").to(DEV)
    m16 = A.SyntheticAVFormer(D, L, H, DH, M, Tv, Ta, compute_dtype="bf16").to(DEV)
    m16.load_state_dict(m32.state_dict())
    g = torch.Generator().manual_seed(125)
    clip = torch.randn(B, Tv, D, generator=g)
    aud = torch.randn(B, Ta, D, generator=g)
    labels = (torch.rand(B, 12, generator=g) > 0.5).float()
    sd = {k: v.detach().cpu() for k, v in m32.state_dict().items()}
    tok = torch.cat([clip, aud], 1) + sd["pos_embedding"]
    tsd = {k[len("transformer."):]: v for k, v in sd.items() if k.startswith("transformer.")}
    logits_ref = oracle.transformer_forward(tok, tsd, L, H).mean(1) @ sd["au_fc.weight"].t() + sd["au_fc.bias"]
    loss_ref = oracle.au_loss(logits_ref, labels)
    batch = {"clip": clip.to(DEV), "audio_features": aud.to(DEV)}
    with torch.no_grad():
        out32, out16 = m32(batch), m16(batch)
        l32, l16 = m32.get_au_loss(out32, labels.to(DEV)), m16.get_au_loss(out16, labels.to(DEV))
    torch.testing.assert_close(out32[:, :12].cpu(), logits_ref, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(l32.cpu(), loss_ref, rtol=1e-4, atol=1e-5)
    check_abs("model_dh128:logits_maxabs", out16[:, :12], logits_ref, 2e-2)
    check_abs("model_dh128:loss", l16, loss_ref, 5e-3, floor=3e-4)


def test_mx8_dh128_vs_bf16():
    B, N, D, L, H, M = 4, 324, 512, 2, 4, 1024
    sd, g = _state(D, L, H, M, 88)
    x = torch.randn(B, N, D, generator=g)
    y16, dx16, g16 = hip_transformer_run(make_hip_transformer(sd, D, L, H, DH, M, "bf16"), x, SQ)
    y, dx, grads = hip_transformer_run(make_hip_transformer(sd, D, L, H, DH, M, "mx8"), x, SQ)
    check_rel("mx8_vs_bf16_dh128:y", y, y16, 5e-2)
    check_rel("mx8_vs_bf16_dh128:dx", dx, dx16, 1e-1)
    for k in g16:
        check_rel(f"mx8_vs_bf16_dh128:g.{k}", grads[k], g16[k], 1.5e-1)


def test_resid16_dh128_vs_oracle():
    import avformer_amd as A
    B, N, D, L, H, M = 2, 324, 512, 2, 4, 1024
    sd, g = _state(D, L, H, M, 321)
    x = torch.randn(B, N, D, generator=g)
    y_ref, dx_ref, g_ref = oracle_transformer_run(x, sd, L, H, SQ)
    t = A.Transformer(D, L, H, DH, M, 0.0, compute_dtype="bf16", residual_dtype="bf16")
    t.load_state_dict(sd, strict=True)
    y, dx, grads = hip_transformer_run(t.to(DEV), x, SQ)
    check_rel("rs16_dh128:y", y, y_ref, 3e-2)
    check_rel("rs16_dh128:dx", dx, dx_ref, 5e-2)
    for k, v in g_ref.items():
        check_rel(f"rs16_dh128:g.{k}", grads[k], v, 6e-2)


def test_identity_to_out_dh128_bf16_vs_f32():
    """heads == 1 and dim_head == dim == 128: to_out is nn.Identity (heads.py:207)"""
    B, N, D, L, H, M = 3, 50, 128, 2, 1, 256
    g = torch.Generator().manual_seed(1400)
    sd = oracle.init_transformer_state(D, L, H, DH, M, generator=g)
    assert not any("to_out" in k for k in sd)
    x = torch.randn(B, N, D, generator=g)
    y32, dx32, g32 = hip_transformer_run(make_hip_transformer(sd, D, L, H, DH, M, "f32"), x, SQ)
    y, dx, grads = hip_transformer_run(make_hip_transformer(sd, D, L, H, DH, M, "bf16"), x, SQ)
    check_rel("identity_dh128:y", y, y32, 1.5e-2)
    check_rel("identity_dh128:dx", dx, dx32, 3e-2)
    for k in g32:
        check_rel(f"identity_dh128:g.{k}", grads[k], g32[k], 4e-2)


# ---------------------------------------------------------------------------------------------- dropout, determinism, capture
def _dropout_run(t, x):
    xg = x.to(DEV).requires_grad_(True)
    for p in t.parameters():
        p.grad = None
    y = t(xg)
    SQ(y).backward()
    torch.cuda.synchronize()
    return y.detach().clone(), xg.grad.clone(), {k: p.grad.clone() for k, p in t.named_parameters()}, t.last_seed


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_dropout_replay_dh128(mode):
    import avformer_amd as A
    B, N, D, L, H, M, p = 3, 77, 256, 2, 2, 512, 0.2
    g = torch.Generator().manual_seed(5)
    sd = oracle.init_transformer_state(D, L, H, DH, M, generator=g)
    x = torch.randn(B, N, D, generator=g)
    mk = lambda: A.Transformer(D, L, H, DH, M, dropout=p, compute_dtype=mode)
    t, t2 = mk(), mk()
    t2._seed_salt = t._seed_salt  # the same dropout seed stream in both modules
    t.load_state_dict(sd)
    t2.load_state_dict(sd)
    t, t2 = t.to(DEV).train(), t2.to(DEV).train()
    y, dx, grads, seed = _dropout_run(t, x)
    assert seed != 0
    R = B * N
    drop = [tuple(A.ops.dropout_factors(seed, l, s, p, R, cols).cpu().view(B, N, cols)
                  for s, cols in ((0, D), (1, M), (2, D))) for l in range(L)]
    xr = x.clone().requires_grad_(True)
    pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yr = oracle.transformer_forward(xr, pr, L, H, drop=drop)
    SQ(yr).backward()
    if mode == "f32":
        _close(y, yr, atol=5e-5, rtol=1e-3)
        _close(dx, xr.grad, atol=1e-6, rtol=2e-3)
        for k in grads:
            _close(grads[k], pr[k].grad, atol=2e-6, rtol=2e-3)
    else:
        tag = "dropout_replay_dh128"
        check_rel(tag + ":y", y, yr, 1.5e-2)
        check_rel(tag + ":dx", dx, xr.grad, 3e-2)
        for k in grads:
            check_rel(f"{tag}:g.{k}", grads[k], pr[k].grad, 4e-2)
    assert rel_fro(yr, oracle.transformer_forward(x, sd, L, H)) > 0.1  # the masks really changed the result
    # the same seed -> bitwise the same output and gradients
    y2, dx2, grads2, seed2 = _dropout_run(t2, x)
    assert seed2 == seed
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_backward_deterministic_dh128(mode):
    B, N, D, L, H, M = 2, 200, 256, 2, 2, 512
    sd, g = _state(D, L, H, M, 9)
    x = torch.randn(B, N, D, generator=g)
    t = make_hip_transformer(sd, D, L, H, DH, M, mode)
    y1, dx1, g1 = hip_transformer_run(t, x, SQ)  # (the next run sets fresh .grad tensors: these stay as they are)
    y2, dx2, g2 = hip_transformer_run(t, x, SQ)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_graph_replay_dh128():
    """one captured training step (SyntheticAVFormer with 2 heads x 128 + AULoss + the library Adam) equals the eager step"""
    import avformer_amd as A
    torch.manual_seed(1)
    mk = lambda: A.SyntheticAVFormer(256, 2, 2, DH, 512, 24, 16, task="AU", compute_dtype="bf16").cuda()
    m_g = mk()
    m_e = mk()
    m_e.load_state_dict(m_g.state_dict())
    opt_g = A.optim.FusedAdam(m_g, lr=1e-3)
    opt_e = A.optim.FusedAdam(m_e, lr=1e-3)

    def loss(m, b):
        return m.get_au_loss(m({"clip": b["clip"], "audio_features": b["audio_features"]}), b["labels"])

    def batch(seed, B=6):
        g = torch.Generator().manual_seed(seed)
        return {"clip": torch.randn(B, 24, 256, generator=g).cuda(), "audio_features": torch.randn(B, 16, 256, generator=g).cuda(),
                "labels": (torch.rand(B, 12, generator=g) > 0.5).float().cuda()}

    gs = A.graphs.GraphedTrainStep(m_g, opt_g, loss, batch(1), warmup=2)
    for _ in range(2):
        opt_e.zero_grad(set_to_none=True)
        loss(m_e, batch(1)).backward()
        opt_e.step()
    b = batch(20)
    lg = gs(b).clone()
    opt_e.zero_grad(set_to_none=True)
    le = loss(m_e, b)
    le.backward()
    opt_e.step()
    torch.cuda.synchronize()
    assert torch.equal(lg, le.detach()), (lg.item(), le.item())
    for (n, p), (_, q) in zip(m_g.named_parameters(), m_e.named_parameters()):
        assert torch.equal(p, q), n
