"""-m gpu: the bottom end of the fused stack on the all-bf16 streams (a pooled Linear head in the pooling launch was built with
them and left out: its backward ran longer than the two launches it replaced).

Part 1 - embed + LayerNorm-1 in one launch (ops.layernorm_fwd_embed, avf_layer_fwd_embed): x0, y, mean and rstd are bit-identical
to fuse_tokens(out_bf16=True) followed by the bf16 LayerNorm forward.

Part 2 - d pos_embedding straight from the bottom layer's token-major LayerNorm-1 backward (ops.layernorm_bwd_pos,
avf_layer_bwd_pos / avf_layer_bwd_dx_pos).  d_pos, dgamma and dbeta are fp32 sums taken in another order than on the row-major path
(fp32 dx -> column sum over the clips; 16-row partials -> fold); everything else in the step is bit-identical.

  Bound of the operator test (fixed by the change's issue): against an fp64 restatement of the LayerNorm backward computed from
  the SAME bf16 inputs and fp32 statistics, the token-major path's maximum absolute error is at most MARGIN = 2 times the
  row-major path's own maximum absolute error on those inputs (the margin is for the summation order).  The row-major
  path's arithmetic is the parent commit's (its kernels are untouched); its error is taken in the test, on the same inputs.
  Measured on an MI355X over the 22 cases below (maximum absolute error against fp64; the row-major figures were taken on the
  parent commit with the same inputs and are the same on this one):
                row-major (parent)        token-major          largest ratio token-major / row-major
    d_pos       4.5e-08 .. 9.6e-07        up to 1.06e-06       1.77  (B = 33, N = 9, D = 64: 1.058e-06 against 5.987e-07)
    dgamma      2.9e-08 .. 2.2e-06        up to 2.09e-06       1.51  (B = 5, N = 9, D = 512)
    dbeta       0 .. 4.8e-07              0 .. 4.8e-07         1.00  (sums of bf16 values: exact in 19 cases on both paths)
  The test prints both errors and the ratio of every case before it asserts.

  Bound of the stack test: d_pos and layer 0's LayerNorm-1 gradients of the two paths differ by a reordering of at most B
  (d_pos) / B * N (dgamma, dbeta) fp32 additions of the same addends, so each element differs by at most ~rows * 2^-24 of the sum
  of the magnitudes of its addends: with rows <= 297 that is 1.8e-5 of an element's absolute sum, and the relative Frobenius
  distance of a tensor is held to 1e-5 (cancellation inside an element makes single elements worse than the tensor).
"""
import os

import pytest
import torch

import avformer_amd as A
from avformer_amd import ops
from gpu_util import DEV

pytestmark = pytest.mark.gpu
MARGIN = 2.0


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- part 1
# (3, 5, 4, 520 / 1536): the two- and three-chunk instantiations of the kernel, the first with a partly filled last chunk
@pytest.mark.parametrize("B,Tv,Ta,D", [(B, Tv, Ta, D) for B in (1, 3) for Tv, Ta in ((5, 4), (1, 16)) for D in (64, 512)] +
                         [(3, 5, 4, 520), (3, 5, 4, 1536)])
def test_embed_ln_matches_the_two_launches_bitwise(B, Tv, Ta, D):
    """rows B * (Tv + Ta) in {9, 17, 27, 51}: none a multiple of the 16 rows of a workgroup, the larger ones more than one"""
    g = _gen(B * 1000 + Tv * 10 + D)
    clip = torch.randn(B, Tv, D, generator=g).to(DEV)
    audio = torch.randn(B, Ta, D, generator=g).to(DEV)
    table = (torch.randn(Tv + Ta + 3, D, generator=g) * 0.5).to(DEV)  # a table longer than the sequence: its first rows are used
    pos = table[:Tv + Ta]
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    b = (0.1 * torch.randn(D, generator=g)).to(DEV)
    x_ref = ops.fuse_tokens(clip, audio, pos, out_bf16=True)
    y_ref, mean_ref, rstd_ref = ops.layernorm_fwd_ex(x_ref.view(-1, D), w, b, 1e-5, torch.bfloat16)
    x0, y, mean, rstd = ops.layernorm_fwd_embed(clip, audio, pos, w, b, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(x0.view(torch.int16), x_ref.view(torch.int16))
    assert torch.equal(y.view(-1, D).view(torch.int16), y_ref.view(torch.int16))
    assert torch.equal(mean, mean_ref) and torch.equal(rstd, rstd_ref)


def _model(D, depth, Tv, Ta, table_extra=0, seed=7):
    torch.manual_seed(seed)
    heads, dh = (2, 32) if D == 64 else (8, 64)
    m = A.SyntheticAVFormer(D, depth, heads, dh, 2 * D, Tv, Ta, task="AU", compute_dtype="bf16", residual_dtype="bf16").to(DEV)
    if table_extra:
        m.pos_embedding = torch.nn.Parameter(torch.randn(1, Tv + Ta + table_extra, D, device=DEV) * 0.02)
    return m


def _batch(B, Tv, Ta, D, seed=11):
    g = _gen(seed)
    clip = torch.randn(B, Tv, D, generator=g).to(DEV)
    audio = torch.randn(B, Ta, D, generator=g).to(DEV)
    labels = (torch.rand(B, 12, generator=g) > 0.5).float().to(DEV)
    return {"clip": clip, "audio_features": audio}, labels


def _step(m, batch, labels):
    """one forward + loss + backward -> (logits, loss, {name: grad}, d_clip, d_audio)"""
    m.zero_grad(set_to_none=True)
    for t in batch.values():
        t.grad = None
    out = m(batch)
    loss = m.get_au_loss(out, labels)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return out.detach().clone(), loss.detach().clone(), grads, batch["clip"].grad, batch["audio_features"].grad


@pytest.mark.parametrize("Tv,Ta,fused", [(5, 4, True), (1, 16, True), (17, 0, False)])
def test_stack_forward_with_the_embed_path_is_bitwise_the_old_one(Tv, Ta, fused):
    """the whole forward of a depth-2 stack (logits and loss) with layer 0 on avf_layer_fwd_embed against fuse_tokens + avf_layer_fwd;
    an audio-less batch is not fused and takes the old launches either way; the positional table is longer than the sequence"""
    B, D = 3, 64
    m = _model(D, 2, Tv, Ta, table_extra=2)
    batch, labels = _batch(B, Tv, Ta, D)
    cfg = m.transformer._cfg(B, Tv + Ta, 0)
    import ctypes as C
    assert A._lib.load().avf_layer_fwd_embed_ok(C.byref(cfg)) == 1
    with torch.no_grad():
        with _env(AVF_STACK_ENDS=1):
            out_new = m(batch)
            loss_new = m.get_au_loss(out_new, labels)
        with _env(AVF_STACK_ENDS=0):
            out_old = m(batch)
            loss_old = m.get_au_loss(out_old, labels)
    torch.cuda.synchronize()
    assert torch.equal(out_new, out_old) and torch.equal(loss_new, loss_old)
    assert bool(torch.isfinite(out_new).all())


# ---------------------------------------------------------------------------------------------------------------- part 2
def _ln_bwd_inputs(B, N, D, seed):
    g = _gen(seed)
    rows = B * N
    x = torch.randn(rows, D, generator=g).to(DEV).bfloat16()
    dy = (torch.randn(rows, D, generator=g) * 0.3).to(DEV).bfloat16()
    dres = (torch.randn(rows, D, generator=g) * 0.3).to(DEV).bfloat16()
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    b = (0.1 * torch.randn(D, generator=g)).to(DEV)
    _, mean, rstd = ops.layernorm_fwd_ex(x, w, b, 1e-5, torch.bfloat16)
    return x, dy, dres, w, mean, rstd


def _ln_bwd_fp64(x, dy, dres, w, mean, rstd, B, N):
    """the LayerNorm backward restated in fp64 from the kernels' own inputs -> d_pos [N, D], dgamma, dbeta"""
    x, dy, dres, w = x.double().cpu(), dy.double().cpu(), dres.double().cpu(), w.double().cpu()
    mu, rs = mean.double().cpu()[:, None], rstd.double().cpu()[:, None]
    xh = (x - mu) * rs
    gg = dy * w
    dx = rs * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) + dres
    D = x.shape[1]
    return dx.view(B, N, D).sum(0), (dy * xh).sum(0), dy.sum(0)


# (5, 9, 520 / 1536): the two- and three-chunk instantiations (RU = 2 / 1 clips per batch), 1536 with more than 64 KiB of LDS
_LN_CASES = [(B, N, D) for B in (1, 3, 5, 17, 33) for N in (1, 9) for D in (64, 512)] + [(5, 9, 520), (5, 9, 1536)]


@pytest.mark.parametrize("B,N,D", _LN_CASES)
def test_token_major_ln_bwd_against_fp64(B, N, D):
    """B = 1, 3: fewer clips than one batch of RU = 4 per wave; 5, 17, 33: a ragged last batch; 17 (D = 64 ... 512: RU = 4) and 33:
    more than one pass of the four waves.  Canaries around d_pos; two runs bit-identical."""
    x, dy, dres, w, mean, rstd = _ln_bwd_inputs(B, N, D, B * 100 + N * 10 + D)
    assert A._lib.load().avf_layernorm_bwd_pos_ok(B, N, D) == 1
    ref_pos, ref_dg, ref_db = _ln_bwd_fp64(x, dy, dres, w, mean, rstd, B, N)
    # the row-major path, as the stack ran it: fp32 dx out of the LayerNorm backward, then the column sums over the clips
    dx, _, _, dg_old, db_old, _ = ops.layernorm_bwd_ex(dy, x, w, mean, rstd, dres, want_dx=True, want_lo=True)
    pos_old = ops.colsum(dx.view(B, N * D)).view(N, D)
    guard = 64
    buf = torch.full((N * D + 2 * guard,), -777.0, dtype=torch.float32, device=DEV)
    pos_new, dg_new, db_new = ops.layernorm_bwd_pos(dy, x, w, mean, rstd, dres, B, d_pos=buf[guard:guard + N * D].view(N, D))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -777.0).all()) and bool((buf[-guard:] == -777.0).all()), "write outside d_pos"
    pos_again, dg_again, db_again = ops.layernorm_bwd_pos(dy, x, w, mean, rstd, dres, B)
    assert torch.equal(pos_again, pos_new) and torch.equal(dg_again, dg_new) and torch.equal(db_again, db_new)
    for name, new, old, ref in (("d_pos", pos_new, pos_old, ref_pos), ("dgamma", dg_new, dg_old, ref_dg), ("dbeta", db_new, db_old, ref_db)):
        e_new = (new.double().cpu() - ref).abs().max().item()
        e_old = (old.double().cpu() - ref).abs().max().item()
        print(f"ln_bwd_pos B={B} N={N} D={D} {name}: max|err| token-major {e_new:.3e} row-major {e_old:.3e} ratio {e_new / max(e_old, 1e-300):.2f}")
        assert e_new <= MARGIN * e_old, (name, e_new, e_old)


_MOVES = ("pos_embedding", "transformer.layers.0.0.fn.norm.weight", "transformer.layers.0.0.fn.norm.bias")


def _compare_steps(new, old):
    out_n, loss_n, g_n, _, _ = new
    out_o, loss_o, g_o, _, _ = old
    assert torch.equal(out_n, out_o) and torch.equal(loss_n, loss_o)
    assert set(g_n) == set(g_o)
    for k in g_o:
        if k in _MOVES:
            d = ((g_n[k].double() - g_o[k].double()).norm() / (g_o[k].double().norm() + 1e-300)).item()
            print(f"{k}: relative Frobenius distance {d:.3e}")
            assert d <= 1e-5, (k, d)
        else:
            assert torch.equal(g_n[k], g_o[k]), k


# (32, 4, 64): 128 token rows, the smallest batch of this width at which the deferred weight-gradient launch engages
@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("B,N,D", [(B, N, D) for B in (1, 3, 5, 17, 33) for N in (1, 9) for D in (64, 512)] + [(32, 4, 64)])
def test_stack_step_with_d_pos_from_ln1_backward(B, N, D, defer):
    Tv = N // 2 + 1
    Ta = N - Tv
    m = _model(D, 2, Tv, Ta, table_extra=2)
    batch, labels = _batch(B, Tv, Ta, D)
    with _env(AVF_DW_DEFER=defer):
        if (B, N, D) == (32, 4, 64) and defer:
            import ctypes as C
            t = m.transformer
            assert t._dw_plan(A._lib.load(), [t._cfg(B, N, l) for l in range(2)]) == [2]
        with _env(AVF_STACK_ENDS=0):
            old = _step(m, batch, labels)
        with _env(AVF_STACK_ENDS=1):
            new = _step(m, batch, labels)
            again = _step(m, batch, labels)
    assert new[2]["pos_embedding"].shape == (1, N + 2, D)
    assert bool((new[2]["pos_embedding"][0, N:] == 0).all())  # the rows of the table past the sequence
    _compare_steps(new, old)
    for k in new[2]:
        assert torch.equal(new[2][k], again[2][k]), k  # run to run


def test_inputs_that_require_grad_keep_the_old_path():
    B, Tv, Ta, D = 3, 5, 4, 64
    m = _model(D, 2, Tv, Ta)
    batch, labels = _batch(B, Tv, Ta, D)
    batch["clip"].requires_grad_(True)
    batch["audio_features"].requires_grad_(True)
    with _env(AVF_STACK_ENDS=0):
        old = _step(m, batch, labels)
    with _env(AVF_STACK_ENDS=1):
        new = _step(m, batch, labels)
    assert new[3] is not None and new[4] is not None
    assert torch.equal(new[3], old[3]) and torch.equal(new[4], old[4])
    for k in old[2]:
        assert torch.equal(new[2][k], old[2][k]), k  # d_pos too: the column sums of the same fp32 dx
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])


# ------------------------------------------------------------------------------------------------------- one captured step
@pytest.mark.parametrize("ends", [0, 1])
def test_captured_step_equals_the_eager_step(ends):
    B, Tv, Ta, D = 4, 5, 4, 64
    m = _model(D, 2, Tv, Ta)
    batch, labels = _batch(B, Tv, Ta, D)
    with _env(AVF_STACK_ENDS=ends):
        eager = _step(m, batch, labels)

        def step():
            m.zero_grad(set_to_none=True)
            out = m(batch)
            loss = m.get_au_loss(out, labels)
            loss.backward()
            return out.detach(), loss.detach()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out_s, loss_s = step()
        for _ in range(2):
            for p in m.parameters():
                p.grad.fill_(float("nan"))  # a replay has to rewrite every gradient
            out_s.fill_(float("nan"))
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(out_s, eager[0]) and torch.equal(loss_s, eager[1])
            for k, p in m.named_parameters():
                assert torch.equal(p.grad, eager[2][k]), k

