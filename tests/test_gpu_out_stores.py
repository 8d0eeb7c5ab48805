"""-m gpu: the output stores of the hot path at their tile edges (csrc/common.hpp store_out16 / store_out8 / store_out4: the
write-through form under AVF_OUT_WT=1, the plain one under 0).  A hand-written store can go wrong in its predicate and in its
address, so every operator case here puts each output inside a larger byte buffer filled with a canary (0xA5), asserts that
every byte outside the logical output still holds it, and holds the output itself to the fp64 restatement the operator's own
test file uses (tests/gemm_nt_util.py, tests/layernorm_util.py, tests/mask_attn_util.py) at that file's tolerances.  Which store
form a GEMM case reaches depends on the tile the launcher picks, so every tiled case asserts the launcher's own plan.

  tiled NT GEMM       M = 97 / 191, N = 128 / 384, K = 64 / 512, the four epilogues, ldc = N + 8: at most six tiles, so all of
                      them run tile 6 (32 x 64, NI = 1) - the general nt_epilogue with its 8-byte stores (store_out8)
  ... the lean tiles  (2100, 256, 128) on tile 5 (96 x 128: what the bench step's 30 tiled launches run) and (4000, 2048, 64) on
                      tile 2 (128 x 128), both with a ragged last row tile and N % 128 == 0: nt_epilogue_lean's 16-byte
                      store_out16 (LEAN 1, and 2 with the column sums of dGELU), ldc = N + 8
  persistent GEMM     M = 2048 + 5 / 2048 + 37 (ragged last 32-row tile), N = 512 / 1536, K = 512, the four epilogues
  LayerNorm row8      rows = 33 / 8192 + 3 (both rows-per-workgroup regimes), D = 512, forward and backward with column sums
  resident attention  forward and merged backward at N = 17 / 324 / 512, B * H = 3
  deferred dW         one avf_layers_dw call of two layers at B = 8, N = 64 against the per-layer path
  Adam                one table with a layer whose W2 is 512 x 1536 and a loose 7-element vector, one step against
                      torch.optim.Adam; W2's three bf16 images (row-major, transposed, fragment-major) against their definitions
  replay              a 2-layer B = 2, N = 64 step captured and replayed three times against the eager step, bit for bit
                      (128 token rows: tile 6 of the NT kernel, row8 LayerNorm, head-resident attention; not the lean tiles
                      and not the persistent kernel, which starts at 2048 rows)

Outputs the Python layer allocates itself (column sums, the fp32 dx of the LayerNorm backward, parameter gradients, the
optimizer's state and weight images) are held to their reference only."""
import ctypes as C

import pytest
import torch

import gemm_nt_util as G
import layernorm_util as L
import mask_attn_util as MA
from gpu_util import DEV, check, rel_fro

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
CANARY = 0xA5
PAD = 512  # canary bytes in front of and behind every output


@pytest.fixture(scope="module")
def A():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A


class Guarded:
    """a [rows, cols] output of leading dimension ld >= cols inside a canary-filled byte buffer"""

    def __init__(self, rows, cols, dtype, ld=None):
        self.rows, self.cols, self.dtype, self.ld = rows, cols, dtype, ld or cols
        self.nbytes = rows * self.ld * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((PAD + self.nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)
        self.view = self._carve(self.raw)

    def _carve(self, raw):
        return raw[PAD:PAD + self.nbytes].view(self.dtype).view(self.rows, self.ld)[:, :self.cols]

    def intact(self, what):
        """every byte outside the logical output still holds the canary"""
        c = self.raw.clone()
        self._carve(c).copy_(torch.full((self.dtype.itemsize,), CANARY, dtype=torch.uint8, device=DEV).view(self.dtype))
        bad = (c != CANARY).nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} bytes outside the output were written, the first at offset {int(bad[0]) - PAD}"


# ------------------------------------------------------------------------------------------------ NT GEMMs
EPIS = (G.EPI_NONE, G.EPI_BIAS_RES, G.EPI_BIAS_GELU, G.EPI_DGELU)
_prod = {}


def _gemm_case(M, N, K):
    """operands and fp64 products of a shape, once (shared by the four epilogues; never modified)"""
    if (M, N, K) not in _prod:
        _prod.clear()
        a, w = G.make_operands(M, N, K, M * 7919 + N * 31 + K, "normal")
        _prod[(M, N, K)] = (a, w, G.products(dict(a=a, w=w)), a.to(DEV), w.to(DEV))
    return _prod[(M, N, K)]


def _dev(t):
    return None if t is None else t.to(DEV)


def _tiled(A, M, N, K, tile, lean_tile):
    """the four epilogues of one shape on the tiled kernel; the launcher's plan must name `tile` and, on a lean tile, LEAN 1
    (2 with the column sums of dGELU), else the general epilogue"""
    a, w, prod, a_dev, w_dev = _gemm_case(M, N, K)
    for epi in EPIS:
        what = f"tiled[{M}x{N}x{K}]/{G.EPI_NAMES[epi]}"
        inp = G.make_inputs(M, N, K, M + N + K, "normal", BF, epi, operands=(a, w))
        ref = G.reference(inp, None, prod)
        c_g = Guarded(M, N, BF, ld=N + 8)
        u_g = Guarded(M, N, BF, ld=N + 8) if epi == G.EPI_BIAS_GELU else None
        c, aux, cs, plan = A.ops.gemm_nt_ex(a_dev, w_dev, out=c_g.view, epilogue=epi, bias=_dev(inp["bias"]), residual=_dev(inp["res"]),
                                            aux=u_g.view if u_g is not None else _dev(inp["aux_in"]), want_colsum=epi == G.EPI_DGELU)
        torch.cuda.synchronize()
        c_g.intact(what + ":C")
        if u_g is not None:
            u_g.intact(what + ":u")
        lean = (2 if epi == G.EPI_DGELU else 1) if lean_tile else 0
        assert plan["kind"] == 1 and plan["tile"] == tile and plan["lean"] == lean, (what, plan)
        stats = G.check_outputs(what, ref, c.cpu(), aux.cpu() if epi == G.EPI_BIAS_GELU else None, None if cs is None else cs.cpu())
        print(what, plan, stats)


@pytest.mark.parametrize("M", [97, 191])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [64, 512])
def test_tiled_nt_gemm(A, M, N, K):
    _tiled(A, M, N, K, tile=6, lean_tile=False)


@pytest.mark.parametrize("M,N,K,tile", [(2100, 256, 128, 5), (4000, 2048, 64, 2)])
def test_tiled_nt_gemm_lean_tiles(A, M, N, K, tile):
    _tiled(A, M, N, K, tile=tile, lean_tile=True)


@pytest.mark.parametrize("M", [2048 + 5, 2048 + 37])
@pytest.mark.parametrize("N", [512, 1536])
def test_persistent_gemm(A, M, N):
    K = 512
    ops, lib = A.ops, A._lib.load()
    a, w, prod, a_dev, w_dev = _gemm_case(M, N, K)
    wp = ops.pack_ws(w_dev)
    for epi in EPIS:
        what = f"persistent[{M}x{N}]/{G.EPI_NAMES[epi]}"
        inp = G.make_inputs(M, N, K, M + N + K, "normal", BF, epi, operands=(a, w))
        if epi == G.EPI_NONE:
            inp["bias"] = None  # (the persistent kernel's plain form is compiled without the bias add)
        ref = G.reference(inp, None, prod)
        c_g = Guarded(M, N, BF, ld=N + 8)
        u_g = Guarded(M, N, BF, ld=N + 8) if epi == G.EPI_BIAS_GELU else None
        bias, res, aux_in = _dev(inp["bias"]), _dev(inp["res"]), _dev(inp["aux_in"])
        colsum = epi == G.EPI_DGELU
        cs_g = Guarded(1, N, F32) if colsum else None
        ws = torch.empty(lib.avf_gemm_nt_ws_workspace_bytes(M, N), dtype=torch.uint8, device=DEV) if colsum else None
        aux = u_g.view if u_g is not None else aux_in
        A._lib.check(lib.avf_gemm_nt_ws(M, N, K, ops._ptr(a_dev), K, ops._ptr(wp), ops._ptr(c_g.view), N + 8, ops.avf_dtype(BF), epi,
                                        ops._ptr(bias), ops._ptr(res), N, ops._ptr(aux), (N + 8) if u_g is not None else N,
                                        ops._ptr(ws), ops._ptr(cs_g.view if colsum else None), None, None, ops._stream()), what)
        torch.cuda.synchronize()
        for g, n in ((c_g, "C"), (u_g, "u"), (cs_g, "colsum")):
            if g is not None:
                g.intact(f"{what}:{n}")
        stats = G.check_outputs(what, ref, c_g.view.cpu(), u_g.view.cpu() if u_g is not None else None,
                                cs_g.view[0].cpu() if colsum else None)
        print(what, stats)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows", [33, 8192 + 3])
def test_layernorm_row8(A, rows):
    D = 512
    ops, lib = A.ops, A._lib.load()
    what = f"ln_row8[{rows}x{D}]"
    inp = L.make_inputs(rows, D, rows * 4099 + D * 7, BF, BF, BF)
    ref = L.reference(inp, None)
    dev = {k: (t.to(DEV) if torch.is_tensor(t) else t) for k, t in inp.items()}
    y, mean, rstd = Guarded(rows, D, BF), Guarded(1, rows, F32), Guarded(1, rows, F32)
    A._lib.check(lib.avf_layernorm_fwd_ex(ops._ptr(dev["x"]), ops.avf_dtype(BF), ops._ptr(dev["gamma"]), ops._ptr(dev["beta"]),
                                          ops._ptr(y.view), ops.avf_dtype(BF), ops._ptr(mean.view), ops._ptr(rstd.view), rows, D,
                                          float(L.EPS), ops._stream()), what)
    torch.cuda.synchronize()
    for g, n in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
        g.intact(f"{what}:{n}")
    stats = L.check_forward(what, ref, y.view.cpu(), mean.view[0].cpu(), rstd.view[0].cpu())
    lo = Guarded(rows, D, BF)
    dx, dx_lo, dx_m, dg, db, cs = ops.layernorm_bwd_ex(dev["dy"], dev["x"], dev["gamma"], mean.view[0].contiguous(),
                                                       rstd.view[0].contiguous(), dres=dev["dres"], want_dx=True, want_colsum=True,
                                                       dx_lo=lo.view)
    torch.cuda.synchronize()
    lo.intact(what + ":dx_lo")
    stats.update(L.check_backward(what, ref, dx.cpu(), dx_lo.cpu(), None, dg.cpu(), db.cpu(), cs.cpu(), dropout=False))
    print(what, stats)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("N", [17, 324, 512])
def test_resident_attention(A, N):
    B, H, dh = 1, 3, 64
    I = H * dh
    ops, lib = A.ops, A._lib.load()
    what = f"attn[{N}]"
    assert ops.attn_masked_on_mfma(N, dh)  # the lengths of the head-resident forward and the merged backward
    qkv, d_o = MA.make_operands(B, N, H, dh, 1000 + N)
    keep = torch.ones(B, N, dtype=torch.bool)
    ref = MA.reference(qkv, keep, B, N, H, dh, d_o)
    q, g = qkv.to(DEV), d_o.to(DEV)
    o, lse2, dqkv = Guarded(B * N, I, BF), Guarded(1, B * H * N, F32), Guarded(B * N, 3 * I, BF)
    A._lib.check(lib.avf_attn_fwd_qs(ops._ptr(q), ops._ptr(o.view), ops._ptr(lse2.view), B, N, H, dh, ops._stream()), what + ":fwd")
    ws = torch.empty(lib.avf_attn_bwd_workspace_bytes(B, N, H, dh) * 2, dtype=torch.uint8, device=DEV)
    A._lib.check(lib.avf_attn_bwd_qs(ops._ptr(q), ops._ptr(o.view), ops._ptr(g), ops._ptr(lse2.view), ops._ptr(dqkv.view), ops._ptr(ws),
                                     B, N, H, dh, ops._stream()), what + ":bwd")
    torch.cuda.synchronize()
    for t, n in ((o, "o"), (lse2, "lse2"), (dqkv, "dqkv")):
        t.intact(f"{what}:{n}")
    o_c, lse_c, dq_c = o.view.cpu(), lse2.view[0].cpu().view(B, H, N), dqkv.view.cpu()
    assert bool(torch.isfinite(o_c.float()).all()) and bool(torch.isfinite(lse_c).all()) and bool(torch.isfinite(dq_c.float()).all())
    MA.assert_grouped(what, MA.grouped_errors(o_c, ref["o"], keep, {"o": slice(None)}), MA.CAP_O, check)
    MA.assert_grouped(what, MA.grouped_errors(dq_c, ref["dqkv"], keep, MA.grad_parts(H, dh)), MA.CAP_GRAD, check)
    torch.testing.assert_close(lse_c, ref["lse2"].float(), **MA.LSE_TOL)


# ------------------------------------------------------------------------------------------------ whole steps
SQ = lambda y: y.pow(2).mean()


def _state(D, layers, H, dh, M, seed):
    import oracle
    g = torch.Generator().manual_seed(seed)
    sd = oracle.init_transformer_state(D, layers, H, dh, M, generator=g)
    for k in sd:  # a non-trivial LayerNorm affine: the dgamma / dbeta folds see real sums
        if k.endswith("norm.weight"):
            sd[k] = 1 + 0.1 * torch.randn(D, generator=g)
        if k.endswith("norm.bias"):
            sd[k] = 0.1 * torch.randn(D, generator=g)
    return sd, g


def _stack(A, sd, D, layers, H, dh, M):
    t = A.Transformer(D, layers, H, dh, M, 0.0, compute_dtype="bf16", residual_dtype="bf16")
    t.load_state_dict(sd, strict=True)
    return t.to(DEV)


def _eager(t, x):
    x = x.detach().to(DEV).clone().requires_grad_(True)
    for p in t.parameters():
        p.grad = None
    loss = SQ(t(x))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in t.named_parameters()}


def test_deferred_dw_of_two_layers(A, monkeypatch):
    """one avf_layers_dw call for both layers (320 .. 512 token rows, a multiple of the 64-row K-step) against the gradients
    avf_layer_bwd computes layer by layer: vectors bit for bit (same fold kernels, same partial rows), matrices to 1e-4 (the
    bounds of tests/test_gpu_dw_deferred.py)"""
    D, layers, H, dh, M, B, N = 128, 2, 4, 32, 256, 8, 64
    sd, g = _state(D, layers, H, dh, M, 77)
    x = torch.randn(B, N, D, generator=g)
    monkeypatch.setenv("AVF_DW_DEFER", "0")
    loss0, g0 = _eager(_stack(A, sd, D, layers, H, dh, M), x)
    monkeypatch.delenv("AVF_DW_DEFER")
    monkeypatch.setenv("AVF_DW_GROUP", "2")
    t = _stack(A, sd, D, layers, H, dh, M)
    loss, g1 = _eager(t, x)
    assert list(t.__dict__["_dw_plan_cache"][2]) == [2], t.__dict__.get("_dw_plan_cache")
    assert torch.equal(loss, loss0)
    for k in g0:
        assert bool(torch.isfinite(g1[k]).all()), k
        if g0[k].dim() == 1:
            assert torch.equal(g1[k], g0[k]), k
        else:
            assert rel_fro(g1[k], g0[k]) <= 1e-4, (k, rel_fro(g1[k], g0[k]))


def test_adam_table_with_a_matrix_and_a_short_vector(A):
    """p, m, v of every tensor against torch.optim.Adam fed the same gradients (the bound of tests/test_gpu_optim.py), and the
    images of W2 [512, 1536] the kernel writes beside them: bf16(W2) row-major, its transpose, and pack_ws of the transpose"""
    import copy

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stack = A.Transformer(512, 1, 8, 64, 1536, 0.0, compute_dtype="bf16", residual_dtype="bf16")
            self.v = torch.nn.Parameter(torch.linspace(-1, 1, 7))

    torch.manual_seed(11)
    ma = Net().to(DEV)
    mb = copy.deepcopy(ma)
    kw = dict(lr=3e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=1e-2)
    oa, ob = A.optim.FusedAdam(ma, **kw), torch.optim.Adam(mb.parameters(), **kw)
    x = torch.randn(2, 64, 512, device=DEV)
    (SQ(ma.stack(x)) + ma.v.pow(2).sum()).backward()  # (also prepares the stack's weight images)
    g = torch.Generator().manual_seed(12)
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        pa.grad = torch.randn(pa.shape, generator=g).to(DEV) * 0.1
        pb.grad = pa.grad.clone()
    oa.step()
    ob.step()
    torch.cuda.synchronize()
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert rel_fro(pa, pb) < 2e-6, (n, rel_fro(pa, pb))
        assert rel_fro(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]) < 1e-5, n
        assert rel_fro(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"]) < 1e-5, n
    st = ma.stack
    assert st._lowp_ready
    w2 = dict(st.named_parameters())["layers.0.1.fn.fn.net.3.weight"].detach()
    assert tuple(w2.shape) == (512, 1536)
    lo = w2.to(BF).contiguous()
    buf = st._lowp_bufs[0].view(torch.uint8)
    for name, img in (("row-major", lo), ("transposed", lo.t().contiguous()), ("fragment-major", A.ops.pack_ws(lo.t().contiguous()))):
        img = img.view(torch.uint8).flatten()
        n = img.numel()
        cand = (buf[: buf.numel() - n + 1].unfold(0, 64, 256) == img[:64]).all(1).nonzero().flatten() * 256  # (256-byte aligned images)
        assert any(torch.equal(buf[int(o): int(o) + n], img) for o in cand.tolist()), f"no {name} image of W2 in the layer's buffer"


def test_replayed_step_equals_the_eager_step(A):
    """d = 512 at 128 token rows in a captured step: row8 LayerNorm, head-resident attention, the NT GEMMs on the small-M tile 6
    (general epilogue), per-layer dW (128 rows: no deferred group) and folds.  Neither the lean tiles nor the persistent kernel
    (2048 rows and more) run here: their stores are held by the operator cases above.  A store that became visible late would
    show as a gradient that differs from the eager step's"""
    D, layers, H, dh, M, B, N = 512, 2, 8, 64, 1024, 2, 64
    sd, g = _state(D, layers, H, dh, M, 78)
    x = torch.randn(B, N, D, generator=g)
    loss0, g0 = _eager(_stack(A, sd, D, layers, H, dh, M), x)
    t = _stack(A, sd, D, layers, H, dh, M)
    opt = torch.optim.Adam(t.parameters(), lr=0.0, fused=True, capturable=True)  # lr 0: every replay starts from the same state
    batch = {"x": x.to(DEV)}
    step = A.graphs.GraphedTrainStep(t, opt, lambda m, b: SQ(m(b["x"])), batch, warmup=2)
    for _ in range(3):
        loss = step(batch)
        torch.cuda.synchronize()
    assert torch.equal(loss.detach().reshape(()), loss0.reshape(())), (float(loss), float(loss0))
    for k, p in t.named_parameters():
        assert torch.equal(p.grad, g0[k]), k
