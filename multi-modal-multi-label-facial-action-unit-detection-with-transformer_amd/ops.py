"""Tensor-level wrappers over the per-operator C entry points (used by the modules and by tests).

All tensors must live on a CUDA(HIP) device; nothing here falls back to PyTorch math.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Tuple

import torch

from . import _cabi, _lib
from ._lib import BF16, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_DGELU, EPI_NONE, F32  # noqa: F401

_TORCH2AVF = {torch.float32: F32, torch.bfloat16: BF16}
_AVF2TORCH = {F32: torch.float32, BF16: torch.bfloat16}


def avf_dtype(dt) -> int:
    if isinstance(dt, int):
        return dt
    if isinstance(dt, str):
        return {"f32": F32, "fp32": F32, "float32": F32, "bf16": BF16, "bfloat16": BF16}[dt.lower()]
    return _TORCH2AVF[dt]


def torch_dtype(dt) -> torch.dtype:
    return _AVF2TORCH[avf_dtype(dt)]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libavformer_hip operators need tensors on the MI355X (got a CPU tensor); "
                               "there is no CPU fallback in the product path")


def _bytes(n: int, device) -> torch.Tensor:
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=device)


def device_ok() -> bool:
    return bool(_lib.load().avf_device_ok())


# ------------------------------------------------------------------------------------------------
def layernorm_fwd(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5,
                  out_dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """nn.LayerNorm(dim) forward (reference models/heads.py:178-185).  x fp32 [..., D]."""
    _need_cuda(x, weight, bias)
    lib = _lib.load()
    x = x.contiguous()
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=torch_dtype(out_dtype), device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _lib.check(lib.avf_layernorm_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), avf_dtype(out_dtype), _ptr(mean),
                                     _ptr(rstd), rows, D, float(eps), _stream()), "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, weight, mean, rstd, dres=None, want_lo=False, want_colsum=False):
    """-> dx fp32, dx_lo (bf16 or None), dgamma, dbeta, colsum(dx) or None."""
    _need_cuda(dy, x, weight, mean, rstd, dres)
    lib = _lib.load()
    dy = dy.contiguous()
    x = x.contiguous()
    D = x.shape[-1]
    rows = x.numel() // D
    dx = torch.empty_like(x)
    dx_lo = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_lo else None
    dg = torch.empty(D, dtype=torch.float32, device=x.device)
    db = torch.empty(D, dtype=torch.float32, device=x.device)
    cs = torch.empty(D, dtype=torch.float32, device=x.device) if want_colsum else None
    ws = _bytes(lib.avf_layernorm_bwd_workspace_bytes(rows, D), x.device)
    _lib.check(lib.avf_layernorm_bwd(_ptr(dy), avf_dtype(dy.dtype), _ptr(x), _ptr(weight), _ptr(mean), _ptr(rstd),
                                     _ptr(dres.contiguous() if dres is not None else None), _ptr(dx), _ptr(dx_lo),
                                     _ptr(dg), _ptr(db), _ptr(cs), _ptr(ws), rows, D, _stream()), "layernorm_bwd")
    return dx, dx_lo, dg, db, cs


def layernorm_fwd_ex(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, out_dtype=torch.float32,
                     y: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """layernorm_fwd for an fp32 or bf16 x [rows, D] (avf_layernorm_fwd_ex); y: optional preallocated [rows, D] output."""
    _need_cuda(x, weight, bias, y)
    lib = _lib.load()
    assert x.is_contiguous() and x.dim() == 2 and (y is None or (y.is_contiguous() and y.shape == x.shape))
    rows, D = x.shape
    if y is None:
        y = torch.empty(x.shape, dtype=torch_dtype(out_dtype), device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _lib.check(lib.avf_layernorm_fwd_ex(_ptr(x), avf_dtype(x.dtype), _ptr(weight), _ptr(bias), _ptr(y), avf_dtype(y.dtype),
                                        _ptr(mean), _ptr(rstd), rows, D, float(eps), _stream()), "layernorm_fwd_ex")
    return y, mean, rstd


def layernorm_bwd_ex(dy, x, weight, mean, rstd, dres=None, want_dx=True, want_lo=False, want_m=False, want_colsum=False,
                     drop=None, dx_lo=None, dx_m=None):
    """avf_layernorm_bwd_ex on [rows, D] tensors of any accepted storage type -> dx (fp32 or None), dx_lo, dx_m (bf16 or
    None), dgamma, dbeta, colsum or None.  drop: (seed, layer, site, p) as ops.dropout_factors takes them, or None.
    dx_lo / dx_m: optional preallocated [rows, D] bf16 outputs (they imply want_lo / want_m)."""
    _need_cuda(dy, x, weight, mean, rstd, dres, dx_lo, dx_m)
    lib = _lib.load()
    assert all(t is None or (t.is_contiguous() and t.shape == x.shape) for t in (dy, x, dres, dx_lo, dx_m)) and x.dim() == 2
    rows, D = x.shape
    dev = x.device
    dx = torch.empty(x.shape, dtype=torch.float32, device=dev) if want_dx else None
    if dx_lo is None and want_lo:
        dx_lo = torch.empty(x.shape, dtype=torch.bfloat16, device=dev)
    if dx_m is None and want_m:
        dx_m = torch.empty(x.shape, dtype=torch.bfloat16, device=dev)
    dg = torch.empty(D, dtype=torch.float32, device=dev)
    db = torch.empty(D, dtype=torch.float32, device=dev)
    cs = torch.empty(D, dtype=torch.float32, device=dev) if want_colsum else None
    ws = _bytes(lib.avf_layernorm_bwd_workspace_bytes(rows, D), dev)
    seed, layer, site, p = drop if drop is not None else (0, 0, 0, 0.0)
    _lib.check(lib.avf_layernorm_bwd_ex(_ptr(dy), avf_dtype(dy.dtype), _ptr(x), avf_dtype(x.dtype), _ptr(weight), _ptr(mean),
                                        _ptr(rstd), _ptr(dres), avf_dtype(dres.dtype) if dres is not None else F32, _ptr(dx),
                                        _ptr(dx_lo), _ptr(dx_m), _ptr(dg), _ptr(db), _ptr(cs), _ptr(ws), rows, D,
                                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, layer, site, float(p), _stream()),
               "layernorm_bwd_ex")
    return dx, dx_lo, dx_m, dg, db, cs


def layernorm_fwd_embed(clip: torch.Tensor, audio: torch.Tensor, pos: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                        eps: float = 1e-5):
    """fuse_tokens(clip, audio, pos, out_bf16=True) and the bf16 LayerNorm of its rows in one launch (avf_layernorm_fwd_embed)
    -> x0 [B, Tv+Ta, D] bf16, y (bf16, same shape), mean, rstd; bit-identical to the two launches."""
    _need_cuda(clip, audio, pos, weight, bias)
    clip, audio, pos = clip.contiguous(), audio.contiguous(), pos.contiguous()
    B, Tv, D = clip.shape
    Ta = audio.shape[1]
    assert audio.shape[0] == B and audio.shape[2] == D and pos.numel() == (Tv + Ta) * D
    assert clip.dtype == audio.dtype == pos.dtype == torch.float32
    x0 = torch.empty((B, Tv + Ta, D), dtype=torch.bfloat16, device=clip.device)
    y = torch.empty_like(x0)
    mean = torch.empty(B * (Tv + Ta), dtype=torch.float32, device=clip.device)
    rstd = torch.empty_like(mean)
    _lib.check(_lib.load().avf_layernorm_fwd_embed(_ptr(clip), _ptr(audio), _ptr(pos), B, Tv, Ta, _ptr(x0), _ptr(weight), _ptr(bias),
                                                   _ptr(y), _ptr(mean), _ptr(rstd), D, float(eps), _stream()), "layernorm_fwd_embed")
    return x0, y, mean, rstd


def layernorm_bwd_pos(dy, x, weight, mean, rstd, dres, batch: int, d_pos: Optional[torch.Tensor] = None):
    """the all-bf16 LayerNorm backward of [batch * tokens, D] rows reduced over the clips (avf_layernorm_bwd_pos, token-major)
    -> d_pos [tokens, D] fp32 (= the column sums of dx over the clips; optionally preallocated), dgamma, dbeta."""
    _need_cuda(dy, x, weight, mean, rstd, dres, d_pos)
    lib = _lib.load()
    assert all(t is None or (t.is_contiguous() and t.shape == x.shape and t.dtype == torch.bfloat16) for t in (dy, x, dres))
    rows, D = x.shape
    tokens = rows // batch
    assert tokens * batch == rows
    dev = x.device
    if d_pos is None:
        d_pos = torch.empty((tokens, D), dtype=torch.float32, device=dev)
    dg = torch.empty(D, dtype=torch.float32, device=dev)
    db = torch.empty(D, dtype=torch.float32, device=dev)
    ws = _bytes(lib.avf_layernorm_bwd_pos_workspace_bytes(batch, tokens, D), dev)
    _lib.check(lib.avf_layernorm_bwd_pos(_ptr(dy), _ptr(x), _ptr(weight), _ptr(mean), _ptr(rstd), _ptr(dres), _ptr(d_pos), _ptr(dg),
                                         _ptr(db), _ptr(ws), batch, tokens, D, _stream()), "layernorm_bwd_pos")
    return d_pos, dg, db


def colsum(t: torch.Tensor) -> torch.Tensor:
    """column sums over all leading axes; a 2-D view whose rows are a constant stride apart (unit column stride) is read
    in place"""
    _need_cuda(t)
    lib = _lib.load()
    if not (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        t = t.contiguous()
    cols = t.shape[-1]
    rows = t.numel() // cols
    ld = t.stride(0) if t.dim() == 2 else cols
    out = torch.empty(cols, dtype=torch.float32, device=t.device)
    ws = _bytes(lib.avf_colsum_workspace_bytes(rows, cols), t.device)
    _lib.check(lib.avf_colsum(_ptr(t), avf_dtype(t.dtype), rows, cols, ld, _ptr(out), _ptr(ws), _stream()), "colsum")
    return out


def cast_bf16(t: torch.Tensor) -> torch.Tensor:
    _need_cuda(t)
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    _lib.check(_lib.load().avf_cast_f32_to_bf16(_ptr(t), _ptr(out), t.numel(), _stream()), "cast")
    return out


def prep_weight_bf16(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _need_cuda(w)
    w = w.contiguous()
    r, c = w.shape
    lo = torch.empty((r, c), dtype=torch.bfloat16, device=w.device)
    lo_t = torch.empty((c, r), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.load().avf_prep_weight_bf16(_ptr(w), _ptr(lo), _ptr(lo_t), r, c, _stream()), "prep_weight")
    return lo, lo_t


def _rows2d(t: torch.Tensor) -> torch.Tensor:
    """a 2-D operand as the library takes it: unit column stride, rows a constant stride (>= width) apart; else a copy"""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    return t.contiguous()


def gemm(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = True, out_dtype=None,
         epilogue: int = EPI_NONE, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         aux: Optional[torch.Tensor] = None, residual_ld: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """C = op(A) op(B) with a fused epilogue.  Returns C (and aux for EPI_BIAS_GELU).  A / B may be row-strided 2-D views
    (leading dimension = their row stride); residual_ld = 0 broadcasts one residual row over all rows (a positional
    table); out: a preallocated, possibly row-strided [M, >= N] fp32 / bf16 view to write into."""
    _need_cuda(a, b, bias, residual, aux)
    lib = _lib.load()
    a = _rows2d(a)
    b = _rows2d(b)
    assert a.dtype == b.dtype
    dt = avf_dtype(a.dtype)
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N = b.shape[0] if trans_b else b.shape[1]
    Kb = b.shape[1] if trans_b else b.shape[0]
    assert K == Kb, (a.shape, b.shape, trans_a, trans_b)
    cdt = torch_dtype(out_dtype) if out_dtype is not None else a.dtype
    if out is not None:
        assert out.dim() == 2 and out.shape[0] == M and out.shape[1] >= N and out.stride(1) == 1 and out.dtype == cdt
        c = out
    else:
        c = torch.empty((M, N), dtype=cdt, device=a.device)
    made_aux = None
    if epilogue == EPI_BIAS_GELU and aux is None:
        made_aux = aux = torch.empty((M, N), dtype=cdt, device=a.device)
    ws = _bytes(lib.avf_gemm_workspace_bytes(dt, int(trans_a), int(trans_b), M, N, K), a.device)
    if residual is not None and residual_ld is None:
        residual = residual.contiguous()
    _lib.check(lib.avf_gemm(dt, int(trans_a), int(trans_b), M, N, K, _ptr(a), a.stride(0), _ptr(b), b.stride(0),
                            _ptr(c), c.stride(0), avf_dtype(cdt), epilogue, _ptr(bias), _ptr(residual),
                            N if residual_ld is None else int(residual_ld), _ptr(aux), N, _ptr(ws), _stream()), "gemm")
    if made_aux is not None:
        return c, made_aux
    return c


def _row_view(name: str, t: torch.Tensor, rows: int, cols: int, dtype, who: str = "gemm_nt_ex") -> torch.Tensor:
    """a [rows, cols] operand of gemm_nt_ex / gemm_mx8_ex, used in place: its row stride is its leading dimension"""
    if not (t.dim() == 2 and tuple(t.shape) == (rows, cols) and t.stride(1) == 1 and t.stride(0) >= cols and t.dtype == dtype):
        raise ValueError(f"{who}: {name} must be a [{rows}, {cols}] {dtype} tensor or row-strided view of one "
                         f"(got {tuple(t.shape)}, strides {t.stride()}, {t.dtype})")
    return t


def gemm_nt_plan(M: int, N: int, K: int, out_dtype=torch.bfloat16, epilogue: int = EPI_NONE, bias: bool = True,
                 want_colsum: bool = False, p: float = 0.0, lda: Optional[int] = None, ldb: Optional[int] = None,
                 ldc: Optional[int] = None, ldres: Optional[int] = None, ldaux: Optional[int] = None) -> dict:
    """Which kernel ``gemm_nt_ex`` runs for these arguments (avf_gemm_nt_plan; 16-byte aligned operands assumed):
    dict(kind = 0 register-staged | 1 tiled, tile = the tile id or -1, lean = the LEAN code, wpf = weight warm-up on).
    Leading dimensions default to the dense ones."""
    out = [C.c_int(-1) for _ in range(4)]
    _lib.check(_lib.load().avf_gemm_nt_plan(int(M), int(N), int(K), int(K if lda is None else lda), int(K if ldb is None else ldb),
                                            int(N if ldc is None else ldc), avf_dtype(torch_dtype(out_dtype)), int(epilogue),
                                            int(bool(bias)), int(N if ldres is None else ldres), int(N if ldaux is None else ldaux),
                                            int(bool(want_colsum)), float(p), *[C.byref(o) for o in out]), "gemm_nt_plan")
    kind, tile, lean, wpf = (o.value for o in out)
    return dict(kind=kind, tile=tile, lean=lean, wpf=bool(wpf))


def gemm_nt_ex(a: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None, out_dtype=None, epilogue: int = EPI_NONE,
               bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
               want_colsum: bool = False, drop=None):
    """C = epilogue(A W^T) on the tiled / register-staged bf16 NT kernels (avf_gemm_nt_ex), with the column sums and the
    dropout site a layer call can ask of them.  a [M, K], w [N, K] bf16; out / residual / aux [M, N] in C's type; all five may
    be row-strided views (leading dimension = row stride).  EPI_BIAS_GELU writes aux (made here when not given), EPI_DGELU
    reads it.  drop: (seed, layer, site, p) as ops.dropout_factors takes them, or None.
    Returns (C, aux or None, column sums or None, plan) with plan = gemm_nt_plan of exactly this call."""
    _need_cuda(a, w, out, bias, residual, aux)
    lib = _lib.load()
    if a.dim() != 2 or w.dim() != 2 or a.shape[1] != w.shape[1]:
        raise ValueError(f"gemm_nt_ex: a is [M, K] and w is [N, K] (got {tuple(a.shape)}, {tuple(w.shape)})")
    M, K = a.shape
    N = w.shape[0]
    a = _row_view("a", a, M, K, torch.bfloat16)
    w = _row_view("w", w, N, K, torch.bfloat16)
    cdt = out.dtype if out is not None else (torch_dtype(out_dtype) if out_dtype is not None else torch.bfloat16)
    if cdt not in (torch.bfloat16, torch.float32):
        raise TypeError(f"gemm_nt_ex: C is bf16 or fp32, not {cdt}")
    c = _row_view("out", out, M, N, cdt) if out is not None else torch.empty((M, N), dtype=cdt, device=a.device)
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (N,) or not bias.is_contiguous()):
        raise TypeError("gemm_nt_ex: bias is a contiguous fp32 [N]")
    if (residual is not None) != (epilogue == EPI_BIAS_RES):
        raise ValueError("gemm_nt_ex: a residual goes with EPI_BIAS_RES, and only with it")
    if epilogue == EPI_DGELU and aux is None:
        raise ValueError("gemm_nt_ex: EPI_DGELU reads aux, the saved pre-activation")
    if epilogue in (EPI_NONE, EPI_BIAS_RES) and aux is not None:
        raise ValueError("gemm_nt_ex: aux goes with EPI_BIAS_GELU / EPI_DGELU only")
    if epilogue == EPI_BIAS_GELU and aux is None:
        aux = torch.empty((M, N), dtype=cdt, device=a.device)
    if residual is not None:
        residual = _row_view("residual", residual, M, N, cdt)
    if aux is not None:
        aux = _row_view("aux", aux, M, N, cdt)
    seed, layer, site, p = drop if drop is not None else (0, 0, 0, 0.0)
    cs = torch.empty(N, dtype=torch.float32, device=a.device) if want_colsum else None
    ws = _bytes(lib.avf_gemm_nt_ws_workspace_bytes(M, N), a.device) if want_colsum else None
    ldres = residual.stride(0) if residual is not None else N
    ldaux = aux.stride(0) if aux is not None else N
    plan = gemm_nt_plan(M, N, K, cdt, epilogue, bias is not None, want_colsum, p, a.stride(0), w.stride(0), c.stride(0), ldres, ldaux)
    for name, t in (("a", a), ("w", w), ("out", c), ("bias", bias), ("residual", residual), ("aux", aux)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"gemm_nt_ex: {name} must be 16-byte aligned")
    _lib.check(lib.avf_gemm_nt_ex(M, N, K, _ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(c), c.stride(0), avf_dtype(cdt),
                                  int(epilogue), _ptr(bias), _ptr(residual), ldres, _ptr(aux), ldaux, _ptr(ws), _ptr(cs),
                                  seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, layer, site, float(p), _stream()), "gemm_nt_ex")
    return c, aux, cs, plan


def pack_ws(w: torch.Tensor) -> torch.Tensor:
    """Fragment-major image of a bf16 weight [rows % 256 == 0, 512] for gemm_ws (avf_pack_weight_ws)."""
    _need_cuda(w)
    lib = _lib.load()
    w = _rows2d(w)
    assert w.dtype == torch.bfloat16
    rows, cols = w.shape
    n = lib.avf_pack_weight_ws_bytes(rows, cols)
    if n == 0:
        raise ValueError(f"pack_ws: needs rows % 256 == 0 and cols == 512, got {tuple(w.shape)}")
    out = torch.empty(n // 2, dtype=torch.bfloat16, device=w.device)
    _lib.check(lib.avf_pack_weight_ws(_ptr(w), w.stride(0), rows, cols, _ptr(out), _stream()), "pack_weight_ws")
    return out


def gemm_ws_used(M: int, n_out: int, K: int, epilogue: int = EPI_NONE, out_dtype=torch.bfloat16) -> bool:
    """True when ``gemm`` / the layer calls run this bf16 NT shape on the weight-stationary persistent kernel
    (avf_gemm_nt_ws_dispatch); ``gemm_ws`` itself forces that kernel for every shape it can run."""
    return bool(_lib.load().avf_gemm_nt_ws_dispatch(int(M), int(n_out), int(K), int(epilogue), avf_dtype(torch_dtype(out_dtype))))


def gemm_ws(a: torch.Tensor, w_packed: torch.Tensor, n_out: int, out_dtype=None, epilogue: int = EPI_NONE,
            bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
            want_colsum: bool = False, want_image: bool = False):
    """C = epilogue(A W^T) on the weight-stationary persistent kernel (avf_gemm_nt_ws); w_packed = pack_ws(W[n_out, 512]).
    Returns C (and the saved pre-activation for EPI_BIAS_GELU; and the column sums of C with want_colsum; and with want_image
    - EPI_DGELU with want_colsum - the MX-FP8 image (q, scales) of the fp32 values behind C)."""
    _need_cuda(a, w_packed, bias, residual, aux)
    lib = _lib.load()
    a = _rows2d(a)
    M, K = a.shape
    cdt = torch_dtype(out_dtype) if out_dtype is not None else a.dtype
    # the C ABI sees raw pointers: everything it cannot check is checked here
    if a.dtype != torch.bfloat16 or w_packed.dtype != torch.bfloat16:
        raise TypeError(f"gemm_ws: bf16 operands only (a {a.dtype}, w_packed {w_packed.dtype})")
    if K != 512 or w_packed.numel() != n_out * 512 or not w_packed.is_contiguous():
        raise ValueError(f"gemm_ws: a is [M, 512] and w_packed = pack_ws(W[{n_out}, 512]); got K = {K}, image of {w_packed.numel()} elements")
    if cdt not in (torch.bfloat16, torch.float32):
        raise TypeError(f"gemm_ws: C is bf16 or fp32, not {cdt}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != n_out):
        raise TypeError("gemm_ws: bias is fp32 [n_out]")
    for name, t in (("residual", residual), ("aux", aux)):
        if t is not None and (t.dtype != cdt or t.numel() != M * n_out):
            raise TypeError(f"gemm_ws: {name} is stored in C's type {cdt} as [M, n_out] (got {t.dtype}, {tuple(t.shape)})")
    if aux is not None and not aux.is_contiguous():
        raise ValueError("gemm_ws: aux must be contiguous")
    c = torch.empty((M, n_out), dtype=cdt, device=a.device)
    made_aux = None
    if epilogue == EPI_BIAS_GELU and aux is None:
        made_aux = aux = torch.empty((M, n_out), dtype=cdt, device=a.device)
    cs = torch.empty(n_out, dtype=torch.float32, device=a.device) if want_colsum else None
    ws = _bytes(lib.avf_gemm_nt_ws_workspace_bytes(M, n_out), a.device) if want_colsum else None
    if residual is not None:
        residual = residual.contiguous()
    cq = torch.empty((M, n_out), dtype=torch.uint8, device=a.device) if want_image else None
    csc = torch.empty((M, n_out // 32), dtype=torch.uint8, device=a.device) if want_image else None
    _lib.check(lib.avf_gemm_nt_ws(M, n_out, K, _ptr(a), a.stride(0), _ptr(w_packed), _ptr(c), c.stride(0), avf_dtype(cdt),
                                  epilogue, _ptr(bias), _ptr(residual), n_out, _ptr(aux), n_out, _ptr(ws), _ptr(cs), _ptr(cq),
                                  _ptr(csc), _stream()),
               "gemm_nt_ws")
    res = (c,)
    if made_aux is not None:
        res += (made_aux,)
    if want_colsum:
        res += (cs,)
    if want_image:
        res += (cq, csc)
    return res[0] if len(res) == 1 else res


TN_GROUP_PLAN_FIELDS = ("big", "waves", "tiles", "S", "kchunk", "xcd_groups", "blocks", "fold")


def gemm_tn_group_plan(shapes, K: int) -> dict:
    """What ``gemm_tn_group`` decides for problems of the shapes [(M_i, N_i), ...] over K reduction rows
    (avf_gemm_tn_group_plan: the launcher's own decision, host code only, no device needed): dict(big = 1 for the 256 x 128
    tile, waves per workgroup, tiles, S = split count, kchunk = rows per split, xcd_groups = block order of the 256 x 128
    kernel, blocks launched, fold = fold_group_kernel's instantiation: 2 .. 8, 0 = run-time loop, -1 = none; and
    workspace_bytes = what avf_gemm_tn_group_workspace_bytes promises for the group)."""
    lib = _lib.load()
    n = len(shapes)
    Ms = (C.c_int64 * n)(*[int(m) for m, _ in shapes])
    Ns = (C.c_int64 * n)(*[int(k) for _, k in shapes])
    out = (C.c_int32 * 8)()
    _lib.check(lib.avf_gemm_tn_group_plan(n, int(K), Ms, Ns, out), "gemm_tn_group_plan")
    plan = dict(zip(TN_GROUP_PLAN_FIELDS, (int(v) for v in out)))
    plan["workspace_bytes"] = int(lib.avf_gemm_tn_group_workspace_bytes(n, int(K), Ms, Ns))
    return plan


def gemm_tn_plan(M: int, N: int, K: int) -> dict:
    """What ``gemm(trans_a=True, trans_b=False)`` decides on bf16 operands (avf_gemm_tn_plan): dict(S = split count,
    kchunk = reduction rows per split)."""
    out = (C.c_int32 * 2)()
    _lib.check(_lib.load().avf_gemm_tn_plan(int(M), int(N), int(K), out), "gemm_tn_plan")
    return dict(S=int(out[0]), kchunk=int(out[1]))


def gemm_tn_group(pairs, outs=None, workspace=None):
    """[(A_i [K, M_i] bf16, B_i [K, N_i] bf16), ...] (up to 16, same K) -> [C_i [M_i, N_i] fp32 = A_i^T B_i]: the grouped
    weight-gradient launch of a layer's backward, or of up to four layers' (avf_gemm_tn_group).  outs: preallocated
    contiguous fp32 [M_i, N_i] tensors to write into (returned); workspace: a contiguous tensor of at least the bytes the
    launch needs (gemm_tn_group_plan) to hold the split-K slabs.  Without them both are made here."""
    lib = _lib.load()
    n = len(pairs)
    As = [a.contiguous() for a, _ in pairs]
    Bs = [b.contiguous() for _, b in pairs]
    _need_cuda(*As, *Bs)
    K = As[0].shape[0]
    assert all(a.shape[0] == K and b.shape[0] == K and a.dtype == b.dtype == torch.bfloat16 for a, b in zip(As, Bs))
    Ms = (C.c_int64 * n)(*[a.shape[1] for a in As])
    Ns = (C.c_int64 * n)(*[b.shape[1] for b in Bs])
    if outs is None:
        Cs = [torch.empty((a.shape[1], b.shape[1]), dtype=torch.float32, device=a.device) for a, b in zip(As, Bs)]
    else:
        Cs = list(outs)
        _need_cuda(*Cs)
        if len(Cs) != n or not all(c.dtype == torch.float32 and c.is_contiguous() and tuple(c.shape) == (a.shape[1], b.shape[1])
                                   for a, b, c in zip(As, Bs, Cs)):
            raise ValueError("gemm_tn_group: outs are contiguous fp32 [M_i, N_i] tensors, one per pair")
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    if workspace is None:
        ws = _bytes(lib.avf_gemm_tn_group_workspace_bytes(n, K, Ms, Ns), As[0].device)
    else:
        ws = workspace
        _need_cuda(ws)
        plan = gemm_tn_group_plan([(a.shape[1], b.shape[1]) for a, b in zip(As, Bs)], K)
        need = 0 if plan["S"] == 1 else 4 * plan["S"] * sum(a.shape[1] * b.shape[1] for a, b in zip(As, Bs))
        if need and (not ws.is_contiguous() or ws.numel() * ws.element_size() < need or ws.data_ptr() % 16):
            raise ValueError(f"gemm_tn_group: workspace must be contiguous, 16-byte aligned and hold {need} bytes")
    _lib.check(lib.avf_gemm_tn_group(n, K, arr(As), arr(Bs), arr(Cs), Ms, Ns, _ptr(ws), _stream()), "gemm_tn_group")
    return Cs


F32_KERNELS = ("x3", "mfma_t1", "mfma_t2")
_F32_MISALIGN_BITS = ("a", "b", "out", "bias", "residual", "aux", "workspace")


def gemm_f32_plan(M: int, N: int, K: int, trans_a: bool = False, trans_b: bool = True, epilogue: int = EPI_NONE,
                  bias: bool = False, workspace: bool = True, lda: Optional[int] = None, ldb: Optional[int] = None,
                  ldc: Optional[int] = None, ldres: Optional[int] = None, ldaux: Optional[int] = None, misaligned=()) -> dict:
    """What ``gemm_f32_ex`` decides for these arguments under the default arithmetic it reads (set_f32_arithmetic; avf_gemm_f32_plan: the
    launcher's own decision, host code only, no device needed): dict(kernel = "x3" (gemm_f32x3_kernel) | "mfma_t1" | "mfma_t2"
    (gemm_f32_kernel on 32 x 32 / 64 x 64 tiles), akf / bkf = the reduction is the unit-stride axis of A / B, S = split count,
    kchunk = reduction rows per split (0 unsplit), vec = 16-byte epilogue accesses of the x3 kernel).  Leading dimensions
    default to the dense ones; misaligned: names among a, b, out, bias, residual, aux, workspace of operands that are not
    16-byte aligned."""
    mask = sum(1 << _F32_MISALIGN_BITS.index(n) for n in misaligned)
    out = (C.c_int32 * 6)()
    _lib.check(_lib.load().avf_gemm_f32_plan(int(trans_a), int(trans_b), int(M), int(N), int(K),
                                             int((M if trans_a else K) if lda is None else lda),
                                             int((K if trans_b else N) if ldb is None else ldb), int(N if ldc is None else ldc),
                                             int(epilogue), int(bool(bias)), int(N if ldres is None else ldres),
                                             int(N if ldaux is None else ldaux), int(bool(workspace)), mask, out), "gemm_f32_plan")
    return dict(kernel=F32_KERNELS[out[0]], akf=bool(out[1]), bkf=bool(out[2]), S=int(out[3]), kchunk=int(out[4]), vec=bool(out[5]))


def gemm_f32_workspace_bytes(M: int, N: int, K: int, trans_a: bool = False, trans_b: bool = True) -> int:
    """the split-K workspace avf_gemm_workspace_bytes promises an fp32 GEMM of this shape (0: it never splits)"""
    return int(_lib.load().avf_gemm_workspace_bytes(F32, int(trans_a), int(trans_b), int(M), int(N), int(K)))


def _f32_view(who: str, name: str, t: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    if not (t.dim() == 2 and tuple(t.shape) == (rows, cols) and t.stride(1) == 1 and t.stride(0) >= cols and t.dtype == torch.float32):
        raise ValueError(f"{who}: {name} must be a [{rows}, {cols}] fp32 tensor or row-strided view of one "
                         f"(got {tuple(t.shape)}, strides {t.stride()}, {t.dtype})")
    return t


def gemm_f32_ex(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = True, out: Optional[torch.Tensor] = None,
                epilogue: int = EPI_NONE, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                aux: Optional[torch.Tensor] = None, drop=None, workspace=True):
    """C = epilogue(op(A) op(B)) on the fp32 GEMM family (avf_gemm_f32_ex) with the dropout site a layer call can ask of it.
    a is [M, K] ([K, M] with trans_a), b is [N, K] with trans_b ([K, N] without); out / residual / aux [M, N]; all fp32, all
    used in place as row-strided views (leading dimension = row stride, any alignment).  A 1-D residual [N] is the broadcast
    row (ldres = 0).  EPI_BIAS_GELU writes aux (made here when not given), EPI_DGELU reads it.  drop: (seed, layer, site, p) as
    ops.dropout_factors takes them, or None.  workspace: True = what avf_gemm_workspace_bytes asks for, made here; False / None
    = none (the call runs unsplit); or a contiguous tensor to hold the split-K slabs.
    Returns (C, aux or None, plan) with plan = gemm_f32_plan of exactly this call."""
    who = "gemm_f32_ex"
    _need_cuda(a, b, out, bias, residual, aux)
    lib = _lib.load()
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError(f"{who}: a and b are 2-D (got {tuple(a.shape)}, {tuple(b.shape)})")
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N, Kb = (b.shape[0], b.shape[1]) if trans_b else (b.shape[1], b.shape[0])
    if K != Kb:
        raise ValueError(f"{who}: reduction lengths differ ({tuple(a.shape)}, {tuple(b.shape)}, trans_a={trans_a}, trans_b={trans_b})")
    a = _f32_view(who, "a", a, *a.shape)
    b = _f32_view(who, "b", b, *b.shape)
    c = _f32_view(who, "out", out, M, N) if out is not None else torch.empty((M, N), dtype=torch.float32, device=a.device)
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (N,) or bias.stride(0) != 1):
        raise TypeError(f"{who}: bias is a unit-stride fp32 [N]")
    if (residual is not None) != (epilogue == EPI_BIAS_RES):
        raise ValueError(f"{who}: a residual goes with EPI_BIAS_RES, and only with it")
    if epilogue == EPI_DGELU and aux is None:
        raise ValueError(f"{who}: EPI_DGELU reads aux, the saved pre-activation")
    if epilogue in (EPI_NONE, EPI_BIAS_RES) and aux is not None:
        raise ValueError(f"{who}: aux goes with EPI_BIAS_GELU / EPI_DGELU only")
    if epilogue == EPI_BIAS_GELU and aux is None:
        aux = torch.empty((M, N), dtype=torch.float32, device=a.device)
    ldres = N
    if residual is not None:
        if residual.dim() == 1:
            if residual.dtype != torch.float32 or tuple(residual.shape) != (N,) or residual.stride(0) != 1:
                raise TypeError(f"{who}: a broadcast residual is a unit-stride fp32 [N]")
            ldres = 0
        else:
            ldres = _f32_view(who, "residual", residual, M, N).stride(0)
    ldaux = _f32_view(who, "aux", aux, M, N).stride(0) if aux is not None else N
    if workspace is True:
        ws = _bytes(gemm_f32_workspace_bytes(M, N, K, trans_a, trans_b), a.device)
    elif workspace is False or workspace is None:
        ws = None
    else:
        ws = workspace
        _need_cuda(ws)
        if not ws.is_contiguous() or ws.numel() * ws.element_size() < gemm_f32_workspace_bytes(M, N, K, trans_a, trans_b):
            raise ValueError(f"{who}: workspace must be contiguous and hold what gemm_f32_workspace_bytes asks for")
    seed, layer, site, p = drop if drop is not None else (0, 0, 0, 0.0)
    named = (("a", a), ("b", b), ("out", c), ("bias", bias), ("residual", residual), ("aux", aux), ("workspace", ws))
    plan = gemm_f32_plan(M, N, K, trans_a, trans_b, epilogue, bias is not None, ws is not None, a.stride(0), b.stride(0),
                         c.stride(0), ldres, ldaux, [n for n, t in named if t is not None and t.data_ptr() % 16])
    _lib.check(lib.avf_gemm_f32_ex(int(trans_a), int(trans_b), M, N, K, _ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(c),
                                   c.stride(0), int(epilogue), _ptr(bias), _ptr(residual), ldres, _ptr(aux), ldaux, _ptr(ws),
                                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, layer, site, float(p), _stream()), who)
    return c, aux, plan


def gemm_f32_tn_group_plan(shapes, K: int) -> dict:
    """What ``gemm_f32_tn_group`` decides for problems of the shapes [(M_i, N_i), ...] over K reduction rows under the default
    arithmetic it reads (set_f32_arithmetic; avf_gemm_f32_tn_group_plan, host code only): dict(ok = the grouped bf16x3 launch takes them,
    tiles = 128 x 128 tiles of the group, S = split count, kchunk = rows per split, workspace_bytes = what
    avf_gemm_f32_tn_group_workspace_bytes promises)."""
    lib = _lib.load()
    n = len(shapes)
    Ms = (C.c_int64 * n)(*[int(m) for m, _ in shapes])
    Ns = (C.c_int64 * n)(*[int(k) for _, k in shapes])
    out = (C.c_int32 * 4)()
    _lib.check(lib.avf_gemm_f32_tn_group_plan(n, int(K), Ms, Ns, out), "gemm_f32_tn_group_plan")
    return dict(ok=bool(out[0]), tiles=int(out[1]), S=int(out[2]), kchunk=int(out[3]),
                workspace_bytes=int(lib.avf_gemm_f32_tn_group_workspace_bytes(n, int(K), Ms, Ns)))


def gemm_f32_tn_group(pairs, outs=None, workspace=None):
    """[(A_i [K, M_i] fp32, B_i [K, N_i] fp32), ...] (2 .. 4, same K) -> [C_i [M_i, N_i] fp32 = A_i^T B_i] in the bf16x3
    arithmetic: the one launch that makes the weight gradients of a parity-mode layer (avf_gemm_f32_tn_group).  The operands
    are used in place as row-strided views (lda / ldb = their row strides), as the layer passes them.  outs: contiguous fp32
    [M_i, N_i] tensors to write into (returned); workspace: a contiguous, 16-byte aligned tensor of at least
    gemm_f32_tn_group_plan(...)["workspace_bytes"].  Raises where the plan says the group is not eligible."""
    who = "gemm_f32_tn_group"
    lib = _lib.load()
    n = len(pairs)
    K = pairs[0][0].shape[0]
    As = [_f32_view(who, "A", a, K, a.shape[1]) for a, _ in pairs]
    Bs = [_f32_view(who, "B", b, K, b.shape[1]) for _, b in pairs]
    _need_cuda(*As, *Bs)
    shapes = [(a.shape[1], b.shape[1]) for a, b in zip(As, Bs)]
    Ms = (C.c_int64 * n)(*[m for m, _ in shapes])
    Ns = (C.c_int64 * n)(*[k for _, k in shapes])
    lda = (C.c_int64 * n)(*[a.stride(0) for a in As])
    ldb = (C.c_int64 * n)(*[b.stride(0) for b in Bs])
    if outs is None:
        Cs = [torch.empty(s, dtype=torch.float32, device=As[0].device) for s in shapes]
    else:
        Cs = list(outs)
        _need_cuda(*Cs)
        if len(Cs) != n or not all(c.dtype == torch.float32 and c.is_contiguous() and tuple(c.shape) == s for c, s in zip(Cs, shapes)):
            raise ValueError(f"{who}: outs are contiguous fp32 [M_i, N_i] tensors, one per pair")
    need = int(lib.avf_gemm_f32_tn_group_workspace_bytes(n, K, Ms, Ns))
    if workspace is None:
        ws = _bytes(need, As[0].device)
    else:
        ws = workspace
        _need_cuda(ws)
        if not ws.is_contiguous() or ws.numel() * ws.element_size() < need or ws.data_ptr() % 16:
            raise ValueError(f"{who}: workspace must be contiguous, 16-byte aligned and hold {need} bytes")
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    _lib.check(lib.avf_gemm_f32_tn_group(n, K, arr(As), lda, arr(Bs), ldb, arr(Cs), Ms, Ns, _ptr(ws), _stream()), who)
    return Cs


def quant_mx8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[rows, cols] f32|bf16 -> (e4m3 bytes [rows, cols] uint8, E8M0 scale bytes [rows, cols/32] uint8)."""
    _need_cuda(x)
    x = x.contiguous()
    rows, cols = x.shape
    q = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    s = torch.empty((rows, cols // 32), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().avf_quant_mx8(avf_dtype(x.dtype), _ptr(x), rows, cols, _ptr(q), _ptr(s), _stream()), "quant_mx8")
    return q, s


def layernorm_fwd_mx8(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5):
    """LayerNorm rows -> (y bf16, mean, rstd, e4m3 image of y, its scale bytes)."""
    _need_cuda(x, weight, bias)
    x = x.contiguous()
    rows, dim = x.shape
    y = torch.empty((rows, dim), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    q = torch.empty((rows, dim), dtype=torch.uint8, device=x.device)
    s = torch.empty((rows, dim // 32), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().avf_layernorm_fwd_mx8(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(q),
                                                 _ptr(s), rows, dim, eps, _stream()), "layernorm_fwd_mx8")
    return y, mean, rstd, q, s


def layernorm_bwd_mx8(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                      dres: Optional[torch.Tensor] = None):
    """LayerNorm backward from a bf16 dy -> (dx fp32, dx bf16, e4m3 image of dx, its scale bytes, dgamma, dbeta)."""
    _need_cuda(dy, x, weight, mean, rstd, dres)
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.float32
    dy, x = dy.contiguous(), x.contiguous()
    rows, dim = x.shape
    lib = _lib.load()
    dev = x.device
    dx = torch.empty((rows, dim), dtype=torch.float32, device=dev)
    dx_lo = torch.empty((rows, dim), dtype=torch.bfloat16, device=dev)
    q = torch.empty((rows, dim), dtype=torch.uint8, device=dev)
    s = torch.empty((rows, dim // 32), dtype=torch.uint8, device=dev)
    dg = torch.empty(dim, dtype=torch.float32, device=dev)
    db = torch.empty(dim, dtype=torch.float32, device=dev)
    ws = torch.empty(max(1, lib.avf_layernorm_bwd_workspace_bytes(rows, dim)), dtype=torch.uint8, device=dev)
    _lib.check(lib.avf_layernorm_bwd_mx8(_ptr(dy), _ptr(x), _ptr(weight), _ptr(mean), _ptr(rstd),
                                         _ptr(dres.contiguous() if dres is not None else None), _ptr(dx), _ptr(dx_lo), _ptr(q),
                                         _ptr(s), _ptr(dg), _ptr(db), _ptr(ws), rows, dim, _stream()), "layernorm_bwd_mx8")
    return dx, dx_lo, q, s, dg, db


def attn_fwd_mx8(qkv: torch.Tensor, batch: int, tokens: int, heads: int, dim_head: int):
    """bf16 attention forward -> (o bf16 [B*N, I], lse2, e4m3 image of o, its scale bytes); dim_head 64, tokens <= 576."""
    _need_cuda(qkv)
    assert qkv.dtype == torch.bfloat16
    qkv = qkv.contiguous()
    inner = heads * dim_head
    dev = qkv.device
    o = torch.empty((batch * tokens, inner), dtype=torch.bfloat16, device=dev)
    lse2 = torch.empty((batch, heads, tokens), dtype=torch.float32, device=dev)
    q = torch.empty((batch * tokens, inner), dtype=torch.uint8, device=dev)
    s = torch.empty((batch * tokens, inner // 32), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().avf_attn_fwd_mx8(_ptr(qkv), _ptr(o), _ptr(lse2), _ptr(q), _ptr(s), batch, tokens, heads, dim_head,
                                            _stream()), "attn_fwd_mx8")
    return o, lse2, q, s


def attn_bwd_mx8(qkv, o, d_o, lse2, batch: int, tokens: int, heads: int, dim_head: int):
    """bf16 attention backward on PRE-SCALED queries -> (dqkv bf16 [B*N, 3I], its e4m3 image, the scale bytes [B*N, 3I/32]);
    only where the merged kernel runs (avf_attn_bwd_emits_mx8)."""
    _need_cuda(qkv, o, d_o, lse2)
    inner = heads * dim_head
    dev = qkv.device
    dqkv = torch.empty((batch * tokens, 3 * inner), dtype=torch.bfloat16, device=dev)
    q = torch.empty((batch * tokens, 3 * inner), dtype=torch.uint8, device=dev)
    s = torch.empty((batch * tokens, 3 * inner // 32), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().avf_attn_bwd_mx8(_ptr(qkv.contiguous()), _ptr(o.contiguous()), _ptr(d_o.contiguous()), _ptr(lse2), _ptr(dqkv),
                                            _ptr(q), _ptr(s), batch, tokens, heads, dim_head, _stream()), "attn_bwd_mx8")
    return dqkv, q, s


def gemm_mx8(a_q: torch.Tensor, a_s: torch.Tensor, b_q: torch.Tensor, b_s: torch.Tensor, out_dtype=torch.float32,
             epilogue: int = EPI_NONE, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
             want_image: bool = False, aux: Optional[torch.Tensor] = None):
    """C[M,N] = A[M,K] B[N,K]^T from MX-FP8 images (quant_mx8).  Returns C (and the saved pre-activation for
    EPI_BIAS_GELU; and with want_image the MX-FP8 image (q, scales) of C).  EPI_DGELU reads ``aux`` (the saved
    pre-activation, in C's type)."""
    _need_cuda(a_q, a_s, b_q, b_s, bias, residual, aux)
    M, K = a_q.shape
    N = b_q.shape[0]
    assert b_q.shape[1] == K and a_s.shape == (M, K // 32) and b_s.shape == (N, K // 32)
    c = torch.empty((M, N), dtype=out_dtype, device=a_q.device)
    if epilogue == EPI_DGELU:
        assert aux is not None and aux.shape == (M, N) and aux.dtype == out_dtype
        aux_in, aux = aux.contiguous(), None
    else:
        aux_in = None
        aux = torch.empty((M, N), dtype=out_dtype, device=a_q.device) if epilogue == EPI_BIAS_GELU else None
    cq = torch.empty((M, N), dtype=torch.uint8, device=a_q.device) if want_image else None
    cs = torch.empty((M, N // 32), dtype=torch.uint8, device=a_q.device) if want_image else None
    _lib.check(_lib.load().avf_gemm_mx8_nt(M, N, K, _ptr(a_q.contiguous()), _ptr(a_s.contiguous()), _ptr(b_q.contiguous()),
                                           _ptr(b_s.contiguous()), _ptr(c), N, avf_dtype(out_dtype), epilogue, _ptr(bias),
                                           _ptr(residual.contiguous() if residual is not None else None), N,
                                           _ptr(aux if aux is not None else aux_in), N, _ptr(cq), _ptr(cs), _stream()),
               "gemm_mx8_nt")
    out = (c, aux) if aux is not None else (c,)
    if want_image:
        out = out + (cq, cs)
    return out if len(out) > 1 else out[0]


def gemm_mx8_plan(M: int, N: int, K: int, out_dtype=torch.float32, epilogue: int = EPI_NONE, bias: bool = True,
                  want_colsum: bool = False, p: float = 0.0, want_image: bool = False, lda: Optional[int] = None,
                  ldb: Optional[int] = None, ldc: Optional[int] = None, ldres: Optional[int] = None,
                  ldaux: Optional[int] = None) -> dict:
    """Which instantiation ``gemm_mx8_ex`` runs for these arguments (avf_gemm_mx8_nt_plan; 16-byte aligned operands assumed):
    dict(tile = the tile id, lean = the LEAN code: 0 general epilogue, 1 lean, + 2 column sums, + 4 MX-FP8 image of C).
    Leading dimensions default to the dense ones (lda, ldb in bytes)."""
    out = [C.c_int(-1) for _ in range(2)]
    _lib.check(_lib.load().avf_gemm_mx8_nt_plan(int(M), int(N), int(K), int(K if lda is None else lda), int(K if ldb is None else ldb),
                                                int(N if ldc is None else ldc), avf_dtype(torch_dtype(out_dtype)), int(epilogue),
                                                int(bool(bias)), int(N if ldres is None else ldres),
                                                int(N if ldaux is None else ldaux), int(bool(want_colsum)), float(p),
                                                int(bool(want_image)), *[C.byref(o) for o in out]), "gemm_mx8_nt_plan")
    return dict(tile=out[0].value, lean=out[1].value)


def gemm_mx8_ex(a_q: torch.Tensor, a_s: torch.Tensor, b_q: torch.Tensor, b_s: torch.Tensor, out: Optional[torch.Tensor] = None,
                out_dtype=None, epilogue: int = EPI_NONE, bias: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None, want_colsum: bool = False, drop=None,
                want_image: bool = False):
    """C = epilogue(A B^T) from MX-FP8 images (avf_gemm_mx8_nt_ex) with the column sums, the dropout site and the operand /
    output views a layer call can ask of the kernel.  a_q [M, K], b_q [N, K] uint8 (row-strided views allowed: the row stride
    in bytes is the leading dimension); a_s [M, K/32], b_s [N, K/32] uint8, contiguous; out / residual / aux [M, N] in C's type,
    row-strided views allowed.  EPI_BIAS_GELU writes aux (made here when not given), EPI_DGELU reads it.  drop: (seed, layer,
    site, p) as ops.dropout_factors takes them, or None.  want_image: also the MX-FP8 image of C (BIAS_GELU / DGELU, N % 32 == 0);
    True, or the pair of buffers to write it to.
    Returns (C, aux or None, column sums or None, (image bytes, image scales) or None, plan) with plan = gemm_mx8_plan of
    exactly this call."""
    _need_cuda(a_q, a_s, b_q, b_s, out, bias, residual, aux)
    lib = _lib.load()
    if a_q.dim() != 2 or b_q.dim() != 2 or a_q.shape[1] != b_q.shape[1]:
        raise ValueError(f"gemm_mx8_ex: a_q is [M, K] and b_q is [N, K] (got {tuple(a_q.shape)}, {tuple(b_q.shape)})")
    M, K = a_q.shape
    N = b_q.shape[0]
    a_q = _row_view("a_q", a_q, M, K, torch.uint8, "gemm_mx8_ex")
    b_q = _row_view("b_q", b_q, N, K, torch.uint8, "gemm_mx8_ex")
    for name, t, rows in (("a_s", a_s, M), ("b_s", b_s, N)):
        if t.dtype != torch.uint8 or tuple(t.shape) != (rows, K // 32) or not t.is_contiguous():
            raise ValueError(f"gemm_mx8_ex: {name} must be a contiguous uint8 [{rows}, {K // 32}]")
    cdt = out.dtype if out is not None else (torch_dtype(out_dtype) if out_dtype is not None else torch.float32)
    if cdt not in (torch.bfloat16, torch.float32):
        raise TypeError(f"gemm_mx8_ex: C is bf16 or fp32, not {cdt}")
    c = torch.empty((M, N), dtype=cdt, device=a_q.device) if out is None else _row_view("out", out, M, N, cdt, "gemm_mx8_ex")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (N,) or not bias.is_contiguous()):
        raise TypeError("gemm_mx8_ex: bias is a contiguous fp32 [N]")
    if (residual is not None) != (epilogue == EPI_BIAS_RES):
        raise ValueError("gemm_mx8_ex: a residual goes with EPI_BIAS_RES, and only with it")
    if epilogue == EPI_DGELU and aux is None:
        raise ValueError("gemm_mx8_ex: EPI_DGELU reads aux, the saved pre-activation")
    if epilogue in (EPI_NONE, EPI_BIAS_RES) and aux is not None:
        raise ValueError("gemm_mx8_ex: aux goes with EPI_BIAS_GELU / EPI_DGELU only")
    if epilogue == EPI_BIAS_GELU and aux is None:
        aux = torch.empty((M, N), dtype=cdt, device=a_q.device)
    if residual is not None:
        residual = _row_view("residual", residual, M, N, cdt, "gemm_mx8_ex")
    if aux is not None:
        aux = _row_view("aux", aux, M, N, cdt, "gemm_mx8_ex")
    seed, layer, site, p = drop if drop is not None else (0, 0, 0, 0.0)
    cs = torch.empty(N, dtype=torch.float32, device=a_q.device) if want_colsum else None
    ws = _bytes(lib.avf_gemm_nt_ws_workspace_bytes(M, N), a_q.device) if want_colsum else None
    if isinstance(want_image, tuple):  # the caller's buffers: contiguous uint8 [M, N] and [M, N / 32]
        cq, csc = want_image
        if not (cq.dtype == csc.dtype == torch.uint8 and tuple(cq.shape) == (M, N) and tuple(csc.shape) == (M, N // 32) and
                cq.is_contiguous() and csc.is_contiguous() and cq.is_cuda and csc.is_cuda):
            raise ValueError("gemm_mx8_ex: the image buffers are contiguous uint8 [M, N] and [M, N / 32] on the device")
        want_image = True
    else:
        cq = torch.empty((M, N), dtype=torch.uint8, device=a_q.device) if want_image else None
        csc = torch.empty((M, N // 32), dtype=torch.uint8, device=a_q.device) if want_image else None
    ldres = residual.stride(0) if residual is not None else N
    ldaux = aux.stride(0) if aux is not None else N
    plan = gemm_mx8_plan(M, N, K, cdt, epilogue, bias is not None, want_colsum, p, want_image, a_q.stride(0), b_q.stride(0),
                         c.stride(0), ldres, ldaux)
    for name, t in (("a_q", a_q), ("b_q", b_q), ("out", c), ("bias", bias), ("residual", residual), ("aux", aux)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"gemm_mx8_ex: {name} must be 16-byte aligned")
    _lib.check(lib.avf_gemm_mx8_nt_ex(M, N, K, _ptr(a_q), a_q.stride(0), _ptr(a_s), _ptr(b_q), b_q.stride(0), _ptr(b_s), _ptr(c),
                                      c.stride(0), avf_dtype(cdt), int(epilogue), _ptr(bias), _ptr(residual), ldres, _ptr(aux),
                                      ldaux, _ptr(ws), _ptr(cs), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, layer, site,
                                      float(p), _ptr(cq), _ptr(csc), _stream()), "gemm_mx8_nt_ex")
    return c, aux, cs, ((cq, csc) if want_image else None), plan


def attn_fwd(qkv: torch.Tensor, batch: int, tokens: int, heads: int, dim_head: int, q_prescaled: bool = False):
    """Attention core on the packed QKV projection [B*N, 3*H*dh] -> (o [B*N, H*dh], lse2 [B,H,N]).
    q_prescaled (bf16 only): the q columns already carry log2(e)/sqrt(dim_head) (avf_attn_fwd_qs)."""
    _need_cuda(qkv)
    qkv = qkv.contiguous()
    inner = heads * dim_head
    assert qkv.shape == (batch * tokens, 3 * inner)
    o = torch.empty((batch * tokens, inner), dtype=qkv.dtype, device=qkv.device)
    lse2 = torch.empty((batch, heads, tokens), dtype=torch.float32, device=qkv.device)
    if q_prescaled:
        assert qkv.dtype == torch.bfloat16
        _lib.check(_lib.load().avf_attn_fwd_qs(_ptr(qkv), _ptr(o), _ptr(lse2), batch, tokens, heads, dim_head, _stream()),
                   "attn_fwd_qs")
    else:
        _lib.check(_lib.load().avf_attn_fwd(avf_dtype(qkv.dtype), _ptr(qkv), _ptr(o), _ptr(lse2), batch, tokens, heads,
                                            dim_head, _stream()), "attn_fwd")
    return o, lse2


def attn_bwd(qkv, o, d_o, lse2, batch: int, tokens: int, heads: int, dim_head: int, q_prescaled: bool = False) -> torch.Tensor:
    _need_cuda(qkv, o, d_o, lse2)
    lib = _lib.load()
    qkv, o, d_o = qkv.contiguous(), o.contiguous(), d_o.contiguous()
    dqkv = torch.empty_like(qkv)
    ws = _bytes(lib.avf_attn_bwd_workspace_bytes(batch, tokens, heads, dim_head), qkv.device)
    if q_prescaled:
        assert qkv.dtype == torch.bfloat16
        _lib.check(lib.avf_attn_bwd_qs(_ptr(qkv), _ptr(o), _ptr(d_o), _ptr(lse2), _ptr(dqkv), _ptr(ws), batch, tokens, heads,
                                       dim_head, _stream()), "attn_bwd_qs")
    else:
        _lib.check(lib.avf_attn_bwd(avf_dtype(qkv.dtype), _ptr(qkv), _ptr(o), _ptr(d_o), _ptr(lse2), _ptr(dqkv), _ptr(ws),
                                    batch, tokens, heads, dim_head, _stream()), "attn_bwd")
    return dqkv


ATTN_KINDS = {_cabi.header()[0]["AVF_ATTN_" + n.upper()]: n for n in ("res8", "res12", "res_multi", "stream", "f32")}
ATTN_MERGED = _cabi.header()[0]["AVF_ATTN_MERGED"]


def attn_plan(tokens: int, dim_head: int, q_prescaled: bool = False, masked: bool = False) -> dict:
    """Which kernels the bf16 attention core launches at this shape (avf_attn_plan, pure host code): attn_fwd / attn_bwd with
    this ``q_prescaled``, or with ``masked`` attn_fwd_masked / attn_bwd_masked(q_prescaled=True) and the layer itself.
    dict(fwd = "res8" | "res12" | "res_multi" (head-resident) | "stream" | "f32" (fp32 arithmetic), bwd = "stream" | "f32" |
    "merged", kb = key blocks per wave of the merged kernel (else 0), ragged = its last key block holds rows past tokens)."""
    fwd, bwd = C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.load().avf_attn_plan(int(tokens), int(dim_head), int(bool(q_prescaled)), int(bool(masked)), C.byref(fwd),
                                         C.byref(bwd)), "attn_plan")
    if bwd.value >= ATTN_MERGED:
        code = bwd.value - ATTN_MERGED
        return dict(fwd=ATTN_KINDS[fwd.value], bwd="merged", kb=code // 2, ragged=bool(code & 1))
    return dict(fwd=ATTN_KINDS[fwd.value], bwd=ATTN_KINDS[bwd.value], kb=0, ragged=False)


def attn_masked_on_mfma(tokens: int, dim_head: int) -> bool:
    """does the masked attention of a bf16 stack (attn_fwd_masked / attn_bwd_masked with q_prescaled=True, and the layer itself)
    run the masked MFMA kernels at this shape (avf_attn_masked_on_mfma), not the fp32-arithmetic ones"""
    return bool(_lib.load().avf_attn_masked_on_mfma(int(tokens), int(dim_head)))


LAYER_SMALL_FWD, LAYER_SMALL_BWD, LAYER_SMALL_ATT = 1, 2, 4


def layer_small_path(cfg: "_lib.LayerCfg") -> int:
    """which kernels a layer of this configuration (``Transformer._cfg(batch, tokens, keep=...)``) runs (avf_layer_small_path, pure
    host code): LAYER_SMALL_FWD - the single-launch short-sequence forward, LAYER_SMALL_BWD - the two fused backward kernels,
    LAYER_SMALL_ATT - the second of them runs the attention backward too; 0: the per-operator path"""
    return int(_lib.load().avf_layer_small_path(C.byref(cfg)))


def attn_fwd_masked(qkv: torch.Tensor, keep: torch.Tensor, batch: int, tokens: int, heads: int, dim_head: int,
                    q_prescaled: bool = False):
    """attn_fwd with the token mask of heads.py:225-232: keep [B, N] uint8 / bool, 1 = token kept (the reference's mask after
    its leading-True pad).  fp32 arithmetic on fp32 or bf16 storage.
    q_prescaled (bf16 only): the q columns already carry log2(e)/sqrt(dim_head) and the call runs what a bf16 layer runs
    (avf_attn_fwd_masked_qs): the masked MFMA kernels where attn_masked_on_mfma says, else the fp32-arithmetic ones."""
    _need_cuda(qkv, keep)
    qkv = qkv.contiguous()
    keep = keep.to(torch.uint8).contiguous()
    inner = heads * dim_head
    assert qkv.shape == (batch * tokens, 3 * inner) and keep.shape == (batch, tokens)
    o = torch.empty((batch * tokens, inner), dtype=qkv.dtype, device=qkv.device)
    lse2 = torch.empty((batch, heads, tokens), dtype=torch.float32, device=qkv.device)
    if q_prescaled:
        assert qkv.dtype == torch.bfloat16
        _lib.check(_lib.load().avf_attn_fwd_masked_qs(_ptr(qkv), _ptr(o), _ptr(lse2), _ptr(keep), batch, tokens, heads, dim_head,
                                                      _stream()), "attn_fwd_masked_qs")
    else:
        _lib.check(_lib.load().avf_attn_fwd_masked(avf_dtype(qkv.dtype), _ptr(qkv), _ptr(o), _ptr(lse2), _ptr(keep), batch, tokens,
                                                   heads, dim_head, _stream()), "attn_fwd_masked")
    return o, lse2


def attn_bwd_masked(qkv, o, d_o, lse2, keep, batch: int, tokens: int, heads: int, dim_head: int,
                    q_prescaled: bool = False) -> torch.Tensor:
    _need_cuda(qkv, o, d_o, lse2, keep)
    lib = _lib.load()
    qkv, o, d_o = qkv.contiguous(), o.contiguous(), d_o.contiguous()
    keep = keep.to(torch.uint8).contiguous()
    assert keep.shape == (batch, tokens)
    dqkv = torch.empty_like(qkv)
    ws = _bytes(lib.avf_attn_bwd_workspace_bytes(batch, tokens, heads, dim_head), qkv.device)
    if q_prescaled:
        assert qkv.dtype == torch.bfloat16
        _lib.check(lib.avf_attn_bwd_masked_qs(_ptr(qkv), _ptr(o), _ptr(d_o), _ptr(lse2), _ptr(dqkv), _ptr(ws), _ptr(keep), batch,
                                              tokens, heads, dim_head, _stream()), "attn_bwd_masked_qs")
    else:
        _lib.check(lib.avf_attn_bwd_masked(avf_dtype(qkv.dtype), _ptr(qkv), _ptr(o), _ptr(d_o), _ptr(lse2), _ptr(dqkv), _ptr(ws),
                                           _ptr(keep), batch, tokens, heads, dim_head, _stream()), "attn_bwd_masked")
    return dqkv


# ---- token producers / consumers either side of the stack (csrc/heads.hip) ---------------------------------------
def bn1d_fwd(x, gamma, beta, running_mean, running_var, num_batches_tracked, eps: float, momentum: float, training: bool):
    """nn.BatchNorm1d on [B, C] -> (y, mean, invstd); training updates the running statistics in place"""
    _need_cuda(x, gamma, beta, running_mean, running_var)
    x = x.contiguous()
    B, Cn = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(Cn, dtype=torch.float32, device=x.device)
    invstd = torch.empty(Cn, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().avf_bn1d_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                        _ptr(num_batches_tracked), _ptr(y), _ptr(mean), _ptr(invstd), B, Cn, float(eps),
                                        float(momentum), int(training), _stream()), "bn1d_fwd")
    return y, mean, invstd


def bn1d_bwd(x, dy, gamma, mean, invstd, training: bool, need_dx: bool = True):
    """-> (dx or None, dgamma, dbeta)"""
    _need_cuda(x, dy, gamma, mean, invstd)
    x, dy = x.contiguous(), dy.contiguous()
    B, Cn = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dg = torch.empty(Cn, dtype=torch.float32, device=x.device)
    db = torch.empty(Cn, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().avf_bn1d_bwd(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(dx), _ptr(dg), _ptr(db),
                                        B, Cn, int(training), _stream()), "bn1d_bwd")
    return dx, dg, db


def token_dots_fwd(tokens: torch.Tensor, w: torch.Tensor, pad_to: Optional[int] = None) -> torch.Tensor:
    """tokens [B,T,E] . w [T,E] (row-strided ok) -> [B, pad_to or T], columns T.. zero"""
    _need_cuda(tokens, w)
    tokens = tokens.contiguous()
    B, T, E = tokens.shape
    w = _rows2d(w)
    width = pad_to or T
    out = torch.empty((B, width), dtype=torch.float32, device=tokens.device)
    _lib.check(_lib.load().avf_token_dots_fwd(_ptr(tokens), _ptr(w), w.stride(0), _ptr(out), width, width, B, T, E, _stream()),
               "token_dots_fwd")
    return out


def token_dots_bwd(dout: torch.Tensor, tokens: torch.Tensor, w: torch.Tensor, need_dtokens=True, need_dw=True):
    _need_cuda(dout, tokens, w)
    tokens = tokens.contiguous()
    dout = _rows2d(dout)
    B, T, E = tokens.shape
    w = _rows2d(w)
    dtok = torch.empty_like(tokens) if need_dtokens else None
    dw = torch.empty((T, E), dtype=torch.float32, device=tokens.device) if need_dw else None
    _lib.check(_lib.load().avf_token_dots_bwd(_ptr(dout), dout.stride(0), _ptr(tokens), _ptr(w), w.stride(0), _ptr(dtok), _ptr(dw),
                                              E, B, T, E, _stream()), "token_dots_bwd")
    return dtok, dw


def assemble_tokens(x: torch.Tensor, lead: Optional[torch.Tensor], pos: Optional[torch.Tensor]) -> torch.Tensor:
    """[B,P,D] (+ lead rows [n_lead,D] in front) + pos[n_lead+P, D] -> [B, n_lead+P, D]"""
    _need_cuda(x, lead, pos)
    x = x.contiguous()
    B, P, D = x.shape
    n_lead = 0 if lead is None else lead.numel() // D
    out = torch.empty((B, P + n_lead, D), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().avf_assemble_tokens(_ptr(x), _ptr(lead.contiguous() if lead is not None else None),
                                               _ptr(pos.contiguous() if pos is not None else None), _ptr(out), B, P, n_lead, D,
                                               _stream()), "assemble_tokens")
    return out


def cat_features(a: torch.Tensor, v: torch.Tensor, pos: Optional[torch.Tensor]) -> torch.Tensor:
    """[B,T,Ea] ++ [B,T,Ev] on the feature axis + pos[T, Ea+Ev]"""
    _need_cuda(a, v, pos)
    a, v = a.contiguous(), v.contiguous()
    B, T, Ea = a.shape
    Ev = v.shape[2]
    out = torch.empty((B, T, Ea + Ev), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().avf_cat_features(_ptr(a), _ptr(v), _ptr(pos.contiguous() if pos is not None else None), _ptr(out), B, T,
                                            Ea, Ev, _stream()), "cat_features")
    return out


def transpose_add(x: torch.Tensor, pos: Optional[torch.Tensor]) -> torch.Tensor:
    """[B, R, C] -> [B, C, R] (+ pos [C, R])"""
    _need_cuda(x, pos)
    x = x.contiguous()
    B, R, Cn = x.shape
    out = torch.empty((B, Cn, R), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().avf_transpose_add(_ptr(x), _ptr(pos.contiguous() if pos is not None else None), _ptr(out), B, R, Cn,
                                             _stream()), "transpose_add")
    return out


def linear_pad_fwd(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], width: int) -> torch.Tensor:
    """[B, K] x [O, K]^T + b into a zero-padded [B, width] row, one launch (K % 4 == 0, K <= 4096)"""
    _need_cuda(x, w, b)
    x, w = x.contiguous(), w.contiguous()
    B, K = x.shape
    out = torch.empty((B, width), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().avf_linear_pad_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(out), B, K, w.shape[0], width, _stream()),
               "linear_pad_fwd")
    return out


def linear_pad_bwd(dout: torch.Tensor, x: torch.Tensor, w: torch.Tensor, need_dx=True, need_dw=True, need_db=True):
    """-> (dx [B, K], dw [O, K], db [O]) of linear_pad_fwd from the gradient of the padded row (read in place)"""
    _need_cuda(dout, x, w)
    assert dout.dim() == 2 and dout.stride(1) == 1 and dout.dtype == torch.float32
    B, K = x.shape
    O = w.shape[0]
    dev = x.device
    dx = torch.empty((B, K), dtype=torch.float32, device=dev) if need_dx else None
    dw = torch.empty((O, K), dtype=torch.float32, device=dev) if need_dw else None
    db = torch.empty(O, dtype=torch.float32, device=dev) if need_db else None
    _lib.check(_lib.load().avf_linear_pad_bwd(_ptr(dout), dout.stride(0), _ptr(x), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db), B, K, O,
                                              _stream()), "linear_pad_bwd")
    return dx, dw, db


def zero_cols(t: torch.Tensor, c0: int, c1: int):
    _need_cuda(t)
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32
    _lib.check(_lib.load().avf_zero_cols(_ptr(t), t.stride(0), t.shape[0], c0, c1, _stream()), "zero_cols")


def au_loss(logits: torch.Tensor, labels: torch.Tensor, pos_weight: torch.Tensor, ignore: float = -1.0):
    """-> (loss scalar tensor, dloss/dlogits [rows, ncls]).  Reference models/loss.py:75-103."""
    _need_cuda(logits, labels, pos_weight)
    assert logits.dim() == 2 and labels.dim() == 2 and logits.shape == labels.shape
    assert logits.stride(1) == 1 and labels.stride(1) == 1 and logits.dtype == torch.float32
    labels = labels.to(torch.float32)
    rows, ncls = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    grad = torch.empty((rows, ncls), dtype=torch.float32, device=logits.device)
    _lib.check(_lib.load().avf_au_loss(_ptr(logits), logits.stride(0), _ptr(labels), labels.stride(0), _ptr(pos_weight),
                                       float(ignore), rows, ncls, _ptr(loss), _ptr(grad), _stream()), "au_loss")
    return loss, grad


def au_loss_sum(logits: torch.Tensor, labels: torch.Tensor, pos_weight: torch.Tensor, ignore: float = -1.0):
    """-> ([sum over kept rows of the row-mean BCE, kept rows] as a 2-vector, d sum / d logits [rows, ncls]): the
    numerator / denominator of loss.py:85-102, for ranks that hold different numbers of ignored rows."""
    _need_cuda(logits, labels, pos_weight)
    assert logits.dim() == 2 and labels.dim() == 2 and logits.shape == labels.shape
    assert logits.stride(1) == 1 and labels.stride(1) == 1 and logits.dtype == torch.float32
    labels = labels.to(torch.float32)
    rows, ncls = logits.shape
    sc = torch.empty(2, dtype=torch.float32, device=logits.device)
    grad = torch.empty((rows, ncls), dtype=torch.float32, device=logits.device)
    _lib.check(_lib.load().avf_au_loss_sum(_ptr(logits), logits.stride(0), _ptr(labels), labels.stride(0), _ptr(pos_weight),
                                           float(ignore), rows, ncls, _ptr(sc), _ptr(grad), _stream()), "au_loss_sum")
    return sc, grad


def au_loss_wide(out: torch.Tensor, labels: torch.Tensor, pos_weight: torch.Tensor, ignore: float = -1.0, sum_mode: bool = False):
    """AULoss on the first ``labels.shape[1]`` slots of the model's output rows ``out`` [rows, width] -> (loss scalar, or the
    (sum, count) 2-vector with sum_mode; d / d out [rows, width], zero beyond the logits) - avf_au_loss_wide."""
    _need_cuda(out, labels, pos_weight)
    assert out.dim() == 2 and labels.dim() == 2 and out.shape[0] == labels.shape[0] and out.shape[1] >= labels.shape[1]
    assert out.stride(1) == 1 and labels.stride(1) == 1 and out.dtype == torch.float32
    labels = labels.to(torch.float32)
    rows, width = out.shape
    ncls = labels.shape[1]
    loss = torch.empty(2 if sum_mode else (), dtype=torch.float32, device=out.device)
    grad = torch.empty((rows, width), dtype=torch.float32, device=out.device)
    _lib.check(_lib.load().avf_au_loss_wide(_ptr(out), out.stride(0), _ptr(labels), labels.stride(0), _ptr(pos_weight), float(ignore),
                                            rows, ncls, width, 1 if sum_mode else 0, _ptr(loss), _ptr(grad), _stream()), "au_loss_wide")
    return loss, grad


def task_loss(out: torch.Tensor, y_ex: Optional[torch.Tensor], y_au: Optional[torch.Tensor], y_va: Optional[torch.Tensor],
              cfg: "_lib.TaskLossCfg"):
    """The EX / AU / VA losses on the model's output rows ``out`` [rows, width] in one launch (avf_task_loss) ->
    (losses [3], counts [3], grad_wide [rows, width]).  A label tensor that is None switches its task off: its loss is 0 and its
    column block of grad_wide zero.  y_ex int64 [rows]; y_au fp32 [rows, 12]; y_va fp32 [rows, cfg.va_ncols]."""
    _need_cuda(out, y_ex, y_au, y_va)
    assert out.dim() == 2 and out.stride(1) == 1 and out.dtype == torch.float32
    rows, width = out.shape
    assert y_ex is None or (y_ex.dtype == torch.int64 and y_ex.shape == (rows,) and y_ex.is_contiguous())
    assert y_au is None or (y_au.dtype == torch.float32 and y_au.shape == (rows, 12) and y_au.stride(1) == 1)
    assert y_va is None or (y_va.dtype == torch.float32 and y_va.shape == (rows, cfg.va_ncols) and y_va.stride(1) == 1)
    res = torch.empty(6, dtype=torch.float32, device=out.device)
    grad = torch.empty((rows, width), dtype=torch.float32, device=out.device)
    _lib.check(_lib.load().avf_task_loss(_ptr(out), out.stride(0), _ptr(y_ex), _ptr(y_au), 0 if y_au is None else y_au.stride(0),
                                         _ptr(y_va), 0 if y_va is None else y_va.stride(0), C.byref(cfg), rows, width,
                                         C.c_void_p(res.data_ptr()), C.c_void_p(res.data_ptr() + 12), _ptr(grad), _stream()),
               "task_loss")
    return res[:3], res[3:], grad


def task_loss_bwd(grad_wide: torch.Tensor, g_ex: Optional[torch.Tensor], g_au: Optional[torch.Tensor],
                  g_va: Optional[torch.Tensor], cfg: "_lib.TaskLossCfg") -> torch.Tensor:
    """grad_wide of task_loss scaled per column block by the incoming gradients of the three losses (fp32 device scalars; None:
    that block is zero) -> d / d out [rows, width], one launch (avf_task_loss_bwd)"""
    _need_cuda(grad_wide, g_ex, g_au, g_va)
    assert grad_wide.dim() == 2 and grad_wide.is_contiguous() and grad_wide.dtype == torch.float32
    assert all(g is None or (g.dtype == torch.float32 and g.numel() == 1) for g in (g_ex, g_au, g_va))
    rows, width = grad_wide.shape
    dout = torch.empty_like(grad_wide)
    _lib.check(_lib.load().avf_task_loss_bwd(_ptr(grad_wide), _ptr(g_ex), _ptr(g_au), _ptr(g_va), C.byref(cfg), rows, width,
                                             _ptr(dout), _stream()), "task_loss_bwd")
    return dout


def eval_update(out: torch.Tensor, y_ex: Optional[torch.Tensor], y_au: Optional[torch.Tensor], y_va: Optional[torch.Tensor],
                loss: Optional[torch.Tensor], cfg: "_lib.EvalCfg", state: Optional[torch.Tensor],
                pred_au: Optional[torch.Tensor] = None, pred_ex: Optional[torch.Tensor] = None,
                pred_va: Optional[torch.Tensor] = None) -> None:
    """One launch (avf_eval_update): adds the sufficient statistics of the rows ``out`` [rows, >= 21] and their labels into
    ``state`` (fp64 [128], layout in include/avformer_hip.h) and / or writes the per-row predictions.  A label tensor that is
    None leaves its task's slots alone; ``loss`` is an fp32 device scalar or None.  Allocates nothing, synchronises nothing."""
    _need_cuda(out, y_ex, y_au, y_va, loss, state, pred_au, pred_ex, pred_va)
    assert out.dim() == 2 and out.stride(1) == 1 and out.dtype == torch.float32
    rows, width = out.shape
    assert width >= max(cfg.ex_col + 7, cfg.au_col + 12, cfg.va_col + 2) and min(cfg.ex_col, cfg.au_col, cfg.va_col) >= 0
    assert y_ex is None or (y_ex.dtype == torch.int64 and y_ex.shape == (rows,) and y_ex.is_contiguous())
    assert y_au is None or (y_au.dtype == torch.float32 and y_au.shape == (rows, 12) and y_au.stride(1) == 1)
    assert y_va is None or (y_va.dtype == torch.float32 and y_va.shape == (rows, 2) and y_va.stride(1) == 1)
    assert loss is None or (loss.dtype == torch.float32 and loss.numel() == 1)
    assert state is None or (state.dtype == torch.float64 and state.shape == (128,) and state.is_contiguous())
    assert pred_au is None or (pred_au.dtype == torch.uint8 and pred_au.shape == (rows, 12) and pred_au.is_contiguous())
    assert pred_ex is None or (pred_ex.dtype == torch.int64 and pred_ex.shape == (rows,) and pred_ex.is_contiguous())
    assert pred_va is None or (pred_va.dtype == torch.float32 and pred_va.shape == (rows, 2) and pred_va.is_contiguous())
    _lib.check(_lib.load().avf_eval_update(_ptr(out), out.stride(0), _ptr(y_ex), _ptr(y_au), 0 if y_au is None else y_au.stride(0),
                                           _ptr(y_va), 0 if y_va is None else y_va.stride(0), _ptr(loss), C.byref(cfg), rows,
                                           _ptr(state), _ptr(pred_au), _ptr(pred_ex), _ptr(pred_va), _stream()), "eval_update")


def eval_scores(state: torch.Tensor, cfg: "_lib.EvalCfg", scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """state [128] -> the twelve fp64 scores on the device in one launch (avf_eval_scores): ex_acc, ex_f1, ex_score, au_acc, au_f1,
    au_score, ccc_v, ccc_a, va_score, avg_loss, ex_kept_rows, au_labelled"""
    _need_cuda(state, scores)
    assert state.dtype == torch.float64 and state.shape == (128,) and state.is_contiguous()
    if scores is None:
        scores = torch.empty(12, dtype=torch.float64, device=state.device)
    assert scores.dtype == torch.float64 and scores.shape == (12,) and scores.is_contiguous()
    _lib.check(_lib.load().avf_eval_scores(_ptr(state), C.byref(cfg), _ptr(scores), _stream()), "eval_scores")
    return scores


def mel_power(audio: torch.Tensor, window: torch.Tensor, fb: torch.Tensor, bin_lo: torch.Tensor, bin_hi: torch.Tensor, n_fft: int,
              hop: int, full_frames: int = 0, rows_per_clip: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """avf_mel_power: audio fp32 [rows, samples] -> (mel power fp32 [rows, n_mels, max(1 + samples // hop, full_frames)], peak
    uint32 bit patterns as int32 [rows // rows_per_clip]).  window [win_length], fb [n_fft // 2 + 1, n_mels] fp32; bin_lo / bin_hi
    int32 [n_mels] on the device."""
    _need_cuda(audio, window, fb, bin_lo, bin_hi)
    assert audio.dim() == 2 and audio.dtype == torch.float32 and audio.is_contiguous()
    assert window.dtype == torch.float32 and window.is_contiguous() and fb.dtype == torch.float32 and fb.is_contiguous()
    assert bin_lo.dtype == torch.int32 and bin_hi.dtype == torch.int32 and bin_lo.is_contiguous() and bin_hi.is_contiguous()
    rows, samples = audio.shape
    n_mels = fb.shape[1]
    assert fb.shape[0] == n_fft // 2 + 1 and bin_lo.numel() == n_mels and bin_hi.numel() == n_mels
    out_frames = max(1 + samples // max(int(hop), 1), int(full_frames))
    mel = torch.empty(rows, n_mels, out_frames, dtype=torch.float32, device=audio.device)
    peak = torch.empty(max(rows // max(int(rows_per_clip), 1), 1), dtype=torch.int32, device=audio.device)
    _lib.check(_lib.load().avf_mel_power(_ptr(audio), rows, samples, _ptr(window), window.numel(), int(n_fft), int(hop), _ptr(fb),
                                         _ptr(bin_lo), _ptr(bin_hi), n_mels, int(full_frames), int(rows_per_clip), _ptr(mel),
                                         _ptr(peak), _stream()), "mel_power")
    return mel, peak


def mel_db_norm(mel: torch.Tensor, peak: torch.Tensor, rows_per_clip: int, top_db: float, mean: float, std: float) -> torch.Tensor:
    """avf_mel_db_norm, IN PLACE on mel [rows, n_mels, frames] with the peak buffer of mel_power: dB, per-clip top_db clamp,
    (x - mean) / std.  Returns mel."""
    _need_cuda(mel, peak)
    assert mel.dim() == 3 and mel.dtype == torch.float32 and mel.is_contiguous() and peak.dtype == torch.int32
    rows, n_mels, frames = mel.shape
    assert rows % int(rows_per_clip) == 0 and peak.numel() >= rows // int(rows_per_clip)
    _lib.check(_lib.load().avf_mel_db_norm(_ptr(mel), _ptr(peak), rows, n_mels, frames, int(rows_per_clip), float(top_db),
                                           float(mean), float(std), _stream()), "mel_db_norm")
    return mel


_WAVE_DTYPES = {torch.float32: _lib.WAVE_F32, torch.int16: _lib.WAVE_I16}


def _wave_bank_args(wave: torch.Tensor, wav_start: torch.Tensor, wav_len: torch.Tensor, wav_of: torch.Tensor,
                    end_sample: torch.Tensor, index: torch.Tensor):
    """the tensors that avf_mel_power_bank and avf_wave_gather share: wave fp32 / int16 [total], wav_start / wav_len int64 [V],
    wav_of int32 [F], end_sample int64 [F], index int64 [B], contiguous and on one device"""
    _need_cuda(wave, wav_start, wav_len, wav_of, end_sample, index)
    assert wave.dim() == 1 and wave.dtype in _WAVE_DTYPES and wave.is_contiguous() and wave.numel() >= 1
    V, F = wav_start.numel(), wav_of.numel()
    assert wav_start.dtype == torch.int64 and wav_len.dtype == torch.int64 and wav_start.dim() == 1 and tuple(wav_len.shape) == (V,)
    assert wav_of.dtype == torch.int32 and wav_of.dim() == 1 and end_sample.dtype == torch.int64 and tuple(end_sample.shape) == (F,)
    assert index.dtype == torch.int64 and index.dim() == 1 and index.numel() >= 1
    for t in (wav_start, wav_len, wav_of, end_sample, index):
        assert t.is_contiguous() and t.device == wave.device
    return _WAVE_DTYPES[wave.dtype], V, F, index.numel()


def mel_power_bank(wave: torch.Tensor, wav_start: torch.Tensor, wav_len: torch.Tensor, wav_of: torch.Tensor,
                   end_sample: torch.Tensor, index: torch.Tensor, N: int, shift: int, window: torch.Tensor, fb: torch.Tensor,
                   bin_lo: torch.Tensor, bin_hi: torch.Tensor, n_fft: int, hop: int, full_frames: int,
                   out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """avf_mel_power_bank, one memset + one launch: the windows of index int64 [B] out of a waveform bank -> (mel power fp32
    [B, n_mels, full_frames], peak int32 [B]), each row what mel_power gives on the window's own samples; a silent window is all
    zero columns.  Everything is read on the device (no host synchronisation).  out: None, or a contiguous fp32 tensor
    [B, n_mels, full_frames] to write into."""
    dt, V, F, B = _wave_bank_args(wave, wav_start, wav_len, wav_of, end_sample, index)
    _need_cuda(window, fb, bin_lo, bin_hi)
    assert window.dtype == torch.float32 and window.is_contiguous() and fb.dtype == torch.float32 and fb.is_contiguous()
    assert bin_lo.dtype == torch.int32 and bin_hi.dtype == torch.int32 and bin_lo.is_contiguous() and bin_hi.is_contiguous()
    n_mels = fb.shape[1]
    assert fb.shape[0] == n_fft // 2 + 1 and bin_lo.numel() == n_mels and bin_hi.numel() == n_mels
    mel = torch.empty(B, n_mels, int(full_frames), dtype=torch.float32, device=wave.device) if out is None else out
    assert mel.dtype == torch.float32 and mel.is_contiguous() and tuple(mel.shape) == (B, n_mels, int(full_frames))
    assert mel.device == wave.device
    peak = torch.empty(B, dtype=torch.int32, device=wave.device)
    _lib.check(_lib.load().avf_mel_power_bank(_ptr(wave), dt, wave.numel(), _ptr(wav_start), _ptr(wav_len), V, _ptr(wav_of),
                                              _ptr(end_sample), F, _ptr(index), B, int(N), int(shift), _ptr(window), window.numel(),
                                              int(n_fft), int(hop), _ptr(fb), _ptr(bin_lo), _ptr(bin_hi), n_mels, int(full_frames),
                                              _ptr(mel), _ptr(peak), _stream()), "mel_power_bank")
    return mel, peak


def wave_gather(wave: torch.Tensor, wav_start: torch.Tensor, wav_len: torch.Tensor, wav_of: torch.Tensor, end_sample: torch.Tensor,
                index: torch.Tensor, N: int, w: int, shift: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """avf_wave_gather, one launch: the windows of index int64 [B] out of a waveform bank -> fp32 [B, N], every window right-aligned
    in N zeros (int16 samples times 2^-15), a silent window all zeros.  out: None, or a contiguous fp32 tensor [B, N] to write
    into (4-byte alignment is enough)."""
    dt, V, F, B = _wave_bank_args(wave, wav_start, wav_len, wav_of, end_sample, index)
    if out is None:
        out = torch.empty(B, int(N), dtype=torch.float32, device=wave.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, int(N)) and out.device == wave.device
    _lib.check(_lib.load().avf_wave_gather(_ptr(wave), dt, wave.numel(), _ptr(wav_start), _ptr(wav_len), V, _ptr(wav_of),
                                           _ptr(end_sample), F, _ptr(index), B, int(N), int(w), int(shift), _ptr(out), _stream()),
               "wave_gather")
    return out


CLIP_LAYOUTS ={"cthw": _lib.CLIP_CTHW, "tchw": _lib.CLIP_TCHW}


def clip_normalize(clip: torch.Tensor, lut: torch.Tensor, k: Optional[int] = None, flip: Optional[torch.Tensor] = None,
                   layout: str = "cthw", out_dtype=torch.float32) -> torch.Tensor:
    """avf_clip_normalize, one launch: clip uint8 [B, T, H, W, C] -> the last k channels as planes, [B, k, T, H, W] ("cthw") or
    [B, T, k, H, W] ("tchw"), value lut[c, byte] with lut fp32 [C, 256].  flip: bool / uint8 [B] on the device or None; where it
    is set the clip is mirrored along W.  The flags are read by the kernel (no host synchronisation)."""
    _need_cuda(clip, lut, flip)
    assert clip.dim() == 5 and clip.dtype == torch.uint8 and clip.is_contiguous()
    B, T, H, W, Cn = clip.shape
    k = Cn if k is None else int(k)
    assert lut.dtype == torch.float32 and lut.is_contiguous() and tuple(lut.shape) == (Cn, 256)
    if flip is not None:
        assert flip.dtype in (torch.bool, torch.uint8) and flip.is_contiguous() and tuple(flip.shape) == (B,)
    dt, lay = torch_dtype(out_dtype), CLIP_LAYOUTS[layout]
    shape = (B, k, T, H, W) if layout == "cthw" else (B, T, k, H, W)
    out = torch.empty(shape, dtype=dt, device=clip.device)
    _lib.check(_lib.load().avf_clip_normalize(_ptr(clip), B, T, H, W, Cn, k, _ptr(lut), _ptr(flip), _ptr(out), avf_dtype(dt),
                                              lay, _stream()), "clip_normalize")
    return out


def clip_denormalize(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, layout: str = "cthw") -> torch.Tensor:
    """avf_clip_denormalize, one launch: x fp32 / bf16 [B, C, T, H, W] ("cthw") or [B, T, C, H, W] ("tchw") -> uint8
    [B, T, H, W, C] = trunc(clamp(((x * std[c]) + mean[c]) * 255, 0, 255)), NaN -> 0; mean / std fp32 [C] on the device."""
    _need_cuda(x, mean, std)
    assert x.dim() == 5 and x.dtype in _TORCH2AVF and x.is_contiguous()
    lay = CLIP_LAYOUTS[layout]
    if layout == "cthw":
        B, Cn, T, H, W = x.shape
    else:
        B, T, Cn, H, W = x.shape
    for v in (mean, std):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.numel() == Cn
    out = torch.empty(B, T, H, W, Cn, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().avf_clip_denormalize(_ptr(x), avf_dtype(x.dtype), lay, B, T, H, W, Cn, _ptr(mean),
                                                _ptr(std), _ptr(out), _stream()), "clip_denormalize")
    return out


def clip_autoaugment_max_pixels() -> int:
    """the largest H * W of a frame avf_clip_autoaugment takes (two frame buffers of a workgroup's LDS; C = 4: 3/4 of it)"""
    return int(_lib.load().avf_clip_autoaugment_max_pixels())


def clip_autoaugment(clip: torch.Tensor, plan: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """avf_clip_autoaugment, one launch: clip uint8 [B, T, H, W, C] (C = 3 or 4) -> uint8 of the same shape, every frame through
    the two slots of plan int32 [B, T, 2, 8] on the device (augment.draw_plan / make_plan).  out: None, or a contiguous uint8
    tensor of the clip's shape - the clip itself is allowed."""
    _need_cuda(clip, plan, out)
    assert clip.dim() == 5 and clip.dtype == torch.uint8 and clip.is_contiguous()
    B, T, H, W, Cn = clip.shape
    assert plan.dtype == torch.int32 and plan.is_contiguous() and tuple(plan.shape) == (B, T, 2, 8)
    if out is None:
        out = torch.empty_like(clip)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == clip.shape and out.device == clip.device
    _lib.check(_lib.load().avf_clip_autoaugment(_ptr(clip), _ptr(out), B, T, H, W, Cn, _ptr(plan), _stream()), "clip_autoaugment")
    return out


def _planes_out(B: int, T: int, H: int, W: int, Cn: int, lut: torch.Tensor, k: Optional[int], flip: Optional[torch.Tensor],
                layout: str, out_dtype, device):
    """the output side that the entry points writing planes share: checks lut fp32 [C, 256] and flip [B], returns k, the avf
    dtype and layout codes and the empty output"""
    k = Cn if k is None else int(k)
    assert lut.dtype == torch.float32 and lut.is_contiguous() and tuple(lut.shape) == (Cn, 256)
    if flip is not None:
        assert flip.dtype in (torch.bool, torch.uint8) and flip.is_contiguous() and tuple(flip.shape) == (B,)
    dt, lay = torch_dtype(out_dtype), CLIP_LAYOUTS[layout]
    shape = (B, k, T, H, W) if layout == "cthw" else (B, T, k, H, W)
    return k, avf_dtype(dt), lay, torch.empty(shape, dtype=dt, device=device)


def clip_autoaugment_normalize(clip: torch.Tensor, plan: torch.Tensor, lut: torch.Tensor, k: Optional[int] = None,
                               flip: Optional[torch.Tensor] = None, layout: str = "cthw", out_dtype=torch.float32) -> torch.Tensor:
    """avf_clip_autoaugment_normalize, one launch: clip_normalize(clip_autoaugment(clip, plan), lut, k, flip, layout, out_dtype)
    without the augmented uint8 clip in between."""
    _need_cuda(clip, plan, lut, flip)
    assert clip.dim() == 5 and clip.dtype == torch.uint8 and clip.is_contiguous()
    B, T, H, W, Cn = clip.shape
    assert plan.dtype == torch.int32 and plan.is_contiguous() and tuple(plan.shape) == (B, T, 2, 8)
    k, dt, lay, out = _planes_out(B, T, H, W, Cn, lut, k, flip, layout, out_dtype, clip.device)
    _lib.check(_lib.load().avf_clip_autoaugment_normalize(_ptr(clip), B, T, H, W, Cn, _ptr(plan), k, _ptr(lut), _ptr(flip), _ptr(out),
                                                          dt, lay, _stream()), "clip_autoaugment_normalize")
    return out


def _bank_args(bank: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor], index: torch.Tensor):
    """the tensors that the avf_clip_gather* entry points share: bank uint8 [F, H, W, C], video_db_nr int32 [F], present uint8 /
    bool [F] or None, index int64 [B], contiguous and on one device"""
    _need_cuda(bank, video_db_nr, present, index)
    assert bank.dim() == 4 and bank.dtype == torch.uint8 and bank.is_contiguous()
    F = bank.shape[0]
    assert video_db_nr.dtype == torch.int32 and video_db_nr.is_contiguous() and tuple(video_db_nr.shape) == (F,)
    if present is not None:
        assert present.dtype in (torch.bool, torch.uint8) and present.is_contiguous() and tuple(present.shape) == (F,)
    assert index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1 and index.numel() >= 1
    for t in (video_db_nr, present, index):
        assert t is None or t.device == bank.device
    return F, index.numel()


def clip_gather(bank: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor], index: torch.Tensor, T: int,
                d: int) -> torch.Tensor:
    """avf_clip_gather, one launch: bank uint8 [F, H, W, C] -> the clips of index int64 [B], uint8 [B, T, H, W, C].  Slot t of
    sample b is frame index[b] - d * (T - 1 - t), black outside the bank, in another video (video_db_nr int32 [F]) or where
    present (uint8 / bool [F] or None) is 0.  Everything is read on the device (no host synchronisation)."""
    F, B = _bank_args(bank, video_db_nr, present, index)
    _, H, W, Cn = bank.shape
    out = torch.empty(B, int(T), H, W, Cn, dtype=torch.uint8, device=bank.device)
    _lib.check(_lib.load().avf_clip_gather(_ptr(bank), _ptr(video_db_nr), _ptr(present), _ptr(index), F, B, int(T), int(d), H, W, Cn,
                                           _ptr(out), _stream()), "clip_gather")
    return out


def clip_gather_normalize(bank: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor], index: torch.Tensor,
                          T: int, d: int, lut: torch.Tensor, k: Optional[int] = None, flip: Optional[torch.Tensor] = None,
                          layout: str = "cthw", out_dtype=torch.float32) -> torch.Tensor:
    """avf_clip_gather_normalize, one launch: clip_normalize(clip_gather(...), lut, k, flip, layout, out_dtype) without the
    uint8 clip in between."""
    F, B = _bank_args(bank, video_db_nr, present, index)
    _need_cuda(lut, flip)
    _, H, W, Cn = bank.shape
    T, k = int(T), Cn if k is None else int(k)
    assert lut.dtype == torch.float32 and lut.is_contiguous() and tuple(lut.shape) == (Cn, 256)
    if flip is not None:
        assert flip.dtype in (torch.bool, torch.uint8) and flip.is_contiguous() and tuple(flip.shape) == (B,)
    dt, lay = torch_dtype(out_dtype), CLIP_LAYOUTS[layout]
    shape = (B, k, T, H, W) if layout == "cthw" else (B, T, k, H, W)
    out = torch.empty(shape, dtype=dt, device=bank.device)
    _lib.check(_lib.load().avf_clip_gather_normalize(_ptr(bank), _ptr(video_db_nr), _ptr(present), _ptr(index), F, B, T, int(d), H, W,
                                                     Cn, k, _ptr(lut), _ptr(flip), _ptr(out), avf_dtype(dt), lay, _stream()),
               "clip_gather_normalize")
    return out


def clip_gather_autoaugment(bank: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor], index: torch.Tensor,
                            T: int, d: int, plan: torch.Tensor) -> torch.Tensor:
    """avf_clip_gather_autoaugment, one launch: clip_autoaugment(clip_gather(...), plan) without the plain clip in between;
    plan int32 [B, T, 2, 8] on the device."""
    F, B = _bank_args(bank, video_db_nr, present, index)
    _need_cuda(plan)
    _, H, W, Cn = bank.shape
    T = int(T)
    assert plan.dtype == torch.int32 and plan.is_contiguous() and tuple(plan.shape) == (B, T, 2, 8)
    out = torch.empty(B, T, H, W, Cn, dtype=torch.uint8, device=bank.device)
    _lib.check(_lib.load().avf_clip_gather_autoaugment(_ptr(bank), _ptr(video_db_nr), _ptr(present), _ptr(index), F, B, T, int(d), H,
                                                       W, Cn, _ptr(plan), _ptr(out), _stream()), "clip_gather_autoaugment")
    return out


def clip_gather_autoaugment_normalize(bank: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor],
                                      index: torch.Tensor, T: int, d: int, plan: torch.Tensor, lut: torch.Tensor,
                                      k: Optional[int] = None, flip: Optional[torch.Tensor] = None, layout: str = "cthw",
                                      out_dtype=torch.float32) -> torch.Tensor:
    """avf_clip_gather_autoaugment_normalize, one launch: clip_normalize(clip_gather_autoaugment(...), lut, k, flip, layout,
    out_dtype) without a uint8 clip in between - the training transform from the bank."""
    F, B = _bank_args(bank, video_db_nr, present, index)
    _need_cuda(plan, lut, flip)
    _, H, W, Cn = bank.shape
    T = int(T)
    assert plan.dtype == torch.int32 and plan.is_contiguous() and tuple(plan.shape) == (B, T, 2, 8)
    k, dt, lay, out = _planes_out(B, T, H, W, Cn, lut, k, flip, layout, out_dtype, bank.device)
    _lib.check(_lib.load().avf_clip_gather_autoaugment_normalize(_ptr(bank), _ptr(video_db_nr), _ptr(present), _ptr(index), F, B, T,
                                                                 int(d), H, W, Cn, _ptr(plan), k, _ptr(lut), _ptr(flip), _ptr(out),
                                                                 dt, lay, _stream()), "clip_gather_autoaugment_normalize")
    return out


def feature_clip_tokens(feat: torch.Tensor, black: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor],
                        index: torch.Tensor, T: int, d: int, lead: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """avf_feature_clip_tokens, one launch: feat fp32 [F, D] (unit column stride, any row stride that is a multiple of 4) ->
    fp32 [B, n_lead + T, D] = cat(lead [n_lead, D], the rows of the clips of index int64 [B]) + pos [n_lead + T, D].  Slot t of
    sample b is row index[b] - d * (T - 1 - t), ``black`` [D] outside the bank, in another video (video_db_nr int32 [F]) or where
    present (uint8 / bool [F] or None) is 0.  Everything is read on the device (no host synchronisation)."""
    _need_cuda(feat, black, video_db_nr, present, index, lead, pos, out)
    assert feat.dim() == 2 and feat.dtype == torch.float32 and feat.stride(1) == 1
    F, D = feat.shape
    assert black.dtype == torch.float32 and tuple(black.shape) == (D,) and black.is_contiguous()
    assert video_db_nr.dtype == torch.int32 and video_db_nr.is_contiguous() and tuple(video_db_nr.shape) == (F,)
    if present is not None:
        assert present.dtype in (torch.bool, torch.uint8) and present.is_contiguous() and tuple(present.shape) == (F,)
    assert index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1 and index.numel() >= 1
    B, T = index.numel(), int(T)
    n_lead = 0 if lead is None else lead.shape[0]
    assert lead is None or (lead.dtype == torch.float32 and lead.is_contiguous() and tuple(lead.shape) == (n_lead, D))
    assert pos is None or (pos.dtype == torch.float32 and pos.is_contiguous() and tuple(pos.shape) == (n_lead + T, D))
    for t in (black, video_db_nr, present, index, lead, pos, out):
        assert t is None or t.device == feat.device
    if out is None:
        out = torch.empty((B, n_lead + T, D), dtype=torch.float32, device=feat.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, n_lead + T, D)
    _lib.check(_lib.load().avf_feature_clip_tokens(_ptr(feat), feat.stride(0), _ptr(black), _ptr(video_db_nr), _ptr(present),
                                                   _ptr(index), F, B, T, int(d), D, _ptr(lead), n_lead, _ptr(pos), _ptr(out),
                                                   _stream()), "feature_clip_tokens")
    return out


def fuse_tokens(clip: torch.Tensor, audio: torch.Tensor, pos: Optional[torch.Tensor], out_bf16: bool = False) -> torch.Tensor:
    """[B,Tv,D] ++ [B,Ta,D] on the token axis, + pos[Tv+Ta, D] (nullable): one pass (avf_fuse_tokens); out_bf16: the
    result is written in bf16 (the storage type of a bf16 residual stream, avf_fuse_tokens_bf16)."""
    _need_cuda(clip, audio)
    clip, audio = clip.contiguous(), audio.contiguous()
    B, Tv, D = clip.shape
    Ta = audio.shape[1]
    assert audio.shape[0] == B and audio.shape[2] == D and clip.dtype == audio.dtype == torch.float32
    if pos is not None:
        pos = pos.contiguous()
        assert pos.numel() == (Tv + Ta) * D and pos.dtype == torch.float32
    out = torch.empty((B, Tv + Ta, D), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=clip.device)
    fn = _lib.load().avf_fuse_tokens_bf16 if out_bf16 else _lib.load().avf_fuse_tokens
    _lib.check(fn(_ptr(clip), _ptr(audio), _ptr(pos), _ptr(out), B, Tv, Ta, D, _stream()), "fuse_tokens")
    return out


def token_mean_fwd(y: torch.Tensor) -> torch.Tensor:
    """[B,T,D] fp32 (or bf16: the bf16 residual stream) -> [B,D] fp32 mean over tokens."""
    _need_cuda(y)
    y = y.contiguous()
    B, T, D = y.shape
    out = torch.empty((B, D), dtype=torch.float32, device=y.device)
    fn = _lib.load().avf_token_mean_fwd_bf16 if y.dtype == torch.bfloat16 else _lib.load().avf_token_mean_fwd
    _lib.check(fn(_ptr(y), _ptr(out), B, T, D, _stream()), "token_mean_fwd")
    return out


def token_mean_bwd(g: torch.Tensor, tokens: int, want_bf16: bool = False, want_colsum: bool = False):
    """g [B,D] -> dy [B,T,D] = g/T broadcast (+ optional bf16 copy and column sums over all B*T rows)."""
    _need_cuda(g)
    g = g.contiguous().to(torch.float32)
    B, D = g.shape
    dy = torch.empty((B, tokens, D), dtype=torch.float32, device=g.device)
    lo = torch.empty((B, tokens, D), dtype=torch.bfloat16, device=g.device) if want_bf16 else None
    cs = torch.empty(D, dtype=torch.float32, device=g.device) if want_colsum else None
    _lib.check(_lib.load().avf_token_mean_bwd(_ptr(g), _ptr(dy), _ptr(lo), _ptr(cs), B, tokens, D, _stream()),
               "token_mean_bwd")
    return dy, lo, cs


# frozen ResNet stages (csrc/conv.hip; csrc/conv_f32.hip: the same kernel, csrc/conv_kernel.hpp, in the parity arithmetic) --------
def _conv_pack(images: int, w, gamma, beta, running_mean, running_var, eps):
    """the body of ``conv_pack_weight`` (images = 1) and ``conv_pack_weight_f32`` (2): -> ([image, ...], scale, shift)"""
    _need_cuda(w, gamma, beta, running_mean, running_var)
    ts = [t.detach().contiguous() for t in (w, gamma, beta, running_mean, running_var)]
    assert all(t.dtype == torch.float32 for t in ts) and ts[0].dim() == 4 and ts[0].shape[2] == ts[0].shape[3]
    Cout, Cin, k, _ = ts[0].shape
    assert all(t.numel() == Cout for t in ts[1:])
    ws = [torch.empty((Cout, k * k * Cin), dtype=torch.bfloat16, device=w.device) for _ in range(images)]
    scale = torch.empty(Cout, dtype=torch.float32, device=w.device)
    shift = torch.empty(Cout, dtype=torch.float32, device=w.device)
    fn, name = ((_lib.load().avf_conv_pack_weight, "conv_pack_weight") if images == 1 else
                (_lib.load().avf_conv_pack_weight_f32x3, "conv_pack_weight_f32"))
    _lib.check(fn(*[_ptr(t) for t in ts], float(eps), *[_ptr(t) for t in ws], _ptr(scale), _ptr(shift), Cout, Cin, k, _stream()), name)
    return ws, scale, shift


def conv_pack_weight(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
                     running_var: torch.Tensor, eps: float = 1e-5):
    """nn.Conv2d weight [Cout, Cin, k, k] fp32 + BatchNorm2d's eval-mode statistics -> (w_packed [Cout, k*k*Cin] bf16 ordered
    tap-major / channel-minor, scale [Cout], shift [Cout] fp32) for ``conv2d_nhwc`` (avf_conv_pack_weight)."""
    (wp,), scale, shift = _conv_pack(1, w, gamma, beta, running_mean, running_var, eps)
    return wp, scale, shift


def conv_out_hw(H: int, W: int, k: int, stride: int) -> Tuple[int, int]:
    pad = 1 if k == 3 else 0
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv_plan(N: int, H: int, W: int, Cin: int, Cout: int, k: int, stride: int = 1) -> dict:
    """The tile ``conv2d_nhwc`` runs this shape on (avf_conv_plan): dict(tile = 0 | 1, tile_m, tile_n).  Raises on a shape
    the kernel does not take."""
    out = [C.c_int(-1) for _ in range(3)]
    _lib.check(_lib.load().avf_conv_plan(int(N), int(H), int(W), int(Cin), int(Cout), int(k), int(stride), *[C.byref(o) for o in out]),
               "conv_plan")
    return dict(tile=out[0].value, tile_m=out[1].value, tile_n=out[2].value)


def _conv2d(name: str, x, ws, scale, shift, k, stride, residual, relu, out, out_dtype):
    """the body of ``conv2d_nhwc`` (ws = (w_packed,); the maps fp32 or bf16) and ``conv2d_nhwc_f32`` (ws = (w_hi, w_lo); the maps
    fp32, checked): shapes / contiguity / dtypes, allocation, the call"""
    f32 = len(ws) == 2
    _need_cuda(x, *ws, scale, shift, residual, out)
    N, H, W, Cin = x.shape
    Cout = ws[0].shape[0]
    Ho, Wo = conv_out_hw(H, W, k, stride)
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch_dtype(out_dtype), device=x.device)
    wnames = ("w_hi", "w_lo") if f32 else ("w_packed",)
    for nm, t, shape, dt in ([("x", x, (N, H, W, Cin), torch.float32)] + [(nm, t, (Cout, k * k * Cin), torch.bfloat16) for nm, t in zip(wnames, ws)] +
                             [("scale", scale, (Cout,), torch.float32), ("shift", shift, (Cout,), torch.float32),
                              ("residual", residual, (N, Ho, Wo, Cout), torch.float32), ("out", out, (N, Ho, Wo, Cout), torch.float32)]):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or (f32 and t.dtype != dt)):
            raise ValueError(f"{name}: {nm} must be a contiguous {shape}{f' {dt}' if f32 else ''} tensor (got {tuple(t.shape)}, strides "
                             f"{t.stride()}, {t.dtype})")
    assert ws[0].dtype == torch.bfloat16 and scale.dtype == shift.dtype == torch.float32
    ptrs, geom = [_ptr(t) for t in (*ws, scale, shift, residual)], (N, H, W, Cin, Cout, _stream())
    if f32:
        rc = _lib.load().avf_conv2d_nhwc_f32x3(_ptr(x), *ptrs, int(bool(relu)), int(k), int(stride), _ptr(out), *geom)
    else:
        rc = _lib.load().avf_conv2d_nhwc(_ptr(x), avf_dtype(x.dtype), *ptrs, avf_dtype(residual.dtype) if residual is not None else F32,
                                         int(bool(relu)), int(k), int(stride), _ptr(out), avf_dtype(out.dtype), *geom)
    _lib.check(rc, name)
    return out


def conv2d_nhwc(x: torch.Tensor, w_packed: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, k: int, stride: int = 1,
                residual: Optional[torch.Tensor] = None, relu: bool = False, out: Optional[torch.Tensor] = None,
                out_dtype=torch.bfloat16) -> torch.Tensor:
    """relu?(conv(x, w) * scale + shift (+ residual)) on NHWC activations (avf_conv2d_nhwc): x [N, H, W, Cin] fp32 or bf16,
    w_packed / scale / shift from ``conv_pack_weight``, k = 3 (pad 1) or 1 (pad 0), stride 1 or 2; residual / out
    [N, Ho, Wo, Cout] fp32 or bf16.  Forward only."""
    return _conv2d("conv2d_nhwc", x, (w_packed,), scale, shift, k, stride, residual, relu, out, out_dtype)


def conv_pack_weight_f32(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
                         running_var: torch.Tensor, eps: float = 1e-5):
    """``conv_pack_weight`` for ``conv2d_nhwc_f32``: -> ((w_hi, w_lo), scale, shift), w_hi = bf16(w) and w_lo = bf16(w - w_hi),
    each [Cout, k*k*Cin] bf16 tap-major / channel-minor; scale / shift [Cout] fp32 (avf_conv_pack_weight_f32x3)."""
    ws, scale, shift = _conv_pack(2, w, gamma, beta, running_mean, running_var, eps)
    return tuple(ws), scale, shift


def conv2d_nhwc_f32(x: torch.Tensor, w_split, scale: torch.Tensor, shift: torch.Tensor, k: int, stride: int = 1,
                    residual: Optional[torch.Tensor] = None, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``conv2d_nhwc`` in the parity arithmetic (avf_conv2d_nhwc_f32x3): x [N, H, W, Cin], residual and out [N, Ho, Wo, Cout] all
    fp32, ``w_split`` = (w_hi, w_lo) / scale / shift from ``conv_pack_weight_f32``.  Every fp32 product runs as three bf16 MFMA
    products (bf16x3, oracle/bf16x3.py).  That is the convolution's one parity arithmetic: ``set_f32_arithmetic("f32")`` does not
    reach it.  Same shapes, tiles (``conv_plan``) and errors as ``conv2d_nhwc``.  Forward only."""
    w_hi, w_lo = w_split
    return _conv2d("conv2d_nhwc_f32", x, (w_hi, w_lo), scale, shift, k, stride, residual, relu, out, torch.float32)


def avgpool_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, ..., C] fp32 or bf16 (NHWC map or [N, HW, C] tokens) -> [N, C] fp32, the mean over the middle axes (avf_avgpool_nhwc)"""
    _need_cuda(x, out)
    if not x.is_contiguous():
        raise ValueError("avgpool_nhwc: x must be contiguous")
    N, Cn = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * Cn)
    if out is None:
        out = torch.empty((N, Cn), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, Cn) and out.is_contiguous()
    _lib.check(_lib.load().avf_avgpool_nhwc(_ptr(x), avf_dtype(x.dtype), _ptr(out), N, HW, Cn, _stream()), "avgpool_nhwc")
    return out


# data gradient of the frozen stages (csrc/conv_dgrad.hip; csrc/conv_dgrad_f32.hip: the same kernel in the parity arithmetic) ------
def _conv_pack_dgrad(images: int, w, gamma, running_var, eps):
    """the body of ``conv_pack_weight_dgrad`` (images = 1) and ``conv_pack_weight_dgrad_f32`` (2): the forward pack kernels run on
    the transposed weight with the folded BatchNorm scale multiplied in -> [image [Cin, k*k*Cout], ...]"""
    _need_cuda(w, gamma, running_var)
    w, gamma, var = [t.detach().contiguous() for t in (w, gamma, running_var)]
    assert w.dtype == gamma.dtype == var.dtype == torch.float32 and w.dim() == 4 and w.shape[2] == w.shape[3]
    Cout, Cin = w.shape[:2]
    assert gamma.numel() == var.numel() == Cout
    scale = (gamma.double() / torch.sqrt(var.double() + float(eps))).float()   # what avf_conv_pack_weight folds (fp64 -> fp32)
    wt = (w * scale.view(Cout, 1, 1, 1)).transpose(0, 1).contiguous()          # fp32(w * scale), [Cin, Cout, k, k]
    one, zero = torch.ones(Cin, dtype=torch.float32, device=w.device), torch.zeros(Cin, dtype=torch.float32, device=w.device)
    return _conv_pack(images, wt, one, zero, zero, one, 0.0)[0]


def conv_pack_weight_dgrad(w: torch.Tensor, gamma: torch.Tensor, running_var: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """nn.Conv2d weight [Cout, Cin, k, k] fp32 + the BatchNorm2d behind it -> wt [Cin, k*k*Cout] bf16, the image of
    fp32(w[co, ci, ky, kx] * scale[co]) ordered tap-major / output-channel-minor, one RNE rounding, for ``conv2d_nhwc_dgrad``.
    scale = gamma / sqrt(running_var + eps) as ``conv_pack_weight`` folds it; the shift has no gradient."""
    return _conv_pack_dgrad(1, w, gamma, running_var, eps)[0]


def conv_pack_weight_dgrad_f32(w: torch.Tensor, gamma: torch.Tensor, running_var: torch.Tensor, eps: float = 1e-5):
    """``conv_pack_weight_dgrad`` for ``conv2d_nhwc_dgrad_f32``: -> (wt_hi, wt_lo), the hi / lo split of fp32(w * scale)"""
    return tuple(_conv_pack_dgrad(2, w, gamma, running_var, eps))


def conv_dgrad_plan(N: int, H: int, W: int, Cin: int, Cout: int, k: int, stride: int = 1) -> dict:
    """The tile ``conv2d_nhwc_dgrad`` runs this shape on (avf_conv_dgrad_plan; H, W the INPUT map's): dict(tile = 0 | 1, tile_m,
    tile_n).  Raises on a shape the kernel does not take."""
    out = [C.c_int(-1) for _ in range(3)]
    _lib.check(_lib.load().avf_conv_dgrad_plan(int(N), int(H), int(W), int(Cin), int(Cout), int(k), int(stride), *[C.byref(o) for o in out]),
               "conv_dgrad_plan")
    return dict(tile=out[0].value, tile_m=out[1].value, tile_n=out[2].value)


def _conv2d_dgrad(name: str, gy, ws, in_hw, k, stride, addend, gate, out, out_dtype):
    """the body of ``conv2d_nhwc_dgrad`` (ws = (wt,)) and ``conv2d_nhwc_dgrad_f32`` (ws = (wt_hi, wt_lo); the maps fp32): shapes /
    contiguity / dtypes, allocation, the call"""
    f32 = len(ws) == 2
    _need_cuda(gy, *ws, addend, gate, out)
    N, Ho, Wo, Cout = gy.shape
    H, W = in_hw
    Cin = ws[0].shape[0]
    if (Ho, Wo) != conv_out_hw(H, W, k, stride):
        raise ValueError(f"{name}: a {H} x {W} input map gives a {conv_out_hw(H, W, k, stride)} output at k={k}, stride={stride}; gy is "
                         f"{tuple(gy.shape)}")
    if out is None:
        out = torch.empty((N, H, W, Cin), dtype=torch_dtype(out_dtype), device=gy.device)
    wnames = ("wt_hi", "wt_lo") if f32 else ("wt",)
    for nm, t, shape, dt in ([("gy", gy, (N, Ho, Wo, Cout), torch.float32 if f32 else gy.dtype)] +
                             [(nm, t, (Cin, k * k * Cout), torch.bfloat16) for nm, t in zip(wnames, ws)] +
                             [(nm, t, (N, H, W, Cin), out.dtype) for nm, t in (("addend", addend), ("gate", gate), ("out", out))]):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != dt):
            raise ValueError(f"{name}: {nm} must be a contiguous {shape} {dt} tensor (got {tuple(t.shape)}, strides {t.stride()}, {t.dtype})")
    if f32 and out.dtype != torch.float32:
        raise ValueError(f"{name}: out must be fp32 (got {out.dtype})")
    ptrs, geom = [_ptr(t) for t in (*ws, addend, gate)], (N, H, W, Cin, Cout, _stream())
    if f32:
        rc = _lib.load().avf_conv2d_nhwc_dgrad_f32x3(_ptr(gy), *ptrs, int(k), int(stride), _ptr(out), *geom)
    else:
        rc = _lib.load().avf_conv2d_nhwc_dgrad(_ptr(gy), avf_dtype(gy.dtype), *ptrs, int(k), int(stride), _ptr(out), avf_dtype(out.dtype), *geom)
    _lib.check(rc, name)
    return out


def conv2d_nhwc_dgrad(gy: torch.Tensor, wt: torch.Tensor, in_hw: Tuple[int, int], k: int, stride: int = 1,
                      addend: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      out_dtype=torch.bfloat16) -> torch.Tensor:
    """The gradient of ``conv2d_nhwc`` with respect to its input (avf_conv2d_nhwc_dgrad): gy [N, Ho, Wo, Cout] fp32 or bf16, wt
    from ``conv_pack_weight_dgrad``, ``in_hw`` = (H, W) of the input map -> gate > 0 ? dx + addend : 0, [N, H, W, Cin] fp32 or
    bf16; addend / gate (optional) have out's shape and type.  The weights are frozen: no weight or BatchNorm gradient."""
    return _conv2d_dgrad("conv2d_nhwc_dgrad", gy, (wt,), in_hw, k, stride, addend, gate, out, out_dtype)


def conv2d_nhwc_dgrad_f32(gy: torch.Tensor, wt_split, in_hw: Tuple[int, int], k: int, stride: int = 1,
                          addend: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``conv2d_nhwc_dgrad`` in the parity arithmetic (avf_conv2d_nhwc_dgrad_f32x3): every map fp32, ``wt_split`` = (wt_hi, wt_lo)
    from ``conv_pack_weight_dgrad_f32``, three bf16 MFMA products per fp32 product (bf16x3, oracle/bf16x3.py)."""
    wt_hi, wt_lo = wt_split
    return _conv2d_dgrad("conv2d_nhwc_dgrad_f32", gy, (wt_hi, wt_lo), in_hw, k, stride, addend, gate, out, torch.float32)


def avgpool_nhwc_bwd(dout: torch.Tensor, hw: int, gate: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     out_dtype=torch.bfloat16) -> torch.Tensor:
    """The backward of ``avgpool_nhwc`` behind a ReLU (avf_avgpool_nhwc_bwd): dout [N, C] fp32 -> out[n, p, c] = gate[n, p, c] > 0 ?
    dout[n, c] / hw : 0, [N, hw, C] fp32 or bf16; gate (optional: no gating) is a contiguous [N, ..., C] map of out's type."""
    _need_cuda(dout, gate, out)
    N, Cn = dout.shape
    if out is None:
        out = torch.empty((N, int(hw), Cn), dtype=gate.dtype if gate is not None else torch_dtype(out_dtype), device=dout.device)
    if dout.dtype != torch.float32 or not dout.is_contiguous() or not out.is_contiguous() or out.numel() != N * hw * Cn:
        raise ValueError(f"avgpool_nhwc_bwd: dout must be a contiguous [N, C] fp32 tensor and out a contiguous [N, {hw}, C] one")
    if gate is not None and (gate.dtype != out.dtype or not gate.is_contiguous() or gate.numel() != out.numel()):
        raise ValueError(f"avgpool_nhwc_bwd: gate must be a contiguous {out.dtype} tensor of out's size (got {tuple(gate.shape)}, {gate.dtype})")
    _lib.check(_lib.load().avf_avgpool_nhwc_bwd(_ptr(dout), _ptr(gate), _ptr(out), avf_dtype(out.dtype), N, int(hw), Cn, _stream()),
               "avgpool_nhwc_bwd")
    return out


# frozen ResNet stem (csrc/stem.hip) -------------------------------------------------------------------
STEM_COUT = 64


def stem_packed_k(Cin: int) -> int:
    """row length of ``stem_pack_weight``'s image for ``Cin`` input channels (avf_stem_packed_k); raises unless Cin is 1, 3 or 4"""
    kp = _lib.load().avf_stem_packed_k(int(Cin))
    if kp <= 0:
        _lib.check(1, "stem_packed_k")
    return kp


STEM_POOLS = {"pad1": _lib.STEM_POOL_PAD1, "ceil": _lib.STEM_POOL_CEIL}


def _stem_pool(pool) -> int:
    if pool not in STEM_POOLS:
        raise ValueError(f"pool must be one of {tuple(STEM_POOLS)}, got {pool!r}")
    return STEM_POOLS[pool]


@functools.lru_cache(maxsize=256)
def _stem_out_hw(H: int, W: int, mode: int) -> Tuple[int, int]:
    out = [C.c_int(-1) for _ in range(4)]
    _lib.check(_lib.load().avf_stem_out_hw(H, W, mode, *[C.byref(o) for o in out]), "stem_out_hw")
    return out[2].value, out[3].value


def stem_out_hw(H: int, W: int, pool: str = "pad1") -> Tuple[int, int]:
    """(Hp, Wp) of conv 7x7 / 2 / pad 3 followed by the stem's maxpool: ``pool="pad1"`` 3x3 / 2 / pad 1 (floor), ``pool="ceil"``
    3x3 / 2 / pad 0 with ceil_mode (VGGFace2's ResNet-50; H, W >= 3).  The rule the launch itself acts on (avf_stem_out_hw; the
    answer per (H, W, pool) is kept, so a launch-bound caller pays the host call once)."""
    return _stem_out_hw(int(H), int(W), _stem_pool(pool))


def stem_plan(N: int, Cin: int, H: int, W: int) -> dict:
    """The tile of pooled outputs one workgroup of ``stem_nchw`` owns (avf_stem_plan): dict(tile_h, tile_w).  Raises on a
    shape the kernel does not take."""
    out = [C.c_int(-1) for _ in range(2)]
    _lib.check(_lib.load().avf_stem_plan(int(N), int(Cin), int(H), int(W), *[C.byref(o) for o in out]), "stem_plan")
    return dict(tile_h=out[0].value, tile_w=out[1].value)


def stem_pack_weight(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
                     running_var: torch.Tensor, eps: float = 1e-5):
    """nn.Conv2d weight [64, Cin, 7, 7] fp32 + BatchNorm2d's eval-mode statistics -> (w_packed [64, stem_packed_k(Cin)] bf16 in the
    kernel's own order, scale [64], shift [64] fp32) for ``stem_nchw`` (avf_stem_pack_weight).  Cin in {1, 3, 4}."""
    _need_cuda(w, gamma, beta, running_mean, running_var)
    ts = [t.detach().contiguous() for t in (w, gamma, beta, running_mean, running_var)]
    if not (all(t.dtype == torch.float32 for t in ts) and ts[0].dim() == 4 and tuple(ts[0].shape[2:]) == (7, 7)):
        raise ValueError(f"stem_pack_weight: w must be a [Cout, Cin, 7, 7] fp32 tensor and the BatchNorm tensors fp32 (got {tuple(w.shape)})")
    Cout, Cin = ts[0].shape[:2]
    if not all(t.numel() == Cout for t in ts[1:]):
        raise ValueError(f"stem_pack_weight: the BatchNorm tensors must have Cout = {Cout} elements")
    lib = _lib.load()
    kp = lib.avf_stem_packed_k(int(Cin))  # 0 for a Cin the kernel does not take: the pack call below names the limit
    wp = torch.zeros((Cout, max(kp, 32)), dtype=torch.bfloat16, device=w.device)
    scale = torch.empty(Cout, dtype=torch.float32, device=w.device)
    shift = torch.empty(Cout, dtype=torch.float32, device=w.device)
    _lib.check(lib.avf_stem_pack_weight(*[_ptr(t) for t in ts], float(eps), _ptr(wp), _ptr(scale), _ptr(shift), int(Cout), int(Cin),
                                        _stream()), "stem_pack_weight")
    return wp, scale, shift


def stem_nchw(x: torch.Tensor, w_packed: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, out: Optional[torch.Tensor] = None,
              out_dtype=torch.bfloat16, pool: str = "pad1") -> torch.Tensor:
    """maxpool3x3/2(relu(conv7x7/2(x, w) * scale + shift)) in one launch (avf_stem_nchw_pool): x [N, Cin, H, W] contiguous planes,
    fp32 or bf16, Cin in {1, 3, 4}, any H, W >= 1; w_packed / scale / shift from ``stem_pack_weight``; -> out [N, Hp, Wp, 64] NHWC,
    fp32 or bf16.  ``pool``: ``"pad1"`` (default) pools with padding 1, floor mode; ``"ceil"`` with padding 0 and ceil_mode
    (H, W >= 3), see ``stem_out_hw``.  x may start at any element (a view into a larger buffer); out must be 16-byte aligned.
    Forward only."""
    mode = _stem_pool(pool)
    _need_cuda(x, w_packed, scale, shift, out)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"stem_nchw: x must be a contiguous [N, Cin, H, W] tensor (got {tuple(x.shape)}, strides {x.stride()})")
    N, Cin, H, W = x.shape
    Hp, Wp = _stem_out_hw(H, W, mode)
    if out is None:
        out = torch.empty((N, Hp, Wp, STEM_COUT), dtype=torch_dtype(out_dtype), device=x.device)
    if tuple(out.shape) != (N, Hp, Wp, STEM_COUT) or not out.is_contiguous():
        raise ValueError(f"stem_nchw: out must be a contiguous {(N, Hp, Wp, STEM_COUT)} tensor (got {tuple(out.shape)}, strides {out.stride()})")
    lib = _lib.load()
    kp = lib.avf_stem_packed_k(int(Cin))
    if kp > 0 and (tuple(w_packed.shape) != (STEM_COUT, kp) or not w_packed.is_contiguous()):
        raise ValueError(f"stem_nchw: w_packed must be the contiguous {(STEM_COUT, kp)} image of stem_pack_weight for Cin = {Cin} "
                         f"(got {tuple(w_packed.shape)})")
    for name, t in (("scale", scale), ("shift", shift)):
        if tuple(t.shape) != (STEM_COUT,) or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError(f"stem_nchw: {name} must be a contiguous fp32 [{STEM_COUT}] tensor")
    if w_packed.dtype != torch.bfloat16:
        raise ValueError("stem_nchw: w_packed must be bf16")
    _lib.check(lib.avf_stem_nchw_pool(_ptr(x), avf_dtype(x.dtype), _ptr(w_packed), _ptr(scale), _ptr(shift), _ptr(out),
                                      avf_dtype(out.dtype), N, Cin, H, W, mode, _stream()), "stem_nchw")
    return out


def dropout_factors(seed: int, layer: int, site: int, p: float, rows: int, cols: int, device="cuda") -> torch.Tensor:
    """keep/(1-p) factors of dropout site `site` of layer `layer` for a [rows, cols] activation (test aid)."""
    out = torch.empty((rows, cols), dtype=torch.float32, device=device)
    _lib.check(_lib.load().avf_dropout_factors(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, layer, site, float(p), rows,
                                               cols, _ptr(out), _stream()), "dropout_factors")
    return out


# hardware self-tests -------------------------------------------------------------------------------
def selftest_mfma_bf16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    c = torch.empty((16, 16), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().avf_selftest_mfma_bf16(_ptr(a.contiguous()), _ptr(b.contiguous()), _ptr(c), _stream()), "selftest")
    return c


def selftest_mfma_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    c = torch.empty((16, 16), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().avf_selftest_mfma_f32(_ptr(a.contiguous()), _ptr(b.contiguous()), _ptr(c), _stream()), "selftest")
    return c


def selftest_tr16(tile: torch.Tensor) -> torch.Tensor:
    out = torch.empty((64, 8), dtype=torch.bfloat16, device=tile.device)
    _lib.check(_lib.load().avf_selftest_tr16(_ptr(tile.contiguous()), _ptr(out), _stream()), "selftest")
    return out
