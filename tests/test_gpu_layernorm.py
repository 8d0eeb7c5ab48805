"""-m gpu: every LayerNorm kernel that csrc/layernorm.hip can launch, forward and backward, element by element against the
fp64 reference of tests/layernorm_util.py (bounds and their reasons: that module's docstring; tests/test_layernorm_ref_cpu.py
shows without a device that they bite).  Reached through avf_layernorm_fwd_ex / avf_layernorm_bwd_ex.

host branch (layernorm.hip)                       kernels                                             cases below
bf16 x, D % 8 == 0                                ln_fwd_row8_kernel<1..3,4>, ln_bwd_row8_kernel      ROW8_CASES
                                                  <1,4>/<2,2>/<3,1> and their DROP forms
bf16 x, D % 4 == 0 (D % 8 != 0, fp32 dres, or     ln_fwd_reg_kernel<bf16,NV,false,bf16>,              REG16_CASES, test_row8_switched_off
  AVF_LN_ROW8=0)                                  ln_bwd_reg_kernel<bf16,NV,bf16|float,bf16>
fp32 x, D % 4 == 0, D <= 1536                     ln_fwd_reg_kernel<float|bf16,NV>,                   REG32_CASES
                                                  ln_bwd_reg_kernel<float|bf16,NV,float|bf16>
fp32 x, other D                                   ln_fwd_kernel<float|bf16>, ln_bwd_kernel<T,VEC>     GENERIC_CASES
Rows: both sides of the rows-per-workgroup switches (4096 | 4097: 4 -> 16 rows in the register backward; 8191 | 8192: 16 -> 32
in the row8 backward) and a ragged last workgroup in each regime.  Every case also checks mean / rstd, that a second call
returns the same bits, and one guard row before and after each preallocated output.  Each test prints a line "LNSTAT {json}"
with the measured column-sum ratios (units of 2^-24 T_c) next to k_seq and the share of bf16 elements within 2^-9 |ref|."""
import json
import os
import subprocess
import sys

import pytest
import torch

import layernorm_util as L

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SENTINEL = -24576.0  # exact in bf16
DROP = (0x1234567887654321, 3, 1, 0.2)  # (seed, layer, site, p) as ops.dropout_factors takes them

ROWS_ALL = [1, 3, 4, 5, 15, 16, 17, 33, 300, 4096, 4097, 8191, 8192, 8193, 8748, 10368]
REGIME_ROWS = [300, 4097, 8193]  # one per regime: rows <= 4096, <= 8191, >= 8192 (each with a ragged last workgroup)


def _cases(all_d, both_d):
    """every D at one row count per regime, every row count at the two D of `both_d`"""
    out = [(D, r) for D in all_d for r in REGIME_ROWS]
    out += [(D, r) for D in both_d for r in ROWS_ALL if (D, r) not in out]
    return out


# one lane live; lanes partly live; exactly 1, 2, 3 chunks of 512; a ragged 2nd and 3rd chunk
ROW8_CASES = _cases([8, 40, 512, 520, 1024, 1048, 1536], [512, 40])
# NV = ceil(D / 256) = 1, 2, 3, 4 and 5 / 6 (both take the NV = 6 build)
REG16_CASES = _cases([36, 260, 516, 772, 1028, 1532], [516, 36])
REG32_CASES = _cases([36, 260, 512, 768, 1024, 1532], [512, 260])
# ln_fwd_kernel / ln_bwd_kernel: VEC false / true; 32 rows per workgroup
GENERIC_CASES = [(D, r) for D in (34, 1540) for r in (1, 5, 31, 32, 33, 300, 4097, 8193)]

# backward options per family: (dy, dres, y) storage types, which outputs are requested, dropout.  A case runs the two
# variants of its parity, so every option meets every D and every row count.
V = lambda dy, dres, y, dx, lo, m, cs, p: dict(dy=dy, dres=dres, y=y, dx=dx, lo=lo, m=m, cs=cs, p=p)
ROW8_VARIANTS = [[V(BF, BF, BF, False, True, False, True, 0.0), V(BF, None, BF, True, True, True, False, 0.2)],
                 [V(BF, BF, BF, True, True, True, True, 0.2), V(BF, None, BF, False, True, False, False, 0.0)]]
REG16_VARIANTS = [[V(BF, BF, BF, False, True, False, True, 0.0), V(BF, F32, BF, True, True, False, True, 0.2)],
                  [V(BF, None, BF, True, False, False, False, 0.0), V(BF, None, BF, False, True, False, True, 0.2)]]
REG32_VARIANTS = [[V(F32, F32, F32, True, True, False, True, 0.2), V(BF, BF, BF, False, True, False, True, 0.0)],
                  [V(BF, None, F32, True, False, False, False, 0.0), V(BF, F32, BF, True, True, False, True, 0.2)]]
GENERIC_VARIANTS = [[V(F32, F32, F32, True, True, False, True, 0.0), V(BF, None, BF, True, False, False, False, 0.0)],
                    [V(BF, F32, F32, True, True, False, False, 0.0), V(F32, None, BF, True, False, False, True, 0.0)]]


@pytest.fixture(scope="module")
def ops():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A.ops


def _guarded(rows, D, dtype):
    buf = torch.full((rows + 2, D), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[1:rows + 1]


def _guards_intact(what, buf):
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), what + ": a write outside the output"


def _cpu(t):
    return None if t is None else t.cpu()


def run_case(ops, kernel, D, rows, x_dtype, v, family="general"):
    # ln_bwd_kernel (the general form) adds its four waves' terms into LDS with atomics: its sums promise no fixed order
    fixed_order = kernel != "generic"
    what = f"{kernel}[{rows}x{D},{family},dy={str(v['dy'])[6:]},dres={str(v['dres'])[6:]},p={v['p']}]"
    inp = L.make_inputs(rows, D, rows * 4099 + D * 7 + int(v["p"] * 10), x_dtype, v["dy"], v["dres"], family)
    drop = DROP if v["p"] else None
    f = ops.dropout_factors(*DROP[:3], v["p"], rows, D).cpu() if drop else None
    ref = L.reference(inp, f)
    dev = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in inp.items()}
    ybuf, yview = _guarded(rows, D, v["y"])
    y, mean, rstd = ops.layernorm_fwd_ex(dev["x"], dev["gamma"], dev["beta"], L.EPS, y=yview)
    _guards_intact(what + ":y", ybuf)
    stats = L.check_forward(what, ref, y.cpu(), mean.cpu(), rstd.cpu())

    def bwd():
        lo = _guarded(rows, D, BF) if v["lo"] else (None, None)
        m = _guarded(rows, D, BF) if v["m"] else (None, None)
        out = ops.layernorm_bwd_ex(dev["dy"], dev["x"], dev["gamma"], mean, rstd, dres=dev["dres"], want_dx=v["dx"],
                                   want_colsum=v["cs"], drop=drop, dx_lo=lo[1], dx_m=m[1])
        for name, (buf, _) in (("dx_lo", lo), ("dx_m", m)):
            if buf is not None:
                _guards_intact(f"{what}:{name}", buf)
        return out

    first, second = bwd(), bwd()
    for name, a, b in zip(("dx", "dx_lo", "dx_m", "dgamma", "dbeta", "colsum"), first, second):
        if fixed_order or name in ("dx", "dx_lo", "dx_m"):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"{what}:{name}: a second call differs"
    dx, dx_lo, dx_m, dg, db, cs = (_cpu(t) for t in first)
    assert (dx is not None) == v["dx"] and (dx_lo is not None) == v["lo"] and (dx_m is not None) == v["m"]
    stats.update(L.check_backward(what, ref, dx, dx_lo, dx_m, dg, db, cs, dropout=bool(v["p"])))
    regime = "<=4096" if rows <= 4096 else ("<=8191" if rows <= 8191 else ">=8192")
    print("LNSTAT " + json.dumps(dict(kernel=kernel, rows=rows, D=D, regime=regime, family=family, p=v["p"], **stats)))
    return stats


def _both(ops, kernel, D, rows, x_dtype, variants, cases):
    for v in variants[cases.index((D, rows)) % 2]:
        run_case(ops, kernel, D, rows, x_dtype, v)


@pytest.mark.parametrize("D,rows", ROW8_CASES)
def test_row8(ops, D, rows):
    _both(ops, "row8", D, rows, BF, ROW8_VARIANTS, ROW8_CASES)


@pytest.mark.parametrize("D,rows", REG16_CASES)
def test_reg_bf16_x(ops, D, rows):
    _both(ops, "reg_bf16x", D, rows, BF, REG16_VARIANTS, REG16_CASES)


@pytest.mark.parametrize("D,rows", [(512, 300), (1048, 4097), (1536, 8193), (40, 17)])
def test_reg_bf16_x_fp32_dres_at_row8_widths(ops, D, rows):
    """D % 8 == 0 with an fp32 residual gradient: the host leaves the row8 form for ln_bwd_reg_kernel<bf16,NV,float,bf16>"""
    run_case(ops, "reg_bf16x", D, rows, BF, V(BF, F32, BF, True, True, False, True, 0.2))
    run_case(ops, "reg_bf16x", D, rows, BF, V(BF, F32, BF, False, True, False, True, 0.0))


@pytest.mark.parametrize("D,rows", REG32_CASES)
def test_reg_fp32_x(ops, D, rows):
    _both(ops, "reg_fp32x", D, rows, F32, REG32_VARIANTS, REG32_CASES)


@pytest.mark.parametrize("D,rows", GENERIC_CASES)
def test_generic_fp32_x(ops, D, rows):
    _both(ops, "generic", D, rows, F32, GENERIC_VARIANTS, GENERIC_CASES)


@pytest.mark.parametrize("family", ["constant_row", "large_offset"])
@pytest.mark.parametrize("kernel,x_dtype,D,rows,v", [
    ("row8", BF, 520, 33, ROW8_VARIANTS[1][0]), ("row8", BF, 1048, 8193, ROW8_VARIANTS[0][0]),
    ("reg_bf16x", BF, 260, 300, REG16_VARIANTS[0][1]), ("reg_fp32x", F32, 768, 4097, REG32_VARIANTS[0][0]),
    ("reg_fp32x", F32, 512, 17, REG32_VARIANTS[0][1]), ("generic", F32, 34, 33, GENERIC_VARIANTS[0][0]),
    ("generic", F32, 1540, 5, GENERIC_VARIANTS[1][0])])
def test_special_rows(ops, family, kernel, x_dtype, D, rows, v):
    """a constant row (variance 0: rstd = eps^-1/2) and |x| ~ 1e3 with a small variance: everything finite and inside the bounds
    widened per row by max(1, rstd |mean|)"""
    run_case(ops, kernel, D, rows, x_dtype, v, family)


def test_refusals(ops):
    """invalid combinations come back as an error that names the reason; nothing is launched (the outputs keep their fill)"""
    rows = 8
    g = lambda D: (torch.ones(D, device="cuda"), torch.zeros(D, device="cuda"))
    x16 = lambda D: torch.ones(rows, D, dtype=BF, device="cuda")
    stat = torch.zeros(rows, device="cuda")
    y = torch.full((rows, 1544), SENTINEL, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="dim <= 1536"):
        ops.layernorm_fwd_ex(x16(1544), *g(1544), y=y)
    y32 = torch.full((rows, 512), SENTINEL, dtype=F32, device="cuda")
    with pytest.raises(RuntimeError, match="a bf16 input needs a bf16 output"):
        ops.layernorm_fwd_ex(x16(512), *g(512), y=y32)
    lo = torch.full((rows, 1544), SENTINEL, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="dim <= 1536"):
        ops.layernorm_bwd_ex(x16(1544), x16(1544), g(1544)[0], stat, stat, dx_lo=lo)
    lo5 = torch.full((rows, 512), SENTINEL, dtype=BF, device="cuda")
    m5 = torch.full((rows, 512), SENTINEL, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="a bf16 residual gradient needs bf16 dy"):
        ops.layernorm_bwd_ex(x16(512).float(), x16(512).float(), g(512)[0], stat, stat, dres=x16(512), dx_lo=lo5)
    with pytest.raises(RuntimeError, match="a separate masked image needs live dropout"):
        ops.layernorm_bwd_ex(x16(512), x16(512), g(512)[0], stat, stat, dres=x16(512), dx_lo=lo5, dx_m=m5)
    with pytest.raises(RuntimeError, match="needs the fp32 dx"):
        lo34 = torch.full((rows, 34), SENTINEL, dtype=BF, device="cuda")
        ops.layernorm_bwd_ex(torch.ones(rows, 34, device="cuda"), torch.ones(rows, 34, device="cuda"), g(34)[0], stat, stat,
                             want_dx=False, dx_lo=lo34)
    with pytest.raises(RuntimeError, match="bad dropout"):
        ops.layernorm_bwd_ex(x16(512), x16(512), g(512)[0], stat, stat, dx_lo=lo5, drop=(1, 0, 3, 0.2))
    torch.cuda.synchronize()
    for t in (y, y32, lo, lo5, m5):
        assert bool((t == SENTINEL).all())


_CHILD = r'''
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import avformer_amd as A
import test_gpu_layernorm as T
V = T.V
for D, rows in [(512, 300), (40, 4097), (1048, 8193), (1536, 33), (1024, 8192)]:
    # all-bf16 streams at D %% 8 == 0, which the parent process runs on the row8 kernels
    T.run_case(A.ops, "reg_bf16x(row8 off)", D, rows, T.BF, V(T.BF, T.BF, T.BF, False, True, False, True, 0.0))
    T.run_case(A.ops, "reg_bf16x(row8 off)", D, rows, T.BF, V(T.BF, None, T.BF, True, True, False, True, 0.2))
# a separate masked image still takes the row8 DROP form (layernorm.hip: ln_row8_on() || dx_m)
T.run_case(A.ops, "row8(row8 off)", 520, 300, T.BF, V(T.BF, T.BF, T.BF, True, True, True, True, 0.2))
print("ROW8_OFF_OK")
'''


def test_row8_switched_off():
    """AVF_LN_ROW8=0 (read once per process, and only under AVF_TUNING=1): the all-bf16 cases at D % 8 == 0 on the register kernels -
    one child process, one time limit"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, AVF_TUNING="1", AVF_LN_ROW8="0"), timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "ROW8_OFF_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
