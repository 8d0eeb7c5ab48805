"""No GPU: the LayerNorm checker of tests/layernorm_util.py is shown to bite.  An honest fp32 emulation of the kernels (fp32
statistics and arithmetic, bf16 on store, partial column sums per block of 16 or 32 rows folded afterwards) goes through
the SAME assertion helpers as tests/test_gpu_layernorm.py and passes on every input family - the fp64 reference alone stays
inside the stated bounds - and emulated mutants, one fault each, fail them for the stated reason."""
import pytest
import torch

import layernorm_util as L

BF = torch.bfloat16
F32 = torch.float32


def _factors(rows, D, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, D, generator=g) >= p).float() / (1.0 - p)


def _run(rows, D, family="general", form="row8", rpb=16, p=0.0, x_dtype=BF, dy_dtype=BF, dres_dtype=BF, y_dtype=BF,
         mutant=None, seed=None):
    inp = L.make_inputs(rows, D, seed if seed is not None else rows * 31 + D, x_dtype, dy_dtype, dres_dtype, family)
    f = _factors(rows, D, p, rows + D) if p else None
    ref = L.reference(inp, f)
    out = L.emulate(inp, f, form, rpb, y_dtype, mutant=mutant)
    what = f"emu[{rows}x{D},{family},{form}]"
    stats = L.check_forward(what, ref, out["y"], out["mean"], out["rstd"])
    stats.update(L.check_backward(what, ref, out["dx"], out["dx_lo"], out["dx_m"], out["dgamma"], out["dbeta"], out["colsum"],
                                  dropout=bool(p)))
    return stats


@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("rows,D,rpb", [(1, 512, 16), (5, 40, 16), (17, 520, 16), (300, 512, 16), (4097, 36, 4), (8193, 1048, 32)])
@pytest.mark.parametrize("form,p", [("row8", 0.0), ("row8", 0.2), ("reg", 0.2)])
def test_honest_emulation_passes(family, rows, D, rpb, form, p):
    _run(rows, D, family, form, rpb, p)


@pytest.mark.parametrize("x_dtype,dy_dtype,dres_dtype,y_dtype", [(F32, F32, F32, F32), (F32, BF, BF, BF), (F32, BF, None, F32),
                                                                  (BF, BF, F32, BF)])
@pytest.mark.parametrize("family", L.FAMILIES)
def test_honest_emulation_passes_every_storage_type(family, x_dtype, dy_dtype, dres_dtype, y_dtype):
    _run(300, 260, family, "reg", 4, 0.2, x_dtype, dy_dtype, dres_dtype, y_dtype)
    _run(33, 1540, family, "reg", 32, 0.0, x_dtype, dy_dtype, dres_dtype, y_dtype)


def test_honest_emulation_passes_at_full_size():
    """rows x D = 10368 x 1536, two batches per wave (32-row partials): the largest shape of the GPU matrix"""
    stats = _run(10368, 1536, "general", "row8", 32, 0.2)
    print(stats)
    for k in ("dgamma", "dbeta", "colsum"):  # honest blocked accumulation does no worse than the sequential baseline
        assert stats[k + "_ratio"] <= stats[k + "_kseq"] + 1.0, stats


# the output(s) whose check has to fire, per mutant
EXPECT = {
    "drop_row_from_sums": r":(dgamma|dbeta|colsum):",
    "last_row_from_previous": r":(y|dx|dx_lo|dx_m):",
    "s1_s2_swapped": r":(dx|dx_lo|dx_m):",
    "bf16_truncation": r":(y|dx_lo|dx_m):.*round-to-nearest",
    "colsum_unmasked": r":colsum:",
    "gamma_chunk0_everywhere": r":(y|dx|dx_lo):",
}


@pytest.mark.parametrize("rows,D,rpb", [(300, 1048, 16), (10368, 520, 32)])
@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_mutant_fails(mutant, rows, D, rpb):
    _run(rows, D, "general", "row8", rpb, 0.2)  # the same case passes without the fault
    with pytest.raises(AssertionError, match=EXPECT[mutant]):
        _run(rows, D, "general", "row8", rpb, 0.2, mutant=mutant)


@pytest.mark.parametrize("mutant", ["drop_row_from_sums", "colsum_unmasked"])
def test_column_sum_mutants_fail_in_each_sum(mutant):
    """not only the first sum that is checked: dgamma, dbeta and colsum are each caught on their own"""
    rows, D = 8748, 512
    inp = L.make_inputs(rows, D, 5, BF, BF, BF)
    f = _factors(rows, D, 0.2, 6)
    ref = L.reference(inp, f)
    out = L.emulate(inp, f, "reg", 16, mutant=mutant)
    for k in ("dgamma", "dbeta", "colsum") if mutant == "drop_row_from_sums" else ("colsum",):
        with pytest.raises(AssertionError, match=k):
            L.check_colsum("emu:" + k, out[k], ref["sums"][k])


def test_masked_image_contract():
    """register form: dx_lo is the masked image; row8 form: dx_lo unmasked, dx_m masked - handing one form's outputs to the
    other form's check fails, and a dropped element that is not exactly 0 fails"""
    rows, D = 33, 40
    inp = L.make_inputs(rows, D, 9, BF, BF, BF)
    f = _factors(rows, D, 0.2, 10)
    ref = L.reference(inp, f)
    r8 = L.emulate(inp, f, "row8", 16)
    rg = L.emulate(inp, f, "reg", 16)
    L.check_backward("c", ref, r8["dx"], r8["dx_lo"], r8["dx_m"], r8["dgamma"], r8["dbeta"], r8["colsum"], True)
    L.check_backward("c", ref, rg["dx"], rg["dx_lo"], None, rg["dgamma"], rg["dbeta"], rg["colsum"], True)
    with pytest.raises(AssertionError, match=":dx_lo:"):
        L.check_backward("c", ref, r8["dx"], r8["dx_lo"], None, r8["dgamma"], r8["dbeta"], r8["colsum"], True)
    with pytest.raises(AssertionError, match=":dx_lo:"):
        L.check_backward("c", ref, rg["dx"], rg["dx_lo"], r8["dx_m"], rg["dgamma"], rg["dbeta"], rg["colsum"], True)
    leaky = r8["dx_m"].clone()
    leaky[ref["f"] == 0] = 1e-30
    with pytest.raises(AssertionError, match="exactly 0"):
        L.check_backward("c", ref, r8["dx"], r8["dx_lo"], leaky, r8["dgamma"], r8["dbeta"], r8["colsum"], True)


def test_nan_and_inf_fail():
    inp = L.make_inputs(5, 40, 1, BF, BF, None, "constant_row")
    ref = L.reference(inp)
    out = L.emulate(inp, None, "row8", 16)
    bad = out["dx_lo"].clone()
    bad[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="finite"):
        L.check_backward("c", ref, out["dx"], bad, None, out["dgamma"], out["dbeta"], out["colsum"], False)
    assert float(ref["rstd"][0]) == pytest.approx(L.EPS ** -0.5)
