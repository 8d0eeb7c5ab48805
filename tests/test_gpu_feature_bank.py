"""-m gpu: avf_feature_clip_tokens (csrc/feature_bank.hip) at the operator level - through the C entry point, with a row stride,
NaN in everything the rule must not read and canary rows around the output - against the torch backend of
``frames.FeatureClipAssembler`` and the numpy restatement of tests/feature_bank_util.py, which test_feature_bank_cpu.py holds to
each other on the CPU.  Every comparison is on bits.  The largest tensor of any case is 2.3 MB."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import avformer_amd as A
from feature_bank_util import GRID, grid_id, make_case, torch_bank, want_tokens

pytestmark = pytest.mark.gpu

FR = A.frames
CANARY = -7.25


def _p(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(case):
    """the inputs of a case on the device, and the restatement's answer (computed once)"""
    c = make_case(case)
    dev = {k: (None if c[k] is None else torch.from_numpy(c[k]).cuda()) for k in ("feat", "black", "video_db_nr", "present", "index", "lead")}
    dev["pos"] = None if c["pos"] is None else torch.from_numpy(np.ascontiguousarray(c["pos"][:c["n_lead"] + c["T"]])).cuda()
    return c, dev, torch.from_numpy(want_tokens(c))


def _call(c, dev, out_t, **over):
    a = dict(feat=_p(dev["feat"]), ldf=c["ldf"], black=_p(dev["black"]), nr=_p(dev["video_db_nr"]), present=_p(dev["present"]),
             index=_p(dev["index"]), F=dev["feat"].shape[0], B=c["B"], T=c["T"], d=c["d"], D=c["D"], lead=_p(dev["lead"]),
             n_lead=c["n_lead"], pos=_p(dev["pos"]), out=_p(out_t))
    a.update(over)
    return A._lib.load().avf_feature_clip_tokens(a["feat"], a["ldf"], a["black"], a["nr"], a["present"], a["index"], a["F"], a["B"], a["T"],
                                                 a["d"], a["D"], a["lead"], a["n_lead"], a["pos"], a["out"], _stream())


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_grid_bit_equal_with_nan_traps_and_canaries(case):
    c, dev, want = _case(case)
    B, R, D = c["B"], c["n_lead"] + c["T"], c["D"]
    assert dev["feat"].stride(0) == c["ldf"] and bool(torch.isnan(dev["feat"][:, D:]).all())
    buf = torch.full((B * R + 2, D), CANARY, device="cuda")
    out = buf[1:-1]
    rc = _call(c, dev, out)
    assert rc == 0, A._lib.load().avf_last_error()
    host = buf.cpu()
    got = host[1:-1].view(B, R, D)
    assert bool(torch.isfinite(got).all())                                      # no absent row, no padding column was used
    assert bool((host[0] == CANARY).all()) and bool((host[-1] == CANARY).all())
    assert torch.equal(_bits(got), _bits(want))
    # the torch backend on the same device, and the module's hip backend with the parameter shapes TFormer holds
    bank, index, lead, pos = torch_bank(c, "cuda")
    lead3, pos3 = None if lead is None else lead[None], None if pos is None else pos[None]
    ref = FR.FeatureClipAssembler(c["T"], c["d"]).tokens(bank, index, lead3, pos3)
    assert torch.equal(_bits(ref.cpu()), _bits(got))
    hip = FR.FeatureClipAssembler(c["T"], c["d"], backend="hip").tokens(bank, index, lead3, pos3)
    assert hip.is_cuda and hip.dtype == torch.float32 and hip.is_contiguous() and tuple(hip.shape) == (B, R, D)
    assert torch.equal(_bits(hip.cpu()), _bits(got))


def test_is_assemble_tokens_on_gathered_rows():
    """bit for bit what avf_assemble_tokens gives on the rows the torch backend gathers"""
    c, dev, want = _case(GRID[0])
    bank, index, lead, pos = torch_bank(c, "cuda")
    rows = FR.FeatureClipAssembler(c["T"], c["d"]).tokens(bank, index)           # no lead, no pos: the gathered rows
    two_step = A.ops.assemble_tokens(rows, lead, pos[:c["n_lead"] + c["T"]])
    assert torch.equal(_bits(two_step.cpu()), _bits(want))


def test_rejected_arguments_name_themselves_and_launch_nothing():
    lib = A._lib.load()
    c, dev, _ = _case(GRID[1])                                                  # D 512, ldf 520, a cls row, pos, present
    B, R, D = c["B"], c["n_lead"] + c["T"], c["D"]
    buf = torch.full((B * R + 2, D), CANARY, device="cuda")
    out = buf[1:-1]
    for over, word in (({"D": 510}, b"D is 510"), ({"D": 0}, b"D is 0"), ({"ldf": D - 4}, b"ldf is 508, below D"),
                       ({"ldf": D + 2}, b"ldf is 514, not a multiple of 4"), ({"T": 0}, b"T is 0"), ({"d": 0}, b"d is 0"),
                       ({"B": 0}, b"B is 0"), ({"F": 0}, b"F is 0"), ({"lead": None}, b"lead is null with n_lead = 1"),
                       ({"n_lead": -1}, b"n_lead is -1"), ({"feat": None}, b"feat is null"), ({"black": None}, b"black is null"),
                       ({"nr": None}, b"video_db_nr is null"), ({"index": None}, b"index is null"), ({"out": None}, b"out is null"),
                       ({"out": _p(out, 4)}, b"out is not 16-byte aligned"), ({"feat": _p(dev["feat"], 8)}, b"feat is not 16-byte aligned"),
                       ({"pos": _p(dev["pos"], 4)}, b"pos is not 16-byte aligned"), ({"black": _p(dev["black"], 4)}, b"black is not 16-byte"),
                       ({"lead": _p(dev["lead"], 12)}, b"lead is not 16-byte aligned"), ({"out": _p(dev["feat"])}, b"out overlaps feat")):
        rc = _call(c, dev, out, **over)
        assert rc != 0 and word in lib.avf_last_error(), (over, lib.avf_last_error())
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    with pytest.raises(RuntimeError, match="D is 6"):                            # ... and through the wrapper the message arrives
        A.ops.feature_clip_tokens(torch.zeros(4, 6, device="cuda"), torch.zeros(6, device="cuda"),
                                  torch.zeros(4, dtype=torch.int32, device="cuda"), None, torch.zeros(1, dtype=torch.int64, device="cuda"), 2, 1)


def test_capture_and_replay_reads_index_at_run_time():
    c, dev, _ = _case(GRID[0])
    bank, index, lead, pos = torch_bank(c, "cuda")
    hip, ref = FR.FeatureClipAssembler(c["T"], c["d"], backend="hip"), FR.FeatureClipAssembler(c["T"], c["d"])
    i0 = index[:8].clone()
    i1 = torch.tensor([27, 0, 39, -1, 13, 30, 7, 26], device="cuda")
    live = i0.clone()
    hip.tokens(bank, live, lead, pos)                                           # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.tokens(bank, live, lead, pos)
    live.copy_(i1)
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    eager = hip.tokens(bank, i1, lead, pos)
    assert torch.equal(_bits(got), _bits(eager)) and torch.equal(_bits(got), _bits(ref.tokens(bank, i1, lead, pos)))
    assert not torch.equal(_bits(got), _bits(ref.tokens(bank, i0, lead, pos)))
