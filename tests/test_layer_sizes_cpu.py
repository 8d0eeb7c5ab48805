"""CPU (no GPU needed): the sizes and the byte layout of a layer's buffers are pinned, as literal numbers recorded
from the build BEFORE the layer orchestration was regrouped around one description per Linear.  One change since: the
workspace's `delta` block holds B*H*N floats, not twice that (its second half was scratch of the retired head-resident
attention backward), so every workspace size and every workspace offset behind `delta` went down by
align256(8 B H N) - align256(4 B H N), and nothing else moved.

- The size queries (host code) for one configuration per layer mode: a changed alignment, piece size or workspace
  maximum shows here.  They cannot see equal-sized pieces changing places.
- The grouped weight-gradient workspace of 1..4 layers, at shapes where the group splits its token reduction.
- The offset of every piece inside the lowp, saved, workspace and deferred-dW buffers: a stand-alone host program
  (tests/layer_layout_main.hip) includes layer.hip, carves each buffer and prints the offsets; they are compared
  with tests/golden/layer_layout.txt.  The Adam kernels find the bf16 weight images by their offsets in the lowp
  buffer, and the MX-FP8 images keep theirs too.

``python tests/test_layer_sizes_cpu.py`` prints the size table of the library that ``AVF_LIB_PATH`` (or the tree) holds."""
import ctypes
import os
import subprocess
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import avformer_amd as A

BF16, F32 = A._lib.BF16, A._lib.F32
MASK = 256  # a non-null key_mask: the size queries never dereference it


def _cfg(batch, tokens, dim, heads, dim_head, mlp, dtype, p=0.0, project_out=1, **flags):
    c = A._lib.LayerCfg(batch, tokens, dim, heads, dim_head, mlp, dtype, project_out, 1e-5, p)
    for k, v in flags.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


# name -> cfg.  Unless noted: B=2, N=100, dim 128, 2 heads x 64, mlp 256
CONFIGS = {
    "f32": lambda: _cfg(2, 100, 128, 2, 64, 256, F32),
    "f32_drop": lambda: _cfg(2, 100, 128, 2, 64, 256, F32, 0.1),
    "bf16_gs16": lambda: _cfg(2, 100, 128, 2, 64, 256, BF16, grad_stream_bf16=1),
    "bf16_drop_f32stream": lambda: _cfg(2, 100, 128, 2, 64, 256, BF16, 0.1),
    "bf16_resid16": lambda: _cfg(2, 100, 128, 2, 64, 256, BF16, grad_stream_bf16=1, resid_bf16=1),
    "bf16_resid16_drop": lambda: _cfg(2, 100, 128, 2, 64, 256, BF16, 0.1, grad_stream_bf16=1, resid_bf16=1),
    "mx8_fwd": lambda: _cfg(2, 64, 512, 8, 64, 1024, BF16, grad_stream_bf16=1, mx8_fwd=1),
    "mx8": lambda: _cfg(2, 64, 512, 8, 64, 1024, BF16, grad_stream_bf16=1, mx8_fwd=1, mx8_bwd=1, dx_out_mx8=1),
    "mask_bf16": lambda: _cfg(2, 100, 128, 2, 64, 256, BF16, grad_stream_bf16=1, key_mask=MASK),
    "mask_bf16_4x32": lambda: _cfg(2, 100, 128, 4, 32, 256, BF16, grad_stream_bf16=1, key_mask=MASK),
    "small_n12": lambda: _cfg(2, 12, 128, 4, 32, 256, BF16, grad_stream_bf16=1),
    "deferred_128rows": lambda: _cfg(2, 64, 128, 2, 64, 256, BF16, grad_stream_bf16=1, resid_bf16=1),
    "deferred_16384rows": lambda: _cfg(32, 512, 512, 8, 64, 1024, BF16, grad_stream_bf16=1, resid_bf16=1),
    "identity_to_out": lambda: _cfg(2, 100, 64, 1, 64, 256, BF16, 0.1, project_out=0),
    "identity_to_out_f32": lambda: _cfg(2, 100, 64, 1, 64, 256, F32, 0.1, project_out=0),
    "ws_k512": lambda: _cfg(2, 64, 512, 8, 64, 1024, BF16, grad_stream_bf16=1, resid_bf16=1),
}
QUERIES = ("avf_layer_saved_bytes", "avf_layer_lowp_bytes", "avf_layer_workspace_bytes", "avf_layer_grad_stream_bytes",
           "avf_layer_dw_block_bytes")

# (saved, lowp, workspace, grad_stream, dw_block, layers_dw_workspace of 1 layer, ... of 4 layers)
EXPECTED = {
    "f32": (1132288, 0, 1055488, 51200, 0, 0, 0),
    "f32_drop": (1132288, 0, 1260288, 51200, 0, 0, 0),
    "bf16_gs16": (620288, 524288, 810752, 51200, 604160, 0, 0),
    "bf16_drop_f32stream": (620288, 524288, 810752, 51200, 0, 0, 0),
    "bf16_resid16": (569088, 524288, 810752, 51200, 604160, 0, 0),
    "bf16_resid16_drop": (569088, 524288, 913152, 102400, 0, 0, 0),
    "mx8_fwd": (1579008, 17432576, 2355200, 131072, 0, 0, 0),
    "mx8": (1579008, 17432576, 2828288, 198656, 0, 0, 0),
    "mask_bf16": (620288, 524288, 810752, 51200, 0, 0, 0),
    "mask_bf16_4x32": (621824, 524288, 812288, 51200, 0, 0, 0),
    "small_n12": (75264, 524288, 113152, 6144, 0, 0, 0),
    "deferred_128rows": (363520, 524288, 521216, 32768, 389120, 0, 0),
    "deferred_16384rows": (185335808, 13107200, 234389504, 16777216, 132153344, 33554432, 0),
    "identity_to_out": (414720, 196608, 464384, 25600, 0, 0, 0),
    "identity_to_out_f32": (773120, 0, 734720, 25600, 0, 0, 0),
    "ws_k512": (1447936, 13107200, 2084864, 131072, 1556480, 0, 0),
}


def measure(lib, name):
    cfg = CONFIGS[name]()
    out = [getattr(lib, q)(ctypes.byref(cfg)) for q in QUERIES]
    for n in (1, 4):
        arr = (A._lib.LayerCfg * n)(*[CONFIGS[name]() for _ in range(n)])
        out.append(lib.avf_layers_dw_workspace_bytes(arr, n))
    return tuple(int(v) for v in out)


@pytest.fixture(scope="module")
def lib():
    A._build.build()
    return A._lib.load()


def test_every_mode_is_listed():
    assert set(EXPECTED) == set(CONFIGS)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_layer_buffer_sizes_are_pinned(lib, name):
    got = measure(lib, name)
    assert got[0] > 0, lib.avf_last_error()  # the configuration itself is valid
    assert got == EXPECTED[name]


# avf_layers_dw_workspace_bytes of n = 1..4 bf16 layers (all-bf16 streams) at shapes whose group needs split-K scratch
DW_GROUP_WS = {
    (8, 512, 128, 2, 64, 256): (4194304, 8388608, 12582912, 16777216),
    (64, 512, 256, 4, 64, 512): (16777216, 33554432, 31457280, 33554432),
    (32, 512, 512, 8, 64, 1024): (33554432, 33554432, 100663296, 0),  # four layers fill one round of the chip: no split
}


@pytest.mark.parametrize("shape", sorted(DW_GROUP_WS))
def test_grouped_dw_workspace_is_pinned(lib, shape):
    got = []
    for n in (1, 2, 3, 4):
        arr = (A._lib.LayerCfg * n)(*[_cfg(*shape, BF16, grad_stream_bf16=1, resid_bf16=1) for _ in range(n)])
        got.append(int(lib.avf_layers_dw_workspace_bytes(arr, n)))
    assert tuple(got) == DW_GROUP_WS[shape]


def test_layer_buffer_layout_is_pinned(lib, tmp_path):
    """every piece of every buffer sits at its recorded offset (see the module docstring)"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "layer_layout")
    so = A._build.lib_path()
    cmd = [A._build._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", f"-DAVF_OUT_WT={A._build.out_wt()}", "-I", A._build.CSRC,
           os.path.join(here, "layer_layout_main.hip"), "-o", exe, "-L", os.path.dirname(so), "-l:" + os.path.basename(so),
           f"-Wl,-rpath,{os.path.dirname(so)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    want = open(os.path.join(here, "golden", "layer_layout.txt")).read().splitlines()
    assert len(want) > 400 and not any(line.endswith("invalid") for line in got)
    assert [g for g, w in zip(got, want) if g != w] == [] and len(got) == len(want)


if __name__ == "__main__":
    handle = A._lib.load()
    for key in CONFIGS:
        print(f'    "{key}": {measure(handle, key)},')
