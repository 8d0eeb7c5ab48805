"""CPU (no GPU needed): the C-ABI shared library builds, loads and exports exactly the symbols that
include/avformer_hip.h declares; the binding that `_cabi` derives from the header agrees with what the C compiler makes of
it (struct layouts, constants), the reader refuses what it does not understand, and a few signatures are pinned literally;
size queries (pure host code) behave; the Python host side mirrors the reference's parameter schema; the product path fails
loudly without a GPU."""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import pytest
import torch

import avformer_amd as A
from conftest import load_golden, split_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTURES = {"avf_layer_cfg": "LayerCfg", "avf_layer_params": "LayerPtrs", "avf_layer_grads": "LayerPtrs",
              "avf_task_loss_cfg": "TaskLossCfg", "avf_eval_cfg": "EvalCfg"}
# Python name -> the macro or enumerator it is read from
CONSTANTS = {(A._lib, "F32"): "AVF_F32", (A._lib, "BF16"): "AVF_BF16", (A._lib, "EPI_NONE"): "AVF_EPI_NONE",
             (A._lib, "EPI_BIAS_RES"): "AVF_EPI_BIAS_RES", (A._lib, "EPI_BIAS_GELU"): "AVF_EPI_BIAS_GELU",
             (A._lib, "EPI_DGELU"): "AVF_EPI_DGELU", (A._lib, "CLIP_CTHW"): "AVF_CLIP_CTHW", (A._lib, "CLIP_TCHW"): "AVF_CLIP_TCHW",
             (A._lib, "STEM_POOL_PAD1"): "AVF_STEM_POOL_PAD1", (A._lib, "STEM_POOL_CEIL"): "AVF_STEM_POOL_CEIL",
             (A._lib, "EX_CROSS_ENTROPY"): "AVF_EX_CROSS_ENTROPY", (A._lib, "EX_FOCAL"): "AVF_EX_FOCAL",
             (A._lib, "AU_BCE"): "AVF_AU_BCE", (A._lib, "AU_DICE_BCE"): "AVF_AU_DICE_BCE",
             (A.ops, "ATTN_MERGED"): "AVF_ATTN_MERGED", (A.metrics, "STATE_WORDS"): "AVF_EVAL_STATE_WORDS",
             (A.metrics, "EX_CONF"): "AVF_EVAL_EX_CONF", (A.metrics, "AU_STATS"): "AVF_EVAL_AU_STATS",
             (A.metrics, "VA_MOMENTS"): "AVF_EVAL_VA_MOMENTS", (A.metrics, "LOSS_SUM"): "AVF_EVAL_LOSS_SUM",
             (A.metrics, "LOSS_STEPS"): "AVF_EVAL_LOSS_STEPS"}
ATTN_KINDS = {"res8": "AVF_ATTN_RES8", "res12": "AVF_ATTN_RES12", "res_multi": "AVF_ATTN_RES_MULTI", "stream": "AVF_ATTN_STREAM",
              "f32": "AVF_ATTN_F32"}


@pytest.fixture(scope="module")
def lib():
    A._build.build()
    return A._lib.load()


def _exported_symbols(path):
    """names of the defined dynamic symbols of a shared library, by whichever binutil is there"""
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(A._build._hipcc()))), "lib", "llvm", "bin", "llvm-readelf")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert os.path.exists(llvm), f"neither nm nor {llvm}: cannot list the exports of {path}"
    out = subprocess.run([llvm, "--dyn-syms", "-W", path], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]
    return {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}


def test_exports_are_exactly_the_header_s_entry_points(lib):
    exported = {s for s in _exported_symbols(A._build.lib_path()) if s.startswith("avf_")}
    assert exported == set(A._lib.SIGNATURES), exported ^ set(A._lib.SIGNATURES)
    assert len(exported) > 100
    for name in exported:
        assert hasattr(lib, name), name
    assert lib.avf_version() == 1
    # the binding's struct declarations match the compiled header
    assert lib.avf_sizeof_layer_cfg() == ctypes.sizeof(A._lib.LayerCfg)
    assert lib.avf_sizeof_layer_params() == ctypes.sizeof(A._lib.LayerPtrs)


@pytest.fixture(scope="module")
def compiler_view(tmp_path_factory):
    """what the host C++ compiler makes of the header: {"sizeof S": n, "S.f": (offset, size), "AVF_X": value}, printed by a
    generated probe that names every struct, field and constant the reader found"""
    defines, structs, _ = A._cabi.header()
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "avformer_hip.h"', "int main() {"]
    for s, fields in structs.items():
        lines.append(f'  std::printf("sizeof {s} %zu\\n", sizeof({s}));')
        lines += [f'  std::printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f, _ in fields]
    lines += [f'  std::printf("{d} %lld\\n", (long long)({d}));' for d in defines]
    tmp = tmp_path_factory.mktemp("abi_probe")
    src, exe = str(tmp / "probe.cpp"), str(tmp / "probe")
    with open(src, "w") as f:
        f.write("\n".join(lines + ["  return 0;", "}", ""]))
    r = subprocess.run([A._build._hipcc(), "-x", "c++", "-std=c++17", "-I", os.path.dirname(A._build.ABI_HEADER), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    view = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *nums = line.rsplit(" ", 2) if "." in line else line.rsplit(" ", 1)
        view[key] = tuple(map(int, nums)) if len(nums) > 1 else int(nums[0])
    return view


def test_struct_layouts_match_the_compiler(compiler_view):
    _, structs, _ = A._cabi.header()
    assert set(structs) == set(STRUCTURES)
    for s, fields in structs.items():
        cls = getattr(A._lib, STRUCTURES[s])
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields]
        assert ctypes.sizeof(cls) == compiler_view[f"sizeof {s}"], s
        for f, _ in fields:
            d = getattr(cls, f)
            assert (d.offset, d.size) == compiler_view[f"{s}.{f}"], (s, f)
    # ... and they cover the struct: no field of the header is missing between two that were read
    for s, fields in structs.items():
        ends = sorted((o, o + n) for o, n in (compiler_view[f"{s}.{f}"] for f, _ in fields))
        assert ends[0][0] == 0 and all(b[0] - a[1] in range(8) for a, b in zip(ends, ends[1:])), s
        assert compiler_view[f"sizeof {s}"] - ends[-1][1] in range(8), s


def test_constants_match_the_compiler(compiler_view):
    for (mod, name), macro in CONSTANTS.items():
        assert getattr(mod, name) == compiler_view[macro], (name, macro)
    assert A.ops.ATTN_KINDS == {compiler_view[macro]: kind for kind, macro in ATTN_KINDS.items()}
    assert A._lib.TaskLossCfg.ex_weight.size == 4 * compiler_view["AVF_TASK_LOSS_EX_CLASSES"]
    assert A._lib.TaskLossCfg.pos_weight.size == 4 * compiler_view["AVF_TASK_LOSS_AU_UNITS"]


def test_pinned_signatures():
    """literal rows: a reader bug that shifts every row alike would pass the checks above"""
    S, L = A._lib.SIGNATURES, A._lib
    res, args = S["avf_gemm_mx8_nt_ex"]
    assert res is c_int and len(args) == 28 and args[20] is c_uint32 and args[21] is c_uint32 and args[24] is c_float
    assert args[:5] == [c_int64, c_int64, c_int64, c_void_p, c_int64] and args[22] is c_int and args[25:] == [c_void_p] * 3
    res, args = S["avf_mel_db_norm"]
    assert res is c_int and len(args) == 10 and args[6:9] == [c_double] * 3 and args[9] is c_void_p and args[2] is c_int64
    assert S["avf_layer_fwd"] == (c_int, [POINTER(L.LayerCfg), POINTER(L.LayerPtrs)] + [c_void_p] * 6)
    assert S["avf_layer_bwd"][1][11] is POINTER(L.LayerPtrs)  # const avf_layer_grads*
    assert S["avf_task_loss"][1][7] is POINTER(L.TaskLossCfg) and S["avf_eval_scores"][1][1] is POINTER(L.EvalCfg)
    assert S["avf_last_error"] == (c_char_p, [])
    assert S["avf_clip_autoaugment_max_pixels"] == (c_int64, [])
    assert S["avf_layer_workspace_bytes"] == (c_size_t, [POINTER(L.LayerCfg)])
    assert S["avf_layers_dw"] == (c_int, [POINTER(L.LayerCfg), c_int, c_void_p, c_void_p, c_size_t, c_void_p])
    assert S["avf_crash_line_arm"] == (c_int, [c_char_p, c_int])
    assert L.PARAM_FIELDS == ("ln1_w", "ln1_b", "w_qkv", "w_out", "b_out", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")
    assert L.LayerCfg.__module__ == L.__name__ and L.LayerCfg.__qualname__ == "LayerCfg"


MINIATURE = """/* a header with one of each form the reader takes; avf_not_code(int) in a comment is not code */
#ifndef MINI_H
#define MINI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define AVF_N 3      /* a length */
#define AVF_HEX 0x10
enum { AVF_A = 0, AVF_B = 5 };
typedef struct avf_pair {
  int32_t a, b;   // two declarators
  const float *p, *q;
  float w[AVF_N];
  double d[2];
  uint32_t u;
  int64_t big;
} avf_pair;
int avf_none(void);
const char* avf_text(void);
size_t avf_bytes(const avf_pair* cfg, int n);
int64_t avf_call(const void* const* rows, float* const* out, int32_t* plan, uint8_t* bytes, const char* line, float x,
                 double y, uint32_t lo, size_t n, int64_t m, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def _parse(tmp_path, text):
    path = tmp_path / "mini.h"
    path.write_text(text)
    return A._cabi.parse(str(path))


def test_reader_parses_every_supported_form(tmp_path):
    defines, structs, functions = _parse(tmp_path, MINIATURE)
    assert defines == {"AVF_N": 3, "AVF_HEX": 16, "AVF_A": 0, "AVF_B": 5}
    assert structs == {"avf_pair": [("a", c_int32), ("b", c_int32), ("p", c_void_p), ("q", c_void_p), ("w", c_float * 3),
                                    ("d", c_double * 2), ("u", c_uint32), ("big", c_int64)]}
    assert functions == {"avf_none": (c_int, []), "avf_text": (c_char_p, []), "avf_bytes": (c_size_t, ["avf_pair", c_int]),
                         "avf_call": (c_int64, [c_void_p, c_void_p, c_void_p, c_void_p, c_char_p, c_float, c_double, c_uint32,
                                                c_size_t, c_int64, c_void_p])}
    Pair = type("Pair", (ctypes.Structure,), {"_fields_": structs["avf_pair"]})
    assert A._cabi.bind(functions, {"avf_pair": Pair})["avf_bytes"] == (c_size_t, [POINTER(Pair), c_int])


@pytest.mark.parametrize("declaration, named", [
    ("int avf_f(long double x);", "long double"),                         # an unknown type
    ("int avf_f(wchar_t* s);", "wchar_t"),                                # ... also behind a pointer
    ("int avf_f(const float*, int n);", "avf_f"),                         # a parameter without a name
    ("int avf_f(int);", "avf_f"),
    ("int avf_f(void (*done)(int), int n);", "avf_f"),                    # a function pointer
    ("typedef struct avf_s { int32_t flag : 1; } avf_s;", "flag : 1"),     # a bit-field
    ("typedef struct avf_s { struct { int32_t a; } in; } avf_s;", "avf_s"),  # a nested struct
    ("typedef struct avf_s { union avf_u v; } avf_s;", "union"),          # a union
    ("typedef struct avf_s { float w[AVF_MISSING]; } avf_s;", "AVF_MISSING"),
    ("AVF_EXPORT(int) avf_f(int n);", "avf_f"),                           # an entry point behind a macro
    ("int AVF_NAME(avf_f)(int n);", "avf_f"),
    ("AVF_API int avf_f(int n);", "AVF_API"),
    ("#define AVF_SQUARE(x) ((x) * (x))", "AVF_SQUARE"),
    ("#define AVF_RATE 0.5", "AVF_RATE"),
    ("#if AVF_WIDE\nint avf_f(int n);\n#endif", "#if"),
    ("enum { AVF_A, AVF_B };", "AVF_A"),
    ("void avf_f(int n);", "void"),
    ("int avf_none(void);", "avf_none"),                                  # declared twice
])
def test_reader_refuses_what_it_does_not_understand(tmp_path, declaration, named):
    with pytest.raises(A._cabi.HeaderError) as e:
        _parse(tmp_path, MINIATURE.replace("int avf_none(void);", "int avf_none(void);\n" + declaration))
    assert named in str(e.value), str(e.value)


def test_size_queries_and_config_validation(lib):
    cfg = A._lib.LayerCfg(32, 512, 512, 8, 64, 1024, A._lib.BF16, 1, 1e-5, 0.0)
    saved = lib.avf_layer_saved_bytes(ctypes.byref(cfg))
    R = 32 * 512
    # bf16: h1,h2 (D) + qkv (3I) + o (I) + u,g (M) at 2 B, x_mid fp32, 4 stats vectors + lse
    expect = R * 2 * (512 * 2 + 1536 + 512 + 2 * 1024) + R * 512 * 4 + 4 * R * 4 + 32 * 8 * 512 * 4
    assert expect <= saved <= expect + 64 * 256
    assert lib.avf_layer_lowp_bytes(ctypes.byref(cfg)) >= 2 * 2 * (1536 * 512 + 512 * 512 + 2 * 512 * 1024)
    assert lib.avf_layer_workspace_bytes(ctypes.byref(cfg)) > 0
    cfg32 = A._lib.LayerCfg(4, 64, 128, 8, 32, 256, A._lib.F32, 1, 1e-5, 0.0)
    assert lib.avf_layer_lowp_bytes(ctypes.byref(cfg32)) == 0
    bad = A._lib.LayerCfg(4, 64, 128, 8, 48, 256, A._lib.BF16, 1, 1e-5, 0.0)
    assert lib.avf_layer_saved_bytes(ctypes.byref(bad)) == 0
    assert b"dim_head" in lib.avf_last_error()
    drop = A._lib.LayerCfg(4, 64, 128, 8, 32, 256, A._lib.F32, 1, 1e-5, 0.2)  # fp32 mode with live dropout (round 2)
    assert lib.avf_layer_saved_bytes(ctypes.byref(drop)) > 0
    nodrop = A._lib.LayerCfg(4, 64, 128, 8, 32, 256, A._lib.F32, 1, 1e-5, 0.0)
    # ... which needs two fp32 masked gradient copies in the workspace
    assert lib.avf_layer_workspace_bytes(ctypes.byref(drop)) >= lib.avf_layer_workspace_bytes(ctypes.byref(nodrop)) + 2 * 256 * 128 * 4
    bad_drop = A._lib.LayerCfg(4, 64, 130, 8, 32, 256, A._lib.F32, 1, 1e-5, 0.2)  # dropout needs dim % 4 == 0
    assert lib.avf_layer_saved_bytes(ctypes.byref(bad_drop)) == 0
    assert b"dropout" in lib.avf_last_error()
    assert lib.avf_gemm_workspace_bytes(A._lib.BF16, 1, 0, 1536, 512, 16384) > 0
    # fp32: split-K slabs of the weight-gradient shapes (round 5; optional - without a workspace avf_gemm runs unsplit) and of
    # skinny shapes; nothing for a shape whose tiles already fill the chip
    assert lib.avf_gemm_workspace_bytes(A._lib.F32, 1, 0, 1536, 512, 16384) % (1536 * 512 * 4) == 0
    assert lib.avf_gemm_workspace_bytes(A._lib.F32, 1, 0, 1536, 512, 16384) > 0
    assert lib.avf_gemm_workspace_bytes(A._lib.F32, 0, 1, 16384, 1536, 512) == 0


def test_state_dict_schema_matches_reference_fixture():
    p, _, r = split_golden(load_golden("g3_transformer_c1"))
    t = A.Transformer(r["dim"], r["depth"], r["heads"], r["dim_head"], r["mlp_dim"])
    sd = t.state_dict()
    assert list(sd.keys()) == list(p.keys())
    assert all(sd[k].shape == p[k].shape for k in p)
    t.load_state_dict(p, strict=True)


def test_same_seed_same_init_as_reference_fixture():
    """the holders are built in the reference's RNG order: seeding like make_golden.py reproduces its weights"""
    p, _, r = split_golden(load_golden("g3_transformer_c1"))
    torch.manual_seed(1003)
    t = A.Transformer(r["dim"], r["depth"], r["heads"], r["dim_head"], r["mlp_dim"])
    for k, v in t.state_dict().items():
        assert torch.equal(v, p[k]), k


def test_head_schemas_match_reference_fixtures():
    for name, mod in (("g5_au_former", A.AU_former(input_dim=64, emb_dim=32)),
                      ("g6_au_head", A.tformer_AU_head(emb_dim=64)),
                      ("g15_va_former_eval", A.VA_former(input_dim=64, emb_dim=128)),
                      ("g7_tformer", A.TFormer(16, 64, 2, 8, 128, 32))):
        p, _, _ = split_golden(load_golden(name))
        ref_keys = [k for k, v in p.items()]
        assert list(mod.state_dict().keys()) == ref_keys, name


def test_no_cpu_fallback():
    t = A.Transformer(32, 1, 8, 32, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t(torch.randn(1, 4, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.AULoss()(torch.zeros(2, 12), torch.zeros(2, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ops.layernorm_fwd(torch.zeros(2, 8), torch.ones(8), torch.zeros(8))


def test_dropout_configuration():
    t = A.Transformer(32, 1, 8, 32, 64, dropout=0.2, compute_dtype="f32")
    t.train()
    assert abs(t._cfg(1, 4).dropout_p - 0.2) < 1e-7  # live in both modes since round 2
    t.eval()
    assert t._cfg(1, 4).dropout_p == 0.0
    t = A.Transformer(32, 1, 8, 32, 64, dropout=0.2)  # bf16: dropout is live in train(), identity in eval()
    t.train()
    seed_t = torch.zeros(1, dtype=torch.int64)
    c = t._cfg(1, 4, layer=3, seed_t=seed_t)
    assert abs(c.dropout_p - 0.2) < 1e-7 and c.layer_index == 3 and c.seed_dev == seed_t.data_ptr()
    s1 = t._advance_seed(torch.device("cpu"))
    s2 = t._advance_seed(torch.device("cpu"))
    assert int(s2) == int(s1) + 1 and t.last_seed == int(s2) & 0xFFFFFFFFFFFFFFFF
    t.eval()
    assert t._cfg(1, 4, seed_t=seed_t).dropout_p == 0.0 and t._advance_seed(torch.device("cpu")) is None


def test_registry_has_the_former_entries_of_train_py():
    """train.py:292-303: avformer / vformer / tformer / sformer resolve; constructor kwargs, .modes, .task and the
    reference's parameter names (checkpoints load with strict=False) are in place - no GPU needed to construct"""
    for name in ("sformer", "vformer", "tformer"):
        m = A.models.build_model(name, modality="A;V;M", task="AU")
        assert m.modes == ["clip"] and m.task == "AU"
        assert hasattr(m, "get_au_loss") and hasattr(m, "get_ex_loss") and hasattr(m, "get_va_loss")
    sd = A.models.build_model("sformer").state_dict()
    assert "base_model.pos_embedding" in sd and "base_model.spatial_transformer.layers.0.0.fn.fn.to_qkv.weight" in sd
    assert "au_head.AU_linear_p1.weight" in sd and "fc.1.weight" in sd
    sd = A.models.build_model("tformer").state_dict()
    assert "video_model.s_former.pos_embedding" in sd and "video_model.t_former.cls_token" in sd
    assert sd["video_model.t_former.pos_embedding"].shape == (1, 17, 1536) and "au_head.AU_linear_last12.weight" in sd
    sd = A.models.build_model("vformer").state_dict()
    assert sd["video_model.t_former.pos_embedding"].shape == (1, 17, 512) and sd["fc.3.weight"].shape == (21, 256)
    with pytest.raises(KeyError):
        A.models.build_model("emonet")


def test_registry():
    assert "avformer" in A.MODEL_REGISTRY
    m = A.build_model("avformer", modality="A;V;M", task="AU")
    assert m.modes == ['clip', 'audio_features'] and m.task == "AU"
    with pytest.raises(KeyError):
        A.build_model("resnet")
