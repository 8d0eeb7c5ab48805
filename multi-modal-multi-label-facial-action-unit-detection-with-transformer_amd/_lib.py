"""ctypes binding of libavformer_hip.so (the C ABI declared in include/avformer_hip.h).

The product path has NO fallback: if the shared library is missing or cannot be loaded, every
entry point raises.  (The CPU oracle under /oracle is test infrastructure and is never imported
from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import _build, _cabi

_defines, _structs, _functions = _cabi.header()

F32, BF16 = _defines["AVF_F32"], _defines["AVF_BF16"]
EPI_NONE, EPI_BIAS_RES, EPI_BIAS_GELU, EPI_DGELU = (_defines["AVF_EPI_" + n] for n in ("NONE", "BIAS_RES", "BIAS_GELU", "DGELU"))
CLIP_CTHW, CLIP_TCHW = _defines["AVF_CLIP_CTHW"], _defines["AVF_CLIP_TCHW"]
STEM_POOL_PAD1, STEM_POOL_CEIL = _defines["AVF_STEM_POOL_PAD1"], _defines["AVF_STEM_POOL_CEIL"]
EX_CROSS_ENTROPY, EX_FOCAL = _defines["AVF_EX_CROSS_ENTROPY"], _defines["AVF_EX_FOCAL"]
AU_BCE, AU_DICE_BCE = _defines["AVF_AU_BCE"], _defines["AVF_AU_DICE_BCE"]
WAVE_F32, WAVE_I16 = 0, 1  # wave_dtype: the header states it in the comment above avf_mel_power_bank


def _structure(name: str, c_name: str):
    """the ctypes image of one of the header's structs, fields in the header's order (pickles by reference as _lib.<name>)"""
    return type(name, (C.Structure,), {"_fields_": _structs[c_name], "__module__": __name__, "__qualname__": name,
                                       "__doc__": c_name})


LayerCfg = _structure("LayerCfg", "avf_layer_cfg")
LayerPtrs = _structure("LayerPtrs", "avf_layer_params")  # 11 device pointers in state_dict order; avf_layer_grads too:
assert _structs["avf_layer_grads"] == _structs["avf_layer_params"], "avf_layer_grads no longer has avf_layer_params' layout"
TaskLossCfg = _structure("TaskLossCfg", "avf_task_loss_cfg")
EvalCfg = _structure("EvalCfg", "avf_eval_cfg")
PARAM_FIELDS = tuple(n for n, _ in _structs["avf_layer_params"])

# name -> (restype, argtypes) of every entry point, as include/avformer_hip.h declares it (read by _cabi.py, not repeated here)
SIGNATURES = _cabi.bind(_functions, {"avf_layer_cfg": LayerCfg, "avf_layer_params": LayerPtrs, "avf_layer_grads": LayerPtrs,
                                     "avf_task_loss_cfg": TaskLossCfg, "avf_eval_cfg": EvalCfg})

_lock = threading.Lock()
_lib = None


class HipLibraryError(RuntimeError):
    pass


def load(build_if_missing: bool = True):
    """Load (once) and return the ctypes handle.  If the shared library has not been built yet and hipcc is present,
    it is compiled in-tree first (``python __graft_entry__.py`` does the same explicitly).  Raises HipLibraryError
    when neither a built library nor a toolchain is available - there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = _build.lib_path()
        if not os.path.exists(path):
            err = None
            if build_if_missing:
                try:
                    _build.build()
                except Exception as e:  # toolchain missing or compile error: report both facts
                    err = e
            if not os.path.exists(path):
                raise HipLibraryError(
                    f"{path} not found and could not be built ({err}); run python __graft_entry__.py on a machine "
                    f"with hipcc - there is no CPU fallback")
        try:
            lib = C.CDLL(path)
        except OSError as e:  # pragma: no cover - environment dependent
            raise HipLibraryError(f"cannot load {path}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise HipLibraryError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        # a stale .so (or an edited struct) must not be called with structs of another layout
        if lib.avf_sizeof_task_loss_cfg() != C.sizeof(TaskLossCfg):
            raise HipLibraryError(f"{path}: avf_task_loss_cfg is {lib.avf_sizeof_task_loss_cfg()} bytes in the library but "
                                  f"{C.sizeof(TaskLossCfg)} in this binding - rebuild with python __graft_entry__.py")
        if lib.avf_sizeof_eval_cfg() != C.sizeof(EvalCfg):
            raise HipLibraryError(f"{path}: avf_eval_cfg is {lib.avf_sizeof_eval_cfg()} bytes in the library but "
                                  f"{C.sizeof(EvalCfg)} in this binding - rebuild with python __graft_entry__.py")
        if lib.avf_sizeof_layer_cfg() != C.sizeof(LayerCfg) or lib.avf_sizeof_layer_params() != C.sizeof(LayerPtrs):
            raise HipLibraryError(
                f"{path}: avf_layer_cfg / avf_layer_params are {lib.avf_sizeof_layer_cfg()} / "
                f"{lib.avf_sizeof_layer_params()} bytes in the library but {C.sizeof(LayerCfg)} / {C.sizeof(LayerPtrs)} "
                f"in this binding - rebuild with python __graft_entry__.py")
        _lib = lib
    return _lib


# class index -> name: the header states it in the comment above avf_timing_enable
KERNEL_CLASSES = ("gemm_bf16_nt", "gemm_bf16_tn", "gemm_f32", "attn_fwd", "attn_bwd", "layernorm", "other", "gemm_mx8_nt")


def timing_enable(on: bool):
    check(load().avf_timing_enable(int(on)), "timing_enable")


def timing_read():
    """-> {class name: dict(ms, launches, flops, bytes)} for the launches recorded since timing_enable(True)."""
    lib = load()
    out = {}
    for i, name in enumerate(KERNEL_CLASSES):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        check(lib.avf_timing_read(i, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), "timing_read")
        out[name] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
    return out


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().avf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libavformer_hip: {what} failed (rc={rc}): {msg}")


F32_ARITH = {"f32": 0, "bf16x3": 1}  # mode: the header states it in the comment above avf_set_f32_arith


def set_f32_arithmetic(mode: str) -> str:
    """Arithmetic of compute_dtype="f32" GEMMs and attention: "bf16x3" (default: fp32 operands split in
    three bf16 products on the bf16 matrix pipe: <= 3 * 2^-16 = 4.6e-5 relative error per product in the worst case, 4e-6 typical) or "f32" (the f32-input MFMA).
    This is the default of calls that carry no arithmetic of their own: an operator-level call reads it when it is made, a
    Transformer once per forward (its backward runs what that forward ran).  Returns the previous mode's name."""
    if mode not in F32_ARITH:
        raise ValueError(f"set_f32_arithmetic: unknown mode {mode!r}; the accepted modes are {sorted(F32_ARITH)}")
    prev = load().avf_set_f32_arith(F32_ARITH[mode])
    return "bf16x3" if prev else "f32"


def get_f32_arithmetic() -> str:
    return "bf16x3" if load().avf_get_f32_arith() else "f32"
