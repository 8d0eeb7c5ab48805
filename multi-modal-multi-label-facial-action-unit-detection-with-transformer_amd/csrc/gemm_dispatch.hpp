// gemm_dispatch.hpp - host-side plumbing shared by the entry points of the four GEMM families (gemm_bf16_nt, gemm_bf16_nt_ws,
// gemm_mx8_nt, gemm_f32): the run-time -> compile-time step of the epilogue and of C's type, the check of what an epilogue
// reads beside C, and the split-K plan.  Host code only.
#pragma once
#include "common.hpp"

namespace avf {

// f(int_c<AVF_EPI_*>{}) for the epilogue `epi`.  f is a generic lambda; the instantiations of a kernel template are exactly the
// calls its entry point makes through this (a form a family does not have sits behind an `if constexpr` in f).
template <typename F>
int with_epilogue(int epi, const char* who, F&& f) {
  switch (epi) {
    case AVF_EPI_NONE: return f(int_c<AVF_EPI_NONE>{});
    case AVF_EPI_BIAS_RES: return f(int_c<AVF_EPI_BIAS_RES>{});
    case AVF_EPI_BIAS_GELU: return f(int_c<AVF_EPI_BIAS_GELU>{});
    case AVF_EPI_DGELU: return f(int_c<AVF_EPI_DGELU>{});
    default: AVF_REQUIRE(false, "%s: bad epilogue %d", who, epi);
  }
}
// f(T{}) with T = float / bf16 for C's storage type; decltype of the argument is the type
template <typename F>
int with_c_type(int c_dtype, const char* who, F&& f) {
  if (c_dtype == AVF_F32) return f(float{});
  AVF_REQUIRE(c_dtype == AVF_BF16, "%s: bad c_dtype", who);
  return f(bf16{});
}

// What the epilogue reads or writes beside C, refused before anything is enqueued: BIAS_RES needs the residual, BIAS_GELU and
// DGELU the saved pre-activation `aux`; ld_multiple > 0 (the NT families: 4) also binds their leading dimensions.
inline int require_epilogue_operands(const GemmArgs& a, const char* who, int ld_multiple) {
  const bool aux = a.epilogue == AVF_EPI_BIAS_GELU || a.epilogue == AVF_EPI_DGELU;
  AVF_REQUIRE(a.epilogue != AVF_EPI_BIAS_RES || a.residual, "%s: BIAS_RES needs a residual (in C's storage type)", who);
  AVF_REQUIRE(!aux || a.aux, "%s: BIAS_GELU / DGELU need aux, the saved pre-activation (in C's type)", who);
  AVF_REQUIRE(ld_multiple <= 0 || ((a.epilogue != AVF_EPI_BIAS_RES || a.ldres % ld_multiple == 0) && (!aux || a.ldaux % ld_multiple == 0)),
              "%s: ldres / ldaux must be a multiple of %d", who, ld_multiple);
  return 0;
}

// split-K: `wanted` splits of a reduction of K, each a whole number of K-steps of `step`; S = the splits that are not empty
struct SplitPlan {
  int S, kchunk;
};
inline SplitPlan split_plan(int64_t K, int64_t wanted, int step) {
  const int64_t kchunk = ceil_div(ceil_div(K, wanted), step) * step;
  return {(int)ceil_div(K, kchunk), (int)kchunk};
}

}  // namespace avf
