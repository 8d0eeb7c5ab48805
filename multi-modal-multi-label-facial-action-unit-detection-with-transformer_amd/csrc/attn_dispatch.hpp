// attn_dispatch.hpp - the run-time -> compile-time steps the attention entry points share (attn_f32, attn_f32_mfma, attn_bf16,
// attn_bwd_merged): the dim_head sets the three kernel families are instantiated for and a bool.  As in gemm_dispatch.hpp a
// helper hands a generic lambda an int_c / std::bool_constant, and the instantiations of a kernel template are exactly the
// calls its entry point makes through them.  Host code only.
#pragma once
#include "common.hpp"

namespace avf {

// f(std::true_type{}) / f(std::false_type{})
template <typename F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(int_c<DH>{}) for the fp32-arithmetic VALU kernels (attn_f32.hip)
template <typename F>
int with_vec_dim_head(int dh, F&& f) {
  switch (dh) {
    case 8: return f(int_c<8>{});
    case 16: return f(int_c<16>{});
    case 32: return f(int_c<32>{});
    case 64: return f(int_c<64>{});
    case 128: return f(int_c<128>{});
    default: AVF_REQUIRE(false, "attention (fp32): unsupported dim_head %d (8,16,32,64,128)", dh);
  }
}

// f(int_c<DH>{}) for the kernels on the fp32 matrix pipe (attn_f32_mfma.hip; attn_f32_mfma_ok lets nothing else through)
template <typename F>
int with_mfma_dim_head(int dh, const char* who, F&& f) {
  switch (dh) {
    case 32: return f(int_c<32>{});
    case 64: return f(int_c<64>{});
    case 128: return f(int_c<128>{});
    default: AVF_REQUIRE(false, "%s: unsupported dim_head %d (32, 64 or 128)", who, dh);
  }
}

// f(int_c<DH>{}, int_c<NW>{}) for the streaming bf16 kernels (attn_bf16.hip): NW waves per workgroup, 8 at dim_head 128
template <typename F>
int with_stream_dim_head(int dh, F&& f) {
  switch (dh) {
    case 32: return f(int_c<32>{}, int_c<4>{});
    case 64: return f(int_c<64>{}, int_c<4>{});
    case 128: return f(int_c<128>{}, int_c<8>{});
    default: AVF_REQUIRE(false, "attention (bf16): unsupported dim_head %d (32, 64 or 128)", dh);
  }
}

}  // namespace avf
