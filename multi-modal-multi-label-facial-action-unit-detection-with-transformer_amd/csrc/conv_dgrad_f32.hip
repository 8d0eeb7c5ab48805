// conv_dgrad_f32.hip - the parity-mode form of conv_dgrad.hip's data gradient: fp32 NHWC throughout, every fp32 product computed
// as three bf16 MFMA products (bf16x3, as conv_f32.hip does it; oracle/bf16x3.py is the CPU statement):
//   conv_dgrad_nhwc_kernel<ConvBf16x3>  conv_dgrad_kernel.hpp's implicit-GEMM data gradient with both operands split into hi + lo
//                                       bf16 images: gy is split while it is staged, the weight images arrive split
#include "conv_dgrad_kernel.hpp"

using namespace avf;

extern "C" int avf_conv2d_nhwc_dgrad_f32x3(const float* gy, const void* wt_hi, const void* wt_lo, const float* addend, const float* gate,
                                           int k, int stride, float* out, int N, int H, int W, int Cin, int Cout, void* stream) {
  ConvDgradArgs a;
  a.gy = gy; a.w = (const bf16*)wt_hi; a.w_lo = (const bf16*)wt_lo; a.addend = addend; a.gate = gate; a.out = out;
  AVF_TRY(conv_dgrad_operands("conv2d_nhwc_dgrad_f32x3", &a, 2, AVF_F32, AVF_F32, N, H, W, Cin, Cout, k, stride));
  return conv_dgrad_launch<ConvBf16x3, float>("conv2d_nhwc_dgrad_f32x3", a, (hipStream_t)stream);
}
