// conv_f32.hip - the parity-mode form of conv.hip's convolution: fp32 NHWC in, fp32 NHWC out, every fp32 product computed as
// three bf16 MFMA products ("bf16x3", as gemm_f32.hip and attn_f32x3.hip do it; oracle/bf16x3.py is the CPU statement):
//   conv_nhwc_kernel<ConvBf16x3>   conv_kernel.hpp's implicit-GEMM convolution with both operands split into hi + lo bf16 images
//   conv_pack_weight_kernel<true>  the two weight images (hi, lo) and the folded BatchNorm
// The split:  hi = bf16(v) (round to nearest even),  lo = bf16(v - hi) (v - hi is exact in fp32);
//   x w ~ hi_w lo_x + lo_w hi_x + hi_w hi_x  (each bf16 x bf16 product is exact in fp32; lo_w lo_x, <= 2^-16 |x w|, is not computed).
// The activations are split while they are staged (a thread's eight fp32 channels -> one 16-byte piece of each image), the weights
// arrive split.  This is the conv's ONE parity arithmetic: there is no plain-fp32 (VALU) form.
#include "conv_kernel.hpp"

using namespace avf;

extern "C" int avf_conv_pack_weight_f32x3(const float* w, const float* gamma, const float* beta, const float* running_mean,
                                          const float* running_var, double eps, void* w_hi, void* w_lo, float* scale, float* shift,
                                          int Cout, int Cin, int k, void* stream) {
  AVF_REQUIRE(w && gamma && beta && running_mean && running_var && w_hi && w_lo && scale && shift, "conv_pack_weight_f32x3: null pointer");
  AVF_REQUIRE(Cout > 0 && Cin > 0 && (k == 1 || k == 3), "conv_pack_weight_f32x3: Cout=%d Cin=%d k=%d (k: 1 or 3)", Cout, Cin, k);
  AVF_REQUIRE(eps >= 0.0, "conv_pack_weight_f32x3: eps %g", eps);
  const int64_t n = (int64_t)Cout * k * k * Cin;
  AVF_REQUIRE(apart(w_hi, (size_t)n * 2, w, (size_t)n * 4) && apart(w_lo, (size_t)n * 2, w, (size_t)n * 4) &&
                  apart(w_hi, (size_t)n * 2, w_lo, (size_t)n * 2) && apart(scale, (size_t)Cout * 4, shift, (size_t)Cout * 4),
              "conv_pack_weight_f32x3: an output overlaps an input or another output");
  conv_pack_weight_kernel<true><<<(unsigned)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(
      w, gamma, beta, running_mean, running_var, eps, (bf16*)w_hi, (bf16*)w_lo, scale, shift, Cout, Cin, k);
  return check_launch("conv_pack_weight_f32x3");
}

extern "C" int avf_conv2d_nhwc_f32x3(const float* x, const void* w_hi, const void* w_lo, const float* scale, const float* shift,
                                     const float* residual, int relu, int k, int stride, float* out, int N, int H, int W, int Cin,
                                     int Cout, void* stream) {
  ConvArgs a;
  a.x = x; a.w = (const bf16*)w_hi; a.w_lo = (const bf16*)w_lo; a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
  AVF_TRY(conv_operands("conv2d_nhwc_f32x3", &a, 2, AVF_F32, AVF_F32, AVF_F32, N, H, W, Cin, Cout, k, stride));
  const hipStream_t s = (hipStream_t)stream;
  return residual ? conv_launch<ConvBf16x3, 1, float>("conv2d_nhwc_f32x3", a, relu, s)
                  : conv_launch<ConvBf16x3, 0, float>("conv2d_nhwc_f32x3", a, relu, s);
}
