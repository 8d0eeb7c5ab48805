// conv.hip - the frozen ResNet BasicBlock stages around the S-Former's token section (vformer.py:117-166, 232-268), forward only:
//   conv_nhwc_kernel<ConvBf16<XT>>  conv_kernel.hpp's implicit-GEMM convolution with bf16 operands: NHWC activations, bf16 or fp32
//                                   (rounded to bf16 while staged), one bf16 weight image
//   conv_pack_weight_kernel<false>  that image and the folded BatchNorm
//   avgpool_nhwc_kernel             AdaptiveAvgPool2d((1, 1)) + flatten on an NHWC map
// The [B', 49, 256] tokens of the transformer ARE the NHWC map [B', 7, 7, 256]: layer3 writes what the token section reads and
// layer4 reads what it writes, no permute on either side.
// conv_f32.hip instantiates the same kernel with fp32 maps in the bf16x3 parity arithmetic.
#include "conv_kernel.hpp"

namespace avf {
namespace {

// [N, HW, C] -> [N, C]: a thread owns four channels of one image and walks its HW pixels, fp32 sum, one division
template <typename XT>
__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const XT* x, float* out, int64_t N, int HW, int C) {
  const int cq = C / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * cq) return;
  const int64_t n = t / cq;
  const int c = (int)(t - n * cq) * 4;
  const XT* p = x + n * HW * C + c;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = 0; i < HW; ++i) {
    const float4 v = load4<XT>(p + (int64_t)i * C);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float d = (float)HW;
  *reinterpret_cast<float4*>(out + n * C + c) = make_float4(s.x / d, s.y / d, s.z / d, s.w / d);
}

// avf_conv2d_nhwc's part of the launch ladder: the residual's type, then the output's (conv_launch: ReLU, tile)
template <typename XT, int RES>
int conv_launch_out(const ConvArgs& a, int relu, int out_dtype, hipStream_t s) {
  return out_dtype == AVF_F32 ? conv_launch<ConvBf16<XT>, RES, float>("conv2d_nhwc", a, relu, s)
                              : conv_launch<ConvBf16<XT>, RES, bf16>("conv2d_nhwc", a, relu, s);
}
template <typename XT>
int conv_launch_res(const ConvArgs& a, int res, int relu, int out_dtype, hipStream_t s) {
  if (res == 0) return conv_launch_out<XT, 0>(a, relu, out_dtype, s);
  if (res == 1) return conv_launch_out<XT, 1>(a, relu, out_dtype, s);
  return conv_launch_out<XT, 2>(a, relu, out_dtype, s);
}

}  // namespace
}  // namespace avf

using namespace avf;

extern "C" int avf_conv_plan(int N, int H, int W, int Cin, int Cout, int k, int stride, int* tile, int* tile_m, int* tile_n) {
  AVF_REQUIRE(tile && tile_m && tile_n, "conv_plan: null pointer");
  ConvArgs a;
  AVF_TRY(conv_shape("conv_plan", N, H, W, Cin, Cout, k, stride, &a));
  *tile = conv_plan(a);
  *tile_m = kConvTiles[*tile].bm;
  *tile_n = kConvTiles[*tile].bn;
  return 0;
}

extern "C" int avf_conv_pack_weight(const float* w, const float* gamma, const float* beta, const float* running_mean,
                                    const float* running_var, double eps, void* w_packed, float* scale, float* shift, int Cout,
                                    int Cin, int k, void* stream) {
  AVF_REQUIRE(w && gamma && beta && running_mean && running_var && w_packed && scale && shift, "conv_pack_weight: null pointer");
  AVF_REQUIRE(Cout > 0 && Cin > 0 && (k == 1 || k == 3), "conv_pack_weight: Cout=%d Cin=%d k=%d (k: 1 or 3)", Cout, Cin, k);
  AVF_REQUIRE(eps >= 0.0, "conv_pack_weight: eps %g", eps);
  const int64_t n = (int64_t)Cout * k * k * Cin;
  AVF_REQUIRE(apart(w_packed, (size_t)n * 2, w, (size_t)n * 4) && apart(scale, (size_t)Cout * 4, shift, (size_t)Cout * 4),
              "conv_pack_weight: an output overlaps an input or another output");
  conv_pack_weight_kernel<false><<<(unsigned)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(
      w, gamma, beta, running_mean, running_var, eps, (bf16*)w_packed, nullptr, scale, shift, Cout, Cin, k);
  return check_launch("conv_pack_weight");
}

extern "C" int avf_conv2d_nhwc(const void* x, int x_dtype, const void* w_packed, const float* scale, const float* shift,
                               const void* residual, int res_dtype, int relu, int k, int stride, void* out, int out_dtype, int N,
                               int H, int W, int Cin, int Cout, void* stream) {
  ConvArgs a;
  a.x = x; a.w = (const bf16*)w_packed; a.w_lo = nullptr; a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
  AVF_TRY(conv_operands("conv2d_nhwc", &a, 1, x_dtype, res_dtype, out_dtype, N, H, W, Cin, Cout, k, stride));
  const int res = residual ? (res_dtype == AVF_F32 ? 1 : 2) : 0;
  const hipStream_t s = (hipStream_t)stream;
  return x_dtype == AVF_F32 ? conv_launch_res<float>(a, res, relu, out_dtype, s) : conv_launch_res<bf16>(a, res, relu, out_dtype, s);
}

extern "C" int avf_avgpool_nhwc(const void* x, int x_dtype, float* out, int64_t N, int HW, int C, void* stream) {
  AVF_REQUIRE(x && out, "avgpool_nhwc: null pointer");
  AVF_REQUIRE(is_dtype(x_dtype), "avgpool_nhwc: bad dtype %d", x_dtype);
  AVF_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 4 == 0, "avgpool_nhwc: N=%lld HW=%d C=%d (C %% 4 == 0)", (long long)N, HW, C);
  AVF_REQUIRE(aligned(out, 16) && aligned(x, 8), "avgpool_nhwc: x must be 8-byte and out 16-byte aligned");
  AVF_REQUIRE(x_dtype == AVF_BF16 || aligned(x, 16), "avgpool_nhwc: an fp32 x must be 16-byte aligned");
  AVF_REQUIRE(apart(out, (size_t)N * C * 4, x, (size_t)N * HW * C * elt(x_dtype)), "avgpool_nhwc: out overlaps x");
  const unsigned grid = (unsigned)ceil_div(N * (C / 4), 256);
  if (x_dtype == AVF_F32) avgpool_nhwc_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)x, out, N, HW, C);
  else avgpool_nhwc_kernel<bf16><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16*)x, out, N, HW, C);
  return check_launch("avgpool_nhwc");
}
