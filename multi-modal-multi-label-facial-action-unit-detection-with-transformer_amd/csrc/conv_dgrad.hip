// conv_dgrad.hip - the backward of the frozen layer4 behind the S-Former's token section (vformer.py:244-265): the gradient reaches
// pos_embedding and spatial_transformer only through layer4's convolutions and avgpool.  The stage's weights are frozen, so this
// is data gradients only:
//   conv_dgrad_nhwc_kernel<ConvBf16<XT>>  conv_dgrad_kernel.hpp's implicit-GEMM data gradient with bf16 operands: gy bf16 or fp32
//                                         (rounded to bf16 while staged), one bf16 weight image
//   avgpool_nhwc_bwd_kernel               the backward of avgpool_nhwc_kernel, with the last block's ReLU gate
// conv_dgrad_f32.hip instantiates the same kernel with fp32 maps in the bf16x3 parity arithmetic.
#include "conv_dgrad_kernel.hpp"

namespace avf {
namespace {

// [N, C] -> [N, HW, C]: a thread owns eight channels of one pixel
template <typename OT, bool GATE>
__global__ __launch_bounds__(256) void avgpool_nhwc_bwd_kernel(const float* dout, const OT* gate, OT* out, int64_t N, int HW, int C) {
  const int c8 = C / 8;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * HW * c8) return;
  const int64_t px = t / c8;
  const int c = (int)(t - px * c8) * 8;
  const int64_t n = px / HW, o = px * C + c;
  float v[8];
  load8f(dout + n * C + c, v);
  const float d = (float)HW;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = v[e] / d;
  if constexpr (GATE) {
    float g[8];
    if constexpr (std::is_same<OT, float>::value) load8f(gate + o, g);
    else unpack8(*reinterpret_cast<const uint4*>(gate + o), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = g[e] > 0.f ? v[e] : 0.f;
  }
  if constexpr (std::is_same<OT, float>::value) {
    *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(out + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    *reinterpret_cast<uint4*>(out + o) = pack8(v);
  }
}

template <typename OT>
int avgpool_bwd_launch(const float* dout, const void* gate, void* out, int64_t N, int HW, int C, hipStream_t s) {
  const unsigned grid = (unsigned)ceil_div(N * HW * (C / 8), 256);
  if (gate) avgpool_nhwc_bwd_kernel<OT, true><<<grid, 256, 0, s>>>(dout, (const OT*)gate, (OT*)out, N, HW, C);
  else avgpool_nhwc_bwd_kernel<OT, false><<<grid, 256, 0, s>>>(dout, nullptr, (OT*)out, N, HW, C);
  return check_launch("avgpool_nhwc_bwd");
}

// avf_conv2d_nhwc_dgrad's part of the launch ladder: the output's type (conv_dgrad_launch: addend, gate, tile)
template <typename XT>
int conv_dgrad_launch_out(const ConvDgradArgs& a, int out_dtype, hipStream_t s) {
  return out_dtype == AVF_F32 ? conv_dgrad_launch<ConvBf16<XT>, float>("conv2d_nhwc_dgrad", a, s)
                              : conv_dgrad_launch<ConvBf16<XT>, bf16>("conv2d_nhwc_dgrad", a, s);
}

}  // namespace
}  // namespace avf

using namespace avf;

extern "C" int avf_conv_dgrad_plan(int N, int H, int W, int Cin, int Cout, int k, int stride, int* tile, int* tile_m, int* tile_n) {
  AVF_REQUIRE(tile && tile_m && tile_n, "conv_dgrad_plan: null pointer");
  ConvDgradArgs a;
  AVF_TRY(conv_dgrad_shape("conv_dgrad_plan", N, H, W, Cin, Cout, k, stride, &a));
  *tile = conv_dgrad_plan(a);
  *tile_m = kConvTiles[*tile].bm;
  *tile_n = kConvTiles[*tile].bn;
  return 0;
}

extern "C" int avf_conv2d_nhwc_dgrad(const void* gy, int gy_dtype, const void* wt_packed, const void* addend, const void* gate, int k,
                                     int stride, void* out, int out_dtype, int N, int H, int W, int Cin, int Cout, void* stream) {
  ConvDgradArgs a;
  a.gy = gy; a.w = (const bf16*)wt_packed; a.w_lo = nullptr; a.addend = addend; a.gate = gate; a.out = out;
  AVF_TRY(conv_dgrad_operands("conv2d_nhwc_dgrad", &a, 1, gy_dtype, out_dtype, N, H, W, Cin, Cout, k, stride));
  const hipStream_t s = (hipStream_t)stream;
  return gy_dtype == AVF_F32 ? conv_dgrad_launch_out<float>(a, out_dtype, s) : conv_dgrad_launch_out<bf16>(a, out_dtype, s);
}

extern "C" int avf_avgpool_nhwc_bwd(const float* dout, const void* gate, void* out, int out_dtype, int64_t N, int HW, int C, void* stream) {
  AVF_REQUIRE(dout && out, "avgpool_nhwc_bwd: null pointer");
  AVF_REQUIRE(is_dtype(out_dtype), "avgpool_nhwc_bwd: bad dtype %d", out_dtype);
  AVF_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 8 == 0, "avgpool_nhwc_bwd: N=%lld HW=%d C=%d (C %% 8 == 0)", (long long)N, HW, C);
  AVF_REQUIRE(N * HW * (C / 8) < (1ll << 39), "avgpool_nhwc_bwd: too many pixels");
  AVF_REQUIRE(aligned(dout, 16) && aligned(out, 16) && aligned(gate, 16), "avgpool_nhwc_bwd: every operand must be 16-byte aligned");
  const size_t on = (size_t)N * HW * C * elt(out_dtype);
  AVF_REQUIRE(apart(out, on, dout, (size_t)N * C * 4) && (!gate || apart(out, on, gate, on)), "avgpool_nhwc_bwd: out overlaps an input");
  const hipStream_t s = (hipStream_t)stream;
  return out_dtype == AVF_F32 ? avgpool_bwd_launch<float>(dout, gate, out, N, HW, C, s) : avgpool_bwd_launch<bf16>(dout, gate, out, N, HW, C, s);
}
