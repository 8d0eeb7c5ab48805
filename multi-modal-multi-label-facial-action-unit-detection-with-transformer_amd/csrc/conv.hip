// conv.hip - the frozen ResNet BasicBlock stages around the S-Former's token section (vformer.py:117-166, 232-268), forward only:
//   conv_nhwc_bf16_kernel    3x3 (pad 1) / 1x1 (pad 0) convolution, stride 1 / 2, as an implicit GEMM on v_mfma_f32_16x16x32_bf16,
//                            NHWC activations, with the folded eval-mode BatchNorm, the identity add and the ReLU in its epilogue
//   avgpool_nhwc_kernel      AdaptiveAvgPool2d((1, 1)) + flatten on an NHWC map
//   conv_pack_weight_kernel  nn.Conv2d's [Cout, Cin, kh, kw] fp32 weight -> [Cout, kh, kw, Cin] bf16, BatchNorm2d's running
//                            statistics -> one (scale, shift) pair per channel
// The [B', 49, 256] tokens of the transformer ARE the NHWC map [B', 7, 7, 256]: layer3 writes what the token section reads and
// layer4 reads what it writes, no permute on either side.
//
// GEMM view: rows = the N*Ho*Wo output pixels, columns = Cout, reduction = kh*kw*Cin ordered tap-major / channel-minor, so a
// 32-deep chunk of one pixel is 32 consecutive channels of ONE tap: in range (two or four 16-byte loads) or padding (zeros
// written to LDS by index - no load is issued, nothing outside the input is read).
// The argument block, the LDS swizzle, the shape rules and the tile dispatch are conv_common.hpp, shared with conv_f32.hip (the
// same convolution with fp32 maps in the bf16x3 parity arithmetic).
#include "conv_common.hpp"

namespace avf {
namespace {

// 8 consecutive channels as they come from memory: kept raw until they are written to LDS, so that the wait for the load
// sits behind the MFMAs of the chunk before (the one stage of look-ahead)
template <typename T>
struct Raw8;
template <>
struct Raw8<bf16> {
  uint4 v;
  __device__ __forceinline__ void load(const bf16* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void zero() { v = make_uint4(0u, 0u, 0u, 0u); }
  __device__ __forceinline__ uint4 packed() const { return v; }
};
template <>
struct Raw8<float> {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ __forceinline__ void zero() { a = b = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ uint4 packed() const {  // RNE, as a bf16 activation would have been stored
    return make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
  }
};

// Tile BM pixels x BN channels.  The weights are the MFMA's A operand and the pixels its B operand, so a lane's four accumulator
// registers are four consecutive CHANNELS of one pixel; tile row f * 16 + q * 4 + r of the weight image holds channel
// (f / 2) * 32 + q * 8 + (f % 2) * 4 + r, which makes the registers of fragments 2j and 2j + 1 eight consecutive channels:
// one 16-byte store per lane for bf16, two for fp32.
// RES: 0 none, 1 fp32, 2 bf16.
template <typename XT, int RES, bool RELU, typename OT, int BM, int BN>
__global__ __launch_bounds__(kConvThreads) void conv_nhwc_bf16_kernel(const ConvArgs a) {
  constexpr int FM = BM / 64, FN = BN / 16, AP = BM * 4 / kConvThreads;
  static_assert(BM % 64 == 0 && BN % 32 == 0 && BN * 4 <= kConvThreads, "tile");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][(BM + BN) * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const XT* x = reinterpret_cast<const XT*>(a.x);

  // staging: thread -> tile row(s) tid / 4 (+ 64), piece tid % 4.  (n, oy, ox) of a row is decoded here, once.
  const int piece = tid & 3;
  int iy0[AP], ix0[AP];
  int64_t img[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int64_t m = m0 + (tid >> 2) + i * 64;
    const bool valid = m < a.M;
    const int64_t n = valid ? m / (a.Ho * a.Wo) : 0;
    const int r = valid ? (int)(m - n * (a.Ho * a.Wo)) : 0;
    const int oy = r / a.Wo, ox = r - oy * a.Wo;
    iy0[i] = valid ? oy * a.stride - a.pad : -(1 << 24);  // a row past M: every tap is padding
    ix0[i] = ox * a.stride - a.pad;
    img[i] = n * a.H;
  }
  const int wr = tid >> 2;  // weight tile row (threads below BN * 4)
  const int wch = n0 + (wr >> 5) * 32 + ((wr >> 2) & 3) * 8 + ((wr >> 4) & 1) * 4 + (wr & 3);
  const bool wvalid = tid < BN * 4 && wch < a.Cout;
  const bf16* wrow = a.w + (int64_t)(wvalid ? wch : 0) * a.K + piece * 8;

  const int cpt = a.Cin / kConvBK;  // chunks per tap
  const int nc = a.k * a.k * cpt;
  Raw8<XT> ra[AP];
  uint4 rb;
  auto fetch = [&](int c) {
    const int tap = c / cpt, c0 = (c - tap * cpt) * kConvBK + piece * 8;
    const int ky = tap / a.k, kx = tap - ky * a.k;
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int iy = iy0[i] + ky, ix = ix0[i] + kx;
      if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ra[i].load(x + ((img[i] + iy) * a.W + ix) * a.Cin + c0);
      else ra[i].zero();
    }
    if (wvalid) rb = *reinterpret_cast<const uint4*>(wrow + (int64_t)c * kConvBK);
    else rb = make_uint4(0u, 0u, 0u, 0u);
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AP; ++i) *reinterpret_cast<uint4*>(&lds[buf][conv_lds_off((tid >> 2) + i * 64, piece)]) = ra[i].packed();
    if (tid < BN * 4) *reinterpret_cast<uint4*>(&lds[buf][BM * 64 + conv_lds_off(wr, piece)]) = rb;
  };

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const int buf = c & 1;
    if (c + 1 < nc) fetch(c + 1);
    bf16x8_t pf[FM], wf[FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
      pf[i] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][conv_lds_off(wave * (BM / 4) + i * 16 + (lane & 15), lane >> 4)]);
#pragma unroll
    for (int j = 0; j < FN; ++j)
      wf[j] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][BM * 64 + conv_lds_off(j * 16 + (lane & 15), lane >> 4)]);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], pf[i], acc[i][j], 0, 0, 0);
    // the other buffer was last read in the iteration before, which every wave left through the barrier below
    if (c + 1 < nc) stash(buf ^ 1);
    __syncthreads();
  }

  // epilogue: y = acc * scale[c] + shift[c] (the folded BatchNorm), + identity, ReLU, store
  OT* out = reinterpret_cast<OT*>(a.out);
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int64_t m = m0 + wave * (BM / 4) + i * 16 + (lane & 15);
    if (m >= a.M) continue;
#pragma unroll
    for (int j = 0; j < FN / 2; ++j) {
      const int ch = n0 + j * 32 + (lane >> 4) * 8;
      if (ch >= a.Cout) continue;  // Cout % 16 == 0: eight channels are inside or outside together
      float v[8], sc[8], sh[8];
      load8f(a.scale + ch, sc);
      load8f(a.shift + ch, sh);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = acc[i][2 * j][e] * sc[e] + sh[e];
        v[4 + e] = acc[i][2 * j + 1][e] * sc[4 + e] + sh[4 + e];
      }
      const int64_t o = m * a.Cout + ch;
      if constexpr (RES != 0) {
        float r[8];
        if constexpr (RES == 1) load8f(reinterpret_cast<const float*>(a.res) + o, r);
        else unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(a.res) + o), r);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += r[e];
      }
      if constexpr (RELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];  // (a NaN stays a NaN)
      }
      if constexpr (std::is_same<OT, float>::value) {
        *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(out + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
      } else {
        *reinterpret_cast<uint4*>(out + o) = pack8(v);
      }
    }
  }
}

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

// one thread per packed element; the first Cout threads also fold their channel's BatchNorm in fp64
__global__ __launch_bounds__(256) void conv_pack_weight_kernel(const float* w, const float* gamma, const float* beta, const float* mean,
                                                               const float* var, double eps, bf16* wp, float* scale, float* shift,
                                                               int Cout, int Cin, int k) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t K = (int64_t)k * k * Cin;
  if (idx >= Cout * K) return;
  const int64_t co = idx / K;
  const int r = (int)(idx - co * K);
  const int tap = r / Cin, ci = r - tap * Cin;
  const int ky = tap / k, kx = tap - ky * k;
  wp[idx] = from_f32<bf16>(w[((co * Cin + ci) * k + ky) * k + kx]);
  if (idx < Cout) {
    const double s = (double)gamma[idx] / sqrt((double)var[idx] + eps);
    scale[idx] = (float)s;
    shift[idx] = (float)((double)beta[idx] - (double)mean[idx] * s);
  }
}

template <typename XT, int RES, bool RELU, typename OT>
int conv_launch_tile(const ConvArgs& a, int tile, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(a.M, kConvTiles[tile].bm), (unsigned)ceil_div(a.Cout, kConvTiles[tile].bn));
  if (tile == 0) conv_nhwc_bf16_kernel<XT, RES, RELU, OT, kConvTiles[0].bm, kConvTiles[0].bn><<<grid, kConvThreads, 0, s>>>(a);
  else conv_nhwc_bf16_kernel<XT, RES, RELU, OT, kConvTiles[1].bm, kConvTiles[1].bn><<<grid, kConvThreads, 0, s>>>(a);
  return check_launch("conv2d_nhwc");
}
template <typename XT, int RES, bool RELU>
int conv_launch_out(const ConvArgs& a, int out_dtype, int tile, hipStream_t s) {
  return out_dtype == AVF_F32 ? conv_launch_tile<XT, RES, RELU, float>(a, tile, s) : conv_launch_tile<XT, RES, RELU, bf16>(a, tile, s);
}
template <typename XT, int RES>
int conv_launch_relu(const ConvArgs& a, int relu, int out_dtype, int tile, hipStream_t s) {
  return relu ? conv_launch_out<XT, RES, true>(a, out_dtype, tile, s) : conv_launch_out<XT, RES, false>(a, out_dtype, tile, s);
}
template <typename XT>
int conv_launch_res(const ConvArgs& a, int res, int relu, int out_dtype, int tile, hipStream_t s) {
  if (res == 0) return conv_launch_relu<XT, 0>(a, relu, out_dtype, tile, s);
  if (res == 1) return conv_launch_relu<XT, 1>(a, relu, out_dtype, tile, s);
  return conv_launch_relu<XT, 2>(a, relu, out_dtype, tile, s);
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
  conv_pack_weight_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(
      w, gamma, beta, running_mean, running_var, eps, (bf16*)w_packed, scale, shift, Cout, Cin, k);
  return check_launch("conv_pack_weight");
}

extern "C" int avf_conv2d_nhwc(const void* x, int x_dtype, const void* w_packed, const float* scale, const float* shift,
                               const void* residual, int res_dtype, int relu, int k, int stride, void* out, int out_dtype, int N,
                               int H, int W, int Cin, int Cout, void* stream) {
  AVF_REQUIRE(x && w_packed && scale && shift && out, "conv2d_nhwc: null pointer");
  AVF_REQUIRE(is_dtype(x_dtype) && is_dtype(out_dtype) && (!residual || is_dtype(res_dtype)), "conv2d_nhwc: bad dtype (x %d, out %d, residual %d)",
              x_dtype, out_dtype, res_dtype);
  ConvArgs a;
  AVF_TRY(conv_shape("conv2d_nhwc", N, H, W, Cin, Cout, k, stride, &a));
  AVF_REQUIRE(aligned16(x) && aligned16(w_packed) && aligned16(scale) && aligned16(shift) && aligned16(out) && aligned16(residual),
              "conv2d_nhwc: every operand must be 16-byte aligned");
  const size_t xn = (size_t)N * H * W * Cin * elt(x_dtype), on = (size_t)a.M * Cout * elt(out_dtype);
  AVF_REQUIRE(apart(out, on, x, xn) && apart(out, on, w_packed, (size_t)Cout * a.K * 2) && apart(out, on, scale, (size_t)Cout * 4) &&
                  apart(out, on, shift, (size_t)Cout * 4) && (!residual || apart(out, on, residual, (size_t)a.M * Cout * elt(res_dtype))),
              "conv2d_nhwc: out overlaps an input (a tile reads pixels other tiles write)");
  a.x = x; a.w = (const bf16*)w_packed; a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
  const int res = residual ? (res_dtype == AVF_F32 ? 1 : 2) : 0;
  const int tile = conv_plan(a);
  const hipStream_t s = (hipStream_t)stream;
  return x_dtype == AVF_F32 ? conv_launch_res<float>(a, res, relu, out_dtype, tile, s) : conv_launch_res<bf16>(a, res, relu, out_dtype, tile, s);
}

extern "C" int avf_avgpool_nhwc(const void* x, int x_dtype, float* out, int64_t N, int HW, int C, void* stream) {
  AVF_REQUIRE(x && out, "avgpool_nhwc: null pointer");
  AVF_REQUIRE(is_dtype(x_dtype), "avgpool_nhwc: bad dtype %d", x_dtype);
  AVF_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 4 == 0, "avgpool_nhwc: N=%lld HW=%d C=%d (C %% 4 == 0)", (long long)N, HW, C);
  AVF_REQUIRE(aligned16(out) && ((uintptr_t)x & 7) == 0, "avgpool_nhwc: x must be 8-byte and out 16-byte aligned");
  AVF_REQUIRE(x_dtype == AVF_BF16 || aligned16(x), "avgpool_nhwc: an fp32 x must be 16-byte aligned");
  AVF_REQUIRE(apart(out, (size_t)N * C * 4, x, (size_t)N * HW * C * elt(x_dtype)), "avgpool_nhwc: out overlaps x");
  const unsigned grid = (unsigned)ceil_div(N * (C / 4), 256);
  if (x_dtype == AVF_F32) avgpool_nhwc_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)x, out, N, HW, C);
  else avgpool_nhwc_kernel<bf16><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16*)x, out, N, HW, C);
  return check_launch("avgpool_nhwc");
}
