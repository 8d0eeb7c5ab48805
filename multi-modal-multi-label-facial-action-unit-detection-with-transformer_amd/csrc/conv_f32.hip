// conv_f32.hip - the parity-mode form of conv.hip's convolution: fp32 NHWC in, fp32 NHWC out, every fp32 product computed as
// three bf16 MFMA products ("bf16x3", as gemm_f32.hip and attn_f32x3.hip do it; oracle/bf16x3.py is the CPU statement):
//   conv_nhwc_f32x3_kernel          the implicit GEMM of conv_nhwc_bf16_kernel - same GEMM view, tiles, staging decode,
//                                   padding-by-index rule and epilogue - with both operands split into hi + lo bf16 images
//   conv_pack_weight_f32x3_kernel   nn.Conv2d's [Cout, Cin, kh, kw] fp32 weight -> two [Cout, kh, kw, Cin] bf16 images (hi, lo),
//                                   BatchNorm2d's running statistics -> one (scale, shift) pair per channel
// The split:  hi = bf16(v) (round to nearest even),  lo = bf16(v - hi) (v - hi is exact in fp32);
//   x w ~ hi_w lo_x + lo_w hi_x + hi_w hi_x  (each bf16 x bf16 product is exact in fp32; lo_w lo_x, <= 2^-16 |x w|, is not computed).
// The activations are split while they are staged (a thread's eight fp32 channels -> one 16-byte piece of each image), the weights
// arrive split.  This is the conv's ONE parity arithmetic: there is no plain-fp32 (VALU) form.
#include "conv_common.hpp"

namespace avf {
namespace {

struct ConvF32Args : ConvArgs {  // w: the hi image
  const bf16* w_lo;              // packed [Cout][K], as w
};

// gemm_f32.hip's split2: two fp32 -> the packed hi pair and the packed lo pair
__device__ __forceinline__ void conv_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack_bf16x2(a, b);
  lo = pack_bf16x2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

// 8 consecutive fp32 channels as they come from memory: kept raw until they are written to LDS (the one stage of look-ahead)
struct RawF8 {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ __forceinline__ void zero() { a = b = make_float4(0.f, 0.f, 0.f, 0.f); }
  // -> the 16-byte piece of the hi image (LO = false) or of the lo image
  template <bool LO>
  __device__ __forceinline__ uint4 piece() const {
    uint32_t h[4], l[4];
    conv_split2(a.x, a.y, h[0], l[0]);
    conv_split2(a.z, a.w, h[1], l[1]);
    conv_split2(b.x, b.y, h[2], l[2]);
    conv_split2(b.z, b.w, h[3], l[3]);
    return LO ? make_uint4(l[0], l[1], l[2], l[3]) : make_uint4(h[0], h[1], h[2], h[3]);
  }
};

// Tile BM pixels x BN channels, laid out as conv_nhwc_bf16_kernel lays it out (weights = the MFMA's A operand, pixels = B; tile
// row f * 16 + q * 4 + r of a weight image holds channel (f / 2) * 32 + q * 8 + (f % 2) * 4 + r).  One buffer is two images, hi
// then lo, each (BM + BN) rows of 64 bytes with conv_lds_off's swizzle; two buffers: 4 * (BM + BN) * 64 bytes (48 KiB at 128 x 64).
template <bool RES, bool RELU, int BM, int BN>
__global__ __launch_bounds__(kConvThreads) void conv_nhwc_f32x3_kernel(const ConvF32Args a) {
  constexpr int FM = BM / 64, FN = BN / 16, AP = BM * 4 / kConvThreads, IMG = (BM + BN) * 64;
  static_assert(BM % 64 == 0 && BN % 32 == 0 && BN * 4 <= kConvThreads, "tile");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const float* x = reinterpret_cast<const float*>(a.x);

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
  const int64_t woff = (int64_t)(wvalid ? wch : 0) * a.K + piece * 8;
  const bf16 *wrow_hi = a.w + woff, *wrow_lo = a.w_lo + woff;

  const int cpt = a.Cin / kConvBK;  // chunks per tap
  const int nc = a.k * a.k * cpt;
  RawF8 ra[AP];
  uint4 rb_hi, rb_lo;
  auto fetch = [&](int c) {
    const int tap = c / cpt, c0 = (c - tap * cpt) * kConvBK + piece * 8;
    const int ky = tap / a.k, kx = tap - ky * a.k;
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int iy = iy0[i] + ky, ix = ix0[i] + kx;
      if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ra[i].load(x + ((img[i] + iy) * a.W + ix) * a.Cin + c0);
      else ra[i].zero();
    }
    // (an invalid row reads row 0 - inside the images - and keeps zeros)
    const uint4 h = *reinterpret_cast<const uint4*>(wrow_hi + (int64_t)c * kConvBK), l = *reinterpret_cast<const uint4*>(wrow_lo + (int64_t)c * kConvBK);
    rb_hi = wvalid ? h : make_uint4(0u, 0u, 0u, 0u);
    rb_lo = wvalid ? l : make_uint4(0u, 0u, 0u, 0u);
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int off = conv_lds_off((tid >> 2) + i * 64, piece);
      *reinterpret_cast<uint4*>(&lds[buf][0][off]) = ra[i].template piece<false>();
      *reinterpret_cast<uint4*>(&lds[buf][1][off]) = ra[i].template piece<true>();
    }
    if (tid < BN * 4) {
      const int off = BM * 64 + conv_lds_off(wr, piece);
      *reinterpret_cast<uint4*>(&lds[buf][0][off]) = rb_hi;
      *reinterpret_cast<uint4*>(&lds[buf][1][off]) = rb_lo;
    }
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
    bf16x8_t ph[FM], pl[FM], wh[FN], wl[FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int off = conv_lds_off(wave * (BM / 4) + i * 16 + (lane & 15), lane >> 4);
      ph[i] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][0][off]);
      pl[i] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][1][off]);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int off = BM * 64 + conv_lds_off(j * 16 + (lane & 15), lane >> 4);
      wh[j] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][0][off]);
      wl[j] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][1][off]);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {  // the two small terms first
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], pl[i], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], ph[i], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], ph[i], acc[i][j], 0, 0, 0);
      }
    // the other buffer was last read in the iteration before, which every wave left through the barrier below
    if (c + 1 < nc) stash(buf ^ 1);
    __syncthreads();
  }

  // epilogue: y = acc * scale[c] + shift[c] (the folded BatchNorm), + identity, ReLU, two 16-byte stores
  float* out = reinterpret_cast<float*>(a.out);
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
      if constexpr (RES) {
        float r[8];
        load8f(reinterpret_cast<const float*>(a.res) + o, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += r[e];
      }
      if constexpr (RELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];  // (a NaN stays a NaN)
      }
      *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(out + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
  }
}

// one thread per packed element; the first Cout threads also fold their channel's BatchNorm in fp64
__global__ __launch_bounds__(256) void conv_pack_weight_f32x3_kernel(const float* w, const float* gamma, const float* beta,
                                                                     const float* mean, const float* var, double eps, bf16* w_hi,
                                                                     bf16* w_lo, float* scale, float* shift, int Cout, int Cin, int k) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t K = (int64_t)k * k * Cin;
  if (idx >= Cout * K) return;
  const int64_t co = idx / K;
  const int r = (int)(idx - co * K);
  const int tap = r / Cin, ci = r - tap * Cin;
  const int ky = tap / k, kx = tap - ky * k;
  const float v = w[((co * Cin + ci) * k + ky) * k + kx];
  const bf16 hi = from_f32<bf16>(v);
  w_hi[idx] = hi;
  w_lo[idx] = from_f32<bf16>(v - to_f32<bf16>(hi));
  if (idx < Cout) {
    const double s = (double)gamma[idx] / sqrt((double)var[idx] + eps);
    scale[idx] = (float)s;
    shift[idx] = (float)((double)beta[idx] - (double)mean[idx] * s);
  }
}

template <bool RES, bool RELU>
int conv_f32x3_launch_tile(const ConvF32Args& a, int tile, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(a.M, kConvTiles[tile].bm), (unsigned)ceil_div(a.Cout, kConvTiles[tile].bn));
  if (tile == 0) conv_nhwc_f32x3_kernel<RES, RELU, kConvTiles[0].bm, kConvTiles[0].bn><<<grid, kConvThreads, 0, s>>>(a);
  else conv_nhwc_f32x3_kernel<RES, RELU, kConvTiles[1].bm, kConvTiles[1].bn><<<grid, kConvThreads, 0, s>>>(a);
  return check_launch("conv2d_nhwc_f32x3");
}
template <bool RES>
int conv_f32x3_launch_relu(const ConvF32Args& a, int relu, int tile, hipStream_t s) {
  return relu ? conv_f32x3_launch_tile<RES, true>(a, tile, s) : conv_f32x3_launch_tile<RES, false>(a, tile, s);
}

}  // namespace
}  // namespace avf

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
  conv_pack_weight_f32x3_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(
      w, gamma, beta, running_mean, running_var, eps, (bf16*)w_hi, (bf16*)w_lo, scale, shift, Cout, Cin, k);
  return check_launch("conv_pack_weight_f32x3");
}

extern "C" int avf_conv2d_nhwc_f32x3(const float* x, const void* w_hi, const void* w_lo, const float* scale, const float* shift,
                                     const float* residual, int relu, int k, int stride, float* out, int N, int H, int W, int Cin,
                                     int Cout, void* stream) {
  AVF_REQUIRE(x && w_hi && w_lo && scale && shift && out, "conv2d_nhwc_f32x3: null pointer");
  ConvF32Args a;
  AVF_TRY(conv_shape("conv2d_nhwc_f32x3", N, H, W, Cin, Cout, k, stride, &a));
  AVF_REQUIRE(aligned16(x) && aligned16(w_hi) && aligned16(w_lo) && aligned16(scale) && aligned16(shift) && aligned16(out) &&
                  aligned16(residual),
              "conv2d_nhwc_f32x3: every operand must be 16-byte aligned");
  const size_t xn = (size_t)N * H * W * Cin * 4, on = (size_t)a.M * Cout * 4, wn = (size_t)Cout * a.K * 2;
  AVF_REQUIRE(apart(out, on, x, xn) && apart(out, on, w_hi, wn) && apart(out, on, w_lo, wn) && apart(out, on, scale, (size_t)Cout * 4) &&
                  apart(out, on, shift, (size_t)Cout * 4) && (!residual || apart(out, on, residual, on)),
              "conv2d_nhwc_f32x3: out overlaps an input (a tile reads pixels other tiles write)");
  a.x = x; a.w = (const bf16*)w_hi; a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
  a.w_lo = (const bf16*)w_lo;
  const int tile = conv_plan(a);
  const hipStream_t s = (hipStream_t)stream;
  return residual ? conv_f32x3_launch_relu<true>(a, relu, tile, s) : conv_f32x3_launch_relu<false>(a, relu, tile, s);
}
