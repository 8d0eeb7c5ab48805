// conv_kernel.hpp - the NHWC implicit-GEMM convolution of the frozen ResNet stages, written once for its two arithmetics:
//   conv_nhwc_kernel         3x3 (pad 1) / 1x1 (pad 0) convolution, stride 1 / 2, on v_mfma_f32_16x16x32_bf16, with the folded
//                            eval-mode BatchNorm, the identity add and the ReLU in its epilogue
//   conv_pack_weight_kernel  nn.Conv2d's [Cout, Cin, kh, kw] fp32 weight -> [Cout, kh, kw, Cin] bf16 (one image, or hi and lo),
//                            BatchNorm2d's running statistics -> one (scale, shift) pair per channel
// An operand policy (Ops) says how eight activation channels are held raw and how many bf16 LDS images they become:
//   ConvBf16<XT>  one image: a bf16 activation as it is, an fp32 one rounded to nearest even                         (conv.hip)
//   ConvBf16x3    two images, hi = bf16(v) and lo = bf16(v - hi), of an fp32 activation; the weights arrive split the same way
//                 and every fp32 product runs as three bf16 MFMA products                                            (conv_f32.hip)
//
// GEMM view: rows = the N*Ho*Wo output pixels, columns = Cout, reduction = kh*kw*Cin ordered tap-major / channel-minor, so a
// 32-deep chunk of one pixel is 32 consecutive channels of ONE tap: in range (two or four 16-byte loads) or padding (zeros
// written to LDS by index - no load is issued, nothing outside the input is read).
#pragma once
#include "bf16x3.hpp"
#include "conv_common.hpp"

namespace avf {
namespace {

// 8 consecutive channels as they come from memory: kept raw until they are written to LDS, so that the wait for the load
// sits behind the MFMAs of the chunk before (the one stage of look-ahead).  image<IM>(): the 16-byte piece of LDS image IM.
template <typename XT>
struct ConvBf16;
template <>
struct ConvBf16<bf16> {
  using X = bf16;
  static constexpr int IMAGES = 1;
  uint4 v;
  __device__ __forceinline__ void load(const bf16* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void zero() { v = make_uint4(0u, 0u, 0u, 0u); }
  template <int IM>
  __device__ __forceinline__ uint4 image() const { return v; }
};
struct ConvRawF8 {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ __forceinline__ void zero() { a = b = make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <>
struct ConvBf16<float> : ConvRawF8 {
  using X = float;
  static constexpr int IMAGES = 1;
  template <int IM>
  __device__ __forceinline__ uint4 image() const {  // RNE, as a bf16 activation would have been stored
    return make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
  }
};

struct ConvBf16x3 : ConvRawF8 {
  using X = float;
  static constexpr int IMAGES = 2;  // hi, lo
  template <int IM>
  __device__ __forceinline__ uint4 image() const {
    uint32_t h[4], l[4];
    split2(a.x, a.y, h[0], l[0]);
    split2(a.z, a.w, h[1], l[1]);
    split2(b.x, b.y, h[2], l[2]);
    split2(b.z, b.w, h[3], l[3]);
    return IM ? make_uint4(l[0], l[1], l[2], l[3]) : make_uint4(h[0], h[1], h[2], h[3]);
  }
};

// Tile BM pixels x BN channels.  The weights are the MFMA's A operand and the pixels its B operand, so a lane's four accumulator
// registers are four consecutive CHANNELS of one pixel; tile row f * 16 + q * 4 + r of a weight image holds channel
// (f / 2) * 32 + q * 8 + (f % 2) * 4 + r, which makes the registers of fragments 2j and 2j + 1 eight consecutive channels:
// one 16-byte store per lane for bf16, two for fp32.  One buffer is Ops::IMAGES images, each (BM + BN) rows of 64 bytes with
// conv_lds_off's swizzle; two buffers: 24 KiB at 128 x 64 with one image, 48 KiB with two.
// RES: 0 none, 1 fp32, 2 bf16.
// The second image is written out under if constexpr (NI == 2) at each site (weight load, the two stashes, the two fragment
// reads, the MFMA step) instead of looped over: loops over the images are unrolled late and hipcc then orders the instructions
// of both forms differently, which moved their timings.
template <typename Ops, int RES, bool RELU, typename OT, int BM, int BN>
__global__ __launch_bounds__(kConvThreads) void conv_nhwc_kernel(const ConvArgs a) {
  constexpr int FM = BM / 64, FN = BN / 16, AP = BM * 4 / kConvThreads, NI = Ops::IMAGES;
  static_assert(BM % 64 == 0 && BN % 32 == 0 && BN * 4 <= kConvThreads, "tile");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][NI][(BM + BN) * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const typename Ops::X* x = reinterpret_cast<const typename Ops::X*>(a.x);

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
  const bf16 *wrow = a.w + woff, *wrow_lo = a.w_lo + woff;

  const int cpt = a.Cin / kConvBK;  // chunks per tap
  const int nc = a.k * a.k * cpt;
  Ops ra[AP];
  uint4 rb[NI];
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
    const uint4 h = *reinterpret_cast<const uint4*>(wrow + (int64_t)c * kConvBK);
    if constexpr (NI == 2) {
      const uint4 l = *reinterpret_cast<const uint4*>(wrow_lo + (int64_t)c * kConvBK);
      rb[1] = wvalid ? l : make_uint4(0u, 0u, 0u, 0u);
    }
    rb[0] = wvalid ? h : make_uint4(0u, 0u, 0u, 0u);
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int off = conv_lds_off((tid >> 2) + i * 64, piece);
      *reinterpret_cast<uint4*>(&lds[buf][0][off]) = ra[i].template image<0>();
      if constexpr (NI == 2) *reinterpret_cast<uint4*>(&lds[buf][1][off]) = ra[i].template image<1>();
    }
    if (tid < BN * 4) {
      const int off = BM * 64 + conv_lds_off(wr, piece);
      *reinterpret_cast<uint4*>(&lds[buf][0][off]) = rb[0];
      if constexpr (NI == 2) *reinterpret_cast<uint4*>(&lds[buf][1][off]) = rb[1];
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
    bf16x8_t pf[NI][FM], wf[NI][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int off = conv_lds_off(wave * (BM / 4) + i * 16 + (lane & 15), lane >> 4);
      pf[0][i] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][0][off]);
      if constexpr (NI == 2) pf[1][i] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][1][off]);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int off = BM * 64 + conv_lds_off(j * 16 + (lane & 15), lane >> 4);
      wf[0][j] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][0][off]);
      if constexpr (NI == 2) wf[1][j] = *reinterpret_cast<const bf16x8_t*>(&lds[buf][1][off]);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        if constexpr (NI == 2) {  // x w ~ hi_w lo_x + lo_w hi_x + hi_w hi_x: the two small terms first (lo_w lo_x is not computed)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][j], pf[1][i], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][j], pf[0][i], acc[i][j], 0, 0, 0);
        }
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][j], pf[0][i], acc[i][j], 0, 0, 0);
      }
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

// one thread per packed element; the first Cout threads also fold their channel's BatchNorm.  SPLIT: w_lo = bf16(w - w_hi) too.
template <bool SPLIT>
__global__ __launch_bounds__(256) void conv_pack_weight_kernel(const float* w, const float* gamma, const float* beta, const float* mean,
                                                               const float* var, double eps, bf16* w_hi, bf16* w_lo, float* scale,
                                                               float* shift, int Cout, int Cin, int k) {
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
  if constexpr (SPLIT) w_lo[idx] = from_f32<bf16>(v - to_f32<bf16>(hi));
  if (idx < Cout) bn_fold(gamma, beta, mean, var, eps, idx, scale, shift);
}

// the launch ladder below the entry point's own choice of Ops, RES and OT: ReLU, then the tile conv_plan picked
template <typename Ops, int RES, bool RELU, typename OT>
int conv_launch_tile(const char* who, const ConvArgs& a, int tile, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(a.M, kConvTiles[tile].bm), (unsigned)ceil_div(a.Cout, kConvTiles[tile].bn));
  if (tile == 0) conv_nhwc_kernel<Ops, RES, RELU, OT, kConvTiles[0].bm, kConvTiles[0].bn><<<grid, kConvThreads, 0, s>>>(a);
  else conv_nhwc_kernel<Ops, RES, RELU, OT, kConvTiles[1].bm, kConvTiles[1].bn><<<grid, kConvThreads, 0, s>>>(a);
  return check_launch(who);
}
template <typename Ops, int RES, typename OT>
int conv_launch(const char* who, const ConvArgs& a, int relu, hipStream_t s) {
  const int tile = conv_plan(a);
  return relu ? conv_launch_tile<Ops, RES, true, OT>(who, a, tile, s) : conv_launch_tile<Ops, RES, false, OT>(who, a, tile, s);
}

}  // namespace
}  // namespace avf
