// conv_dgrad_kernel.hpp - the data gradient of conv_kernel.hpp's NHWC convolution, its implicit-GEMM sibling, written once for
// the same two arithmetics (the operand policies ConvBf16<XT> and ConvBf16x3 of conv_kernel.hpp):
//   conv_dgrad_nhwc_kernel   gradient with respect to the input map of a 3x3 (pad 1) / 1x1 (pad 0) convolution, stride 1 / 2,
//                            on v_mfma_f32_16x16x32_bf16, with the identity add and the ReLU gate of a residual block's backward
//                            in its epilogue.  The weights are frozen: there is no weight and no BatchNorm gradient.
//
// GEMM view: rows = the N*H*W INPUT pixels, columns = Cin, reduction = kh*kw*Cout ordered tap-major / channel-minor, so a
// 32-deep chunk of one pixel is 32 consecutive output channels of ONE tap of gy:
//   acc[n, iy, ix, ci] = sum over (ky, kx), ty = iy + pad - ky, tx = ix + pad - kx, with ty % stride == 0, tx % stride == 0,
//                        oy = ty / stride in [0, Ho), ox = tx / stride in [0, Wo), and co of  gy[n, oy, ox, co] * wt[ci, ky, kx, co]
// A tap off the stride lattice or out of range is zeros written to LDS by index - no load is issued, nothing outside gy is read
// (the forward's padding rule, generalised).  At stride 2 on average 9/4 of a pixel's 9 taps are live; the dead chunks still run.
// wt [Cin, kh*kw*Cout] is conv_pack_weight_kernel's image of the transposed weight with the BatchNorm scale multiplied in, so
// tiles, staging, swizzle, fragment reads and the MFMA step are the forward's.
#pragma once
#include "conv_kernel.hpp"

namespace avf {
namespace {

struct ConvDgradArgs {
  const void* gy;      // [N, Ho, Wo, Cout]
  const bf16* w;       // packed [Cin][K]: the one bf16 image, or the hi image of the bf16x3 form
  const bf16* w_lo;    // the lo image (bf16x3 form; else null)
  const void* addend;  // [N, H, W, Cin] of out's type, or null
  const void* gate;    // [N, H, W, Cin] of out's type, or null
  void* out;           // [N, H, W, Cin]
  int N, H, W, Cin, Cout, k, stride, pad, Ho, Wo, K;  // K = k * k * Cout
  int64_t M;                                          // N * H * W
};

// Tile BM input pixels x BN input channels; everything about the tile is conv_nhwc_kernel's (weights = the MFMA's A operand, a
// lane's registers of fragments 2j and 2j + 1 = eight consecutive channels of one pixel, two LDS buffers of Ops::IMAGES images).
// ADD: v = acc + addend.  GATE: out = gate > 0 ? v : 0 (a NaN gate gives 0).  addend and gate have OT's type.
template <typename Ops, bool ADD, bool GATE, typename OT, int BM, int BN>
__global__ __launch_bounds__(kConvThreads) void conv_dgrad_nhwc_kernel(const ConvDgradArgs a) {
  constexpr int FM = BM / 64, FN = BN / 16, AP = BM * 4 / kConvThreads, NI = Ops::IMAGES;
  static_assert(BM % 64 == 0 && BN % 32 == 0 && BN * 4 <= kConvThreads, "tile");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][NI][(BM + BN) * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const typename Ops::X* gy = reinterpret_cast<const typename Ops::X*>(a.gy);

  // staging: thread -> tile row(s) tid / 4 (+ 64), piece tid % 4.  (n, iy, ix) of a row is decoded here, once.
  const int piece = tid & 3;
  const int smask = a.stride - 1, sshift = a.stride >> 1;  // stride 1 or 2
  int ty0[AP], tx0[AP];
  int64_t img[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int64_t m = m0 + (tid >> 2) + i * 64;
    const bool valid = m < a.M;
    const int64_t n = valid ? m / (a.H * a.W) : 0;
    const int r = valid ? (int)(m - n * (a.H * a.W)) : 0;
    const int iy = r / a.W, ix = r - iy * a.W;
    ty0[i] = valid ? iy + a.pad : -(1 << 24);  // a row past M: every tap is dead
    tx0[i] = ix + a.pad;
    img[i] = n * a.Ho;
  }
  const int wr = tid >> 2;  // weight tile row (threads below BN * 4)
  const int wch = n0 + (wr >> 5) * 32 + ((wr >> 2) & 3) * 8 + ((wr >> 4) & 1) * 4 + (wr & 3);
  const bool wvalid = tid < BN * 4 && wch < a.Cin;
  const int64_t woff = (int64_t)(wvalid ? wch : 0) * a.K + piece * 8;
  const bf16 *wrow = a.w + woff, *wrow_lo = a.w_lo + woff;

  const int cpt = a.Cout / kConvBK;  // chunks per tap
  const int nc = a.k * a.k * cpt;
  Ops ra[AP];
  uint4 rb[NI];
  auto fetch = [&](int c) {
    const int tap = c / cpt, c0 = (c - tap * cpt) * kConvBK + piece * 8;
    const int ky = tap / a.k, kx = tap - ky * a.k;
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int ty = ty0[i] - ky, tx = tx0[i] - kx;
      const int oy = ty >> sshift, ox = tx >> sshift;
      // on the stride lattice, and inside gy: ty, tx >= 0 is the unsigned compare's other half
      if (((ty | tx) & smask) == 0 && ty >= 0 && tx >= 0 && oy < a.Ho && ox < a.Wo)
        ra[i].load(gy + ((img[i] + oy) * a.Wo + ox) * a.Cout + c0);
      else ra[i].zero();
    }
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
        if constexpr (NI == 2) {  // g w ~ hi_w lo_g + lo_w hi_g + hi_w hi_g: the two small terms first (lo_w lo_g is not computed)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][j], pf[1][i], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][j], pf[0][i], acc[i][j], 0, 0, 0);
        }
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][j], pf[0][i], acc[i][j], 0, 0, 0);
      }
    // the other buffer was last read in the iteration before, which every wave left through the barrier below
    if (c + 1 < nc) stash(buf ^ 1);
    __syncthreads();
  }

  // epilogue: v = acc (+ addend), out = gate > 0 ? v : 0, store
  OT* out = reinterpret_cast<OT*>(a.out);
  constexpr bool F32 = std::is_same<OT, float>::value;
  auto load8 = [](const void* base, int64_t o, float(&r)[8]) {
    if constexpr (F32) load8f(reinterpret_cast<const float*>(base) + o, r);
    else unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(base) + o), r);
  };
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int64_t m = m0 + wave * (BM / 4) + i * 16 + (lane & 15);
    if (m >= a.M) continue;
#pragma unroll
    for (int j = 0; j < FN / 2; ++j) {
      const int ch = n0 + j * 32 + (lane >> 4) * 8;
      if (ch >= a.Cin) continue;  // Cin % 16 == 0: eight channels are inside or outside together
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = acc[i][2 * j][e];
        v[4 + e] = acc[i][2 * j + 1][e];
      }
      const int64_t o = m * a.Cin + ch;
      if constexpr (ADD) {
        float r[8];
        load8(a.addend, o, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += r[e];
      }
      if constexpr (GATE) {
        float g[8];
        load8(a.gate, o, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = g[e] > 0.f ? v[e] : 0.f;
      }
      if constexpr (F32) {
        *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(out + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
      } else {
        *reinterpret_cast<uint4*>(out + o) = pack8(v);
      }
    }
  }
}

// The shape rules of the data gradient; fills a's geometry.  The roles of the two channel counts are the forward's, swapped:
// the reduction runs over Cout, the columns are Cin.
int conv_dgrad_shape(const char* who, int N, int H, int W, int Cin, int Cout, int k, int stride, ConvDgradArgs* a) {
  AVF_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "%s: empty shape (N=%d H=%d W=%d Cin=%d Cout=%d)", who, N, H, W, Cin, Cout);
  AVF_REQUIRE(k == 3 || k == 1, "%s: kernel size %d: 3 (pad 1) or 1 (pad 0)", who, k);
  AVF_REQUIRE(stride == 1 || stride == 2, "%s: stride %d: 1 or 2", who, stride);
  AVF_REQUIRE(Cout % kConvBK == 0, "%s: Cout=%d: Cout %% 32 == 0 (a reduction chunk is 32 output channels of one tap)", who, Cout);
  AVF_REQUIRE(Cin % 16 == 0, "%s: Cin=%d: Cin %% 16 == 0", who, Cin);
  AVF_REQUIRE((int64_t)k * k * Cout < (1 << 30), "%s: reduction too deep", who);
  a->N = N; a->H = H; a->W = W; a->Cin = Cin; a->Cout = Cout; a->k = k; a->stride = stride;
  a->pad = k == 3 ? 1 : 0;
  a->Ho = (H + 2 * a->pad - k) / stride + 1;
  a->Wo = (W + 2 * a->pad - k) / stride + 1;
  a->K = k * k * Cout;
  a->M = (int64_t)N * H * W;
  AVF_REQUIRE((int64_t)H * W < (1ll << 31) && ceil_div(a->M, 64) < (1ll << 31), "%s: too many input pixels", who);
  return 0;
}

// conv_common.hpp's plan rule on M = N*H*W rows and Cin columns
int conv_dgrad_plan(const ConvDgradArgs& a) {
  ConvArgs g{};
  g.M = a.M;
  g.Cout = a.Cin;
  return conv_plan(g);
}

// What the two entry points check before they launch, in conv_operands' order: no null operand, the dtypes, the shape, 16-byte
// alignment, out apart from every input.  a comes with its pointers set; images = 2 needs w_lo.  addend and gate have out's type.
int conv_dgrad_operands(const char* who, ConvDgradArgs* a, int images, int gy_dtype, int out_dtype, int N, int H, int W, int Cin, int Cout,
                        int k, int stride) {
  AVF_REQUIRE(a->gy && a->w && (images == 1 || a->w_lo) && a->out, "%s: null pointer", who);
  AVF_REQUIRE(is_dtype(gy_dtype) && is_dtype(out_dtype), "%s: bad dtype (gy %d, out %d)", who, gy_dtype, out_dtype);
  AVF_TRY(conv_dgrad_shape(who, N, H, W, Cin, Cout, k, stride, a));
  const size_t wn = (size_t)Cin * a->K * 2, on = (size_t)a->M * Cin * elt(out_dtype);
  const void* in[] = {a->gy, a->w, a->w_lo, a->addend, a->gate};
  const size_t bytes[] = {(size_t)N * a->Ho * a->Wo * Cout * elt(gy_dtype), wn, wn, on, on};
  bool al = aligned(a->out, 16), ap = true;
  for (int i = 0; i < 5; ++i) {
    al = al && aligned(in[i], 16);
    ap = ap && (!in[i] || apart(a->out, on, in[i], bytes[i]));
  }
  AVF_REQUIRE(al, "%s: every operand must be 16-byte aligned", who);
  AVF_REQUIRE(ap, "%s: out overlaps an input (a tile reads pixels other tiles write)", who);
  return 0;
}

// the launch ladder below the entry point's own choice of Ops and OT: addend, gate, then the tile conv_dgrad_plan picked
template <typename Ops, bool ADD, bool GATE, typename OT>
int conv_dgrad_launch_tile(const char* who, const ConvDgradArgs& a, hipStream_t s) {
  const int tile = conv_dgrad_plan(a);
  const dim3 grid((unsigned)ceil_div(a.M, kConvTiles[tile].bm), (unsigned)ceil_div(a.Cin, kConvTiles[tile].bn));
  if (tile == 0) conv_dgrad_nhwc_kernel<Ops, ADD, GATE, OT, kConvTiles[0].bm, kConvTiles[0].bn><<<grid, kConvThreads, 0, s>>>(a);
  else conv_dgrad_nhwc_kernel<Ops, ADD, GATE, OT, kConvTiles[1].bm, kConvTiles[1].bn><<<grid, kConvThreads, 0, s>>>(a);
  return check_launch(who);
}
template <typename Ops, typename OT>
int conv_dgrad_launch(const char* who, const ConvDgradArgs& a, hipStream_t s) {
  if (a.addend) return a.gate ? conv_dgrad_launch_tile<Ops, true, true, OT>(who, a, s) : conv_dgrad_launch_tile<Ops, true, false, OT>(who, a, s);
  return a.gate ? conv_dgrad_launch_tile<Ops, false, true, OT>(who, a, s) : conv_dgrad_launch_tile<Ops, false, false, OT>(who, a, s);
}

}  // namespace
}  // namespace avf
