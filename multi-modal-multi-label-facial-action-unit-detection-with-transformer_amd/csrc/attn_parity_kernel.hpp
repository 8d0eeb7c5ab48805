// attn_parity_kernel.hpp - the parity-mode attention core (compute_dtype="f32": the mode held to logits rtol 1e-3 against the fp32
// CPU reference), written once for its two arithmetics: attn_fwd_parity_kernel, attn_dq_parity_kernel, attn_dkv_parity_kernel.
//
// Reference: models/heads.py:222-237 (dots = q k^T * dh^-0.5 ; softmax(dim=-1) ; out = attn v) and its autograd.
//
// fp32 storage, fp32 statistics (flash-style, log2 domain), exp2 and every elementwise step in fp32, no token mask.  An operand
// policy (Ops) says how an operand of a matrix product is held and multiplied:
//   ParityF32Mfma<DH>  fp32 operands on v_mfma_f32_16x16x4_f32, dim_head 32 / 64 / 128       (attn_f32_mfma.hip)
//   ParityBf16x3       hi / lo bf16 operands, three bf16 MFMA products per fp32 product, dim_head 64   (attn_f32x3.hip)
//
// One workgroup = 4 wavefronts = 64 queries (forward, dQ) or 64 keys (dK/dV) of one (clip, head); the opposite operand streams
// through LDS in tiles of 32 rows.  Everything is computed TRANSPOSED so that the row a lane's statistics belong to sits on the
// lane index:   S^T = K Q^T  ->  acc[r] of lane (li, lg) = S[query li][key 4 lg + r]   (MFMA D layout: row 4 lg + r, column li).
// A 16 x 16 block of P (or dS) is then the B operand of the next product ( O^T += V^T P ), whose other operand is read from a
// transposed LDS image of the tile; what it takes to turn the accumulator registers into that B operand is the policy's
// as_operand (beside each policy).
//
// Ops supplies:
//   DH                                dim_head
//   image<I, N, TR>()                 the kernel's I-th of N LDS images of a tile (TR: a transposed one).  The policy declares the
//                                     LDS - one array per image or one per kernel - because hipcc schedules the two forms differently
//   kDeltaInDq                        the dQ kernel computes delta[q] = sum_d O[q, d] dO[q, d] itself and writes it for the dK/dV
//                                     kernel behind it (else delta is an input: attn_bwd_vec's attn_delta launch)
//   RowFrags, load_row                the lane's resident row operand (its q, dO, k or v row), scaled
//   TileRegs, fetch, commit<ROW, TR>  a tile of the streamed operand (rows row0 .., nvalid of them, the rest zero): fetch is called
//                                     before the arithmetic of the tile in front, commit (with the same row0 / nvalid) between the
//                                     barriers, for the row and / or the transposed image.  A policy moves the data in either:
//                                     global -> registers in fetch and registers -> LDS in commit, or global -> LDS in commit
//   tile_dot, as_operand, tile_acc    the two products
#pragma once
#include "common.hpp"
#include "mfma_frag.hpp"

namespace avf {
namespace {

constexpr int kParityTile = 32;  // rows of the streamed operand per tile

// where a workgroup and a lane stand: (clip b, head h), row `row` of the 64 (a query or a key), the head's columns of qkv / o
struct ParityCoords {
  int li, lg, bh, b, h, I, row;
  int64_t ld;         // row stride of qkv
  bool valid;
  const float* base;  // qkv[b, 0, 0, h, 0]
  template <int DH>
  __device__ __forceinline__ static ParityCoords make(const float* qkv, int N, int H) {
    ParityCoords c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c.li = lane & 15, c.lg = lane >> 4;
    c.bh = blockIdx.y, c.b = c.bh / H;
    c.h = c.bh - c.b * H;
    c.I = H * DH;
    c.ld = 3 * (int64_t)c.I;
    c.base = qkv + (int64_t)c.b * N * c.ld + c.h * DH;
    c.row = blockIdx.x * 64 + wave * 16 + c.li;
    c.valid = c.row < N;
    return c;
  }
};

__device__ __forceinline__ int tile_rows(int left) { return left < kParityTile ? left : kParityTile; }  // of `left` rows to go

// ---------------------------------------------------------------------------------------------- forward
template <typename Ops>
__global__ __launch_bounds__(256) void attn_fwd_parity_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                              float* __restrict__ lse2, int N, int H) {
  constexpr int DH = Ops::DH, NC = DH / 16, MT = kParityTile;
  auto *Ks = Ops::template image<0, 2, false>(), *Vt = Ops::template image<1, 2, true>();
  const ParityCoords c = ParityCoords::make<DH>(qkv, N, H);
  const int li = c.li, lg = c.lg, I = c.I;
  typename Ops::RowFrags qf;
  Ops::load_row(qf, c.base + (int64_t)c.row * c.ld, c.valid, lg, LOG2E / sqrtf((float)DH));
  f32x4_t acc[NC];
#pragma unroll
  for (int db = 0; db < NC; ++db) acc[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;  // l: this lane group's share of the row sum (its 8 keys per tile); summed over the groups at the end
  typename Ops::TileRegs kr = Ops::fetch(c.base + I, c.ld, 0, tile_rows(N)), vr = Ops::fetch(c.base + 2 * I, c.ld, 0, tile_rows(N));
  for (int kt = 0; kt < N; kt += MT) {
    const int nk = tile_rows(N - kt);
    __syncthreads();
    Ops::template commit<true, false>(kr, kt, nk, Ks, nullptr);
    Ops::template commit<false, true>(vr, kt, nk, nullptr, Vt);
    __syncthreads();
    if (kt + MT < N) {  // (a policy that loads in fetch: the next tile's loads fly during this tile's arithmetic)
      kr = Ops::fetch(c.base + I, c.ld, kt + MT, tile_rows(N - kt - MT));
      vr = Ops::fetch(c.base + 2 * I, c.ld, kt + MT, tile_rows(N - kt - MT));
    }
    f32x4_t s[2];
    Ops::tile_dot(s, Ks, qf, li, lg);  // s[kb][r] = S[query li][key kt + 16 kb + 4 lg + r] (log2 domain)
    float tmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (16 * kb + 4 * lg + r >= nk) s[kb][r] = -INFINITY;
        tmax = fmaxf(tmax, s[kb][r]);
      }
    tmax = groups_max_shfl(tmax);
    const float mn = fmaxf(m, tmax);
    const float alpha = exp2f(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int db = 0; db < NC; ++db) {
      acc[db][0] *= alpha; acc[db][1] *= alpha; acc[db][2] *= alpha; acc[db][3] *= alpha;
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kb][r] = exp2f(s[kb][r] - mn);
        l += s[kb][r];
      }
      Ops::as_operand(s[kb]);
    }
    Ops::tile_acc(acc, Vt, s, li, lg);  // O^T += V^T P
  }
  l = groups_sum_shfl(l);
  if (c.valid) {
    const float inv = 1.0f / l;
    float* orow = o + ((int64_t)c.b * N + c.row) * I + c.h * DH;
#pragma unroll
    for (int db = 0; db < NC; ++db)
      *reinterpret_cast<float4*>(orow + 16 * db + 4 * lg) =
          make_float4(acc[db][0] * inv, acc[db][1] * inv, acc[db][2] * inv, acc[db][3] * inv);
    if (lg == 0) lse2[(int64_t)c.bh * N + c.row] = m + log2f(l);
  }
}

// ---------------------------------------------------------------------------------------------- dQ
// dS = P o (dP - delta),  dq = dS k * dh^-0.5   (64 queries per workgroup, keys streamed)
// Ops::kDeltaInDq: o is read and delta written (this lane group's 16 of the row's DH products from the rows the kernel loads
// anyway, then the sum over the four groups) - no separate delta launch on that path; else o is unused and delta only read.
template <typename Ops>
__global__ __launch_bounds__(256) void attn_dq_parity_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                             const float* __restrict__ d_o, const float* __restrict__ lse2,
                                                             float* __restrict__ delta, float* __restrict__ dqkv, int N, int H) {
  constexpr int DH = Ops::DH, NC = DH / 16, MT = kParityTile;
  auto *Ks = Ops::template image<0, 3, false>(), *Kt = Ops::template image<1, 3, true>(), *Vs = Ops::template image<2, 3, false>();
  const ParityCoords c = ParityCoords::make<DH>(qkv, N, H);
  const int li = c.li, lg = c.lg, I = c.I;
  const float scale = 1.0f / sqrtf((float)DH);
  typename Ops::RowFrags qf, gf;
  Ops::load_row(qf, c.base + (int64_t)c.row * c.ld, c.valid, lg, LOG2E * scale);
  Ops::load_row(gf, d_o + ((int64_t)c.b * N + c.row) * I + c.h * DH, c.valid, lg, 1.0f);
  const float L = c.valid ? lse2[(int64_t)c.bh * N + c.row] : INFINITY;  // rows past the end: P = 2^(s - inf) = 0
  float dl = 0.f;
  if constexpr (Ops::kDeltaInDq) {
    if (c.valid) {
      const float* gr = d_o + ((int64_t)c.b * N + c.row) * I + c.h * DH;
      const float* orow = o + ((int64_t)c.b * N + c.row) * I + c.h * DH;
#pragma unroll
      for (int j = 0; j < DH / 32; ++j)
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
          const float4 gv = *reinterpret_cast<const float4*>(gr + 32 * j + 8 * lg + 4 * hlf);
          const float4 ov = *reinterpret_cast<const float4*>(orow + 32 * j + 8 * lg + 4 * hlf);
          dl = fmaf(gv.x, ov.x, dl); dl = fmaf(gv.y, ov.y, dl); dl = fmaf(gv.z, ov.z, dl); dl = fmaf(gv.w, ov.w, dl);
        }
    }
    dl = groups_sum_shfl(dl);
    if (c.valid && lg == 0) delta[(int64_t)c.bh * N + c.row] = dl;
  } else {
    if (c.valid) dl = delta[(int64_t)c.bh * N + c.row];
  }
  f32x4_t dq[NC];
#pragma unroll
  for (int db = 0; db < NC; ++db) dq[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  typename Ops::TileRegs kr = Ops::fetch(c.base + I, c.ld, 0, tile_rows(N)), vr = Ops::fetch(c.base + 2 * I, c.ld, 0, tile_rows(N));
  for (int kt = 0; kt < N; kt += MT) {
    const int nk = tile_rows(N - kt);
    __syncthreads();
    Ops::template commit<true, true>(kr, kt, nk, Ks, Kt);
    Ops::template commit<true, false>(vr, kt, nk, Vs, nullptr);
    __syncthreads();
    if (kt + MT < N) {
      kr = Ops::fetch(c.base + I, c.ld, kt + MT, tile_rows(N - kt - MT));
      vr = Ops::fetch(c.base + 2 * I, c.ld, kt + MT, tile_rows(N - kt - MT));
    }
    f32x4_t s[2], dp[2];
    Ops::tile_dot(s, Ks, qf, li, lg);
    Ops::tile_dot(dp, Vs, gf, li, lg);  // dP[query li][key] = dO[q] . V[key]
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool live = 16 * kb + 4 * lg + r < nk;
        const float p = live ? exp2f(s[kb][r] - L) : 0.f;
        s[kb][r] = p * (dp[kb][r] - dl);
      }
      Ops::as_operand(s[kb]);
    }
    Ops::tile_acc(dq, Kt, s, li, lg);  // dQ^T += K^T dS^T
  }
  if (c.valid) {
    float* out = dqkv + ((int64_t)c.b * N + c.row) * c.ld + c.h * DH;
#pragma unroll
    for (int db = 0; db < NC; ++db)
      *reinterpret_cast<float4*>(out + 16 * db + 4 * lg) =
          make_float4(dq[db][0] * scale, dq[db][1] * scale, dq[db][2] * scale, dq[db][3] * scale);
  }
}

// ---------------------------------------------------------------------------------------------- dK, dV
// dv = P^T dO,  dk = dS^T q * dh^-0.5   (64 keys per workgroup, queries streamed; one recomputation of P serves both)
template <typename Ops>
__global__ __launch_bounds__(256) void attn_dkv_parity_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                              const float* __restrict__ lse2, const float* __restrict__ delta,
                                                              float* __restrict__ dqkv, int N, int H) {
  constexpr int DH = Ops::DH, NC = DH / 16, MT = kParityTile;
  auto *Qs = Ops::template image<0, 4, false>(), *Qt = Ops::template image<1, 4, true>();
  auto *Gs = Ops::template image<2, 4, false>(), *Gt = Ops::template image<3, 4, true>();
  __shared__ __attribute__((aligned(16))) float Ls[MT];
  __shared__ __attribute__((aligned(16))) float Ds[MT];
  const ParityCoords c = ParityCoords::make<DH>(qkv, N, H);
  const int li = c.li, lg = c.lg, I = c.I;
  const float* gbase = d_o + (int64_t)c.b * N * I + c.h * DH;
  const float scale = 1.0f / sqrtf((float)DH);
  typename Ops::RowFrags kf, vf;
  Ops::load_row(kf, c.base + I + (int64_t)c.row * c.ld, c.valid, lg, LOG2E * scale);
  Ops::load_row(vf, c.base + 2 * I + (int64_t)c.row * c.ld, c.valid, lg, 1.0f);
  f32x4_t dk[NC], dv[NC];
#pragma unroll
  for (int db = 0; db < NC; ++db) dk[db] = dv[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  typename Ops::TileRegs qr = Ops::fetch(c.base, c.ld, 0, tile_rows(N)), gr = Ops::fetch(gbase, I, 0, tile_rows(N));
  for (int qt = 0; qt < N; qt += MT) {
    const int nq = tile_rows(N - qt);
    __syncthreads();
    Ops::template commit<true, true>(qr, qt, nq, Qs, Qt);
    Ops::template commit<true, true>(gr, qt, nq, Gs, Gt);
    if (threadIdx.x < MT) {
      const bool ok = (int)threadIdx.x < nq;
      Ls[threadIdx.x] = ok ? lse2[(int64_t)c.bh * N + qt + threadIdx.x] : INFINITY;  // 2^(s - inf) = 0
      Ds[threadIdx.x] = ok ? delta[(int64_t)c.bh * N + qt + threadIdx.x] : 0.f;
    }
    __syncthreads();
    if (qt + MT < N) {
      qr = Ops::fetch(c.base, c.ld, qt + MT, tile_rows(N - qt - MT));
      gr = Ops::fetch(gbase, I, qt + MT, tile_rows(N - qt - MT));
    }
    f32x4_t s[2], dp[2];
    Ops::tile_dot(s, Qs, kf, li, lg);   // s[qb][r] = S[query qt + 16 qb + 4 lg + r][key li]
    Ops::tile_dot(dp, Gs, vf, li, lg);  // dP[query][key li] = dO[q] . V[key]
    f32x4_t pt[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const float4 Lq = *reinterpret_cast<const float4*>(Ls + 16 * qb + 4 * lg);
      const float4 Dq = *reinterpret_cast<const float4*>(Ds + 16 * qb + 4 * lg);
      const float Lr[4] = {Lq.x, Lq.y, Lq.z, Lq.w}, Dr[4] = {Dq.x, Dq.y, Dq.z, Dq.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2f(s[qb][r] - Lr[r]);
        pt[qb][r] = p;
        s[qb][r] = p * (dp[qb][r] - Dr[r]);
      }
      Ops::as_operand(pt[qb]);
      Ops::as_operand(s[qb]);
    }
    Ops::tile_acc(dv, Gt, pt, li, lg);  // dV^T += dO^T P
    Ops::tile_acc(dk, Qt, s, li, lg);   // dK^T += Q^T dS
  }
  if (c.valid) {
    float* outk = dqkv + ((int64_t)c.b * N + c.row) * c.ld + I + c.h * DH;
    float* outv = outk + I;
#pragma unroll
    for (int db = 0; db < NC; ++db) {
      *reinterpret_cast<float4*>(outk + 16 * db + 4 * lg) = make_float4(dk[db][0] * scale, dk[db][1] * scale, dk[db][2] * scale, dk[db][3] * scale);
      *reinterpret_cast<float4*>(outv + 16 * db + 4 * lg) = make_float4(dv[db][0], dv[db][1], dv[db][2], dv[db][3]);
    }
  }
}

// the two launches behind an entry point's grid
template <typename Ops>
int attn_parity_fwd(const char* who, const float* qkv, float* o, float* lse2, int B, int N, int H, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(N, 64), (unsigned)(B * H));
  attn_fwd_parity_kernel<Ops><<<grid, 256, 0, s>>>(qkv, o, lse2, N, H);
  return check_launch(who);
}
template <typename Ops>
int attn_parity_bwd(const char* who, const float* qkv, const float* o, const float* d_o, const float* lse2, float* delta, float* dqkv,
                    int B, int N, int H, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(N, 64), (unsigned)(B * H));
  attn_dq_parity_kernel<Ops><<<grid, 256, 0, s>>>(qkv, o, d_o, lse2, delta, dqkv, N, H);
  attn_dkv_parity_kernel<Ops><<<grid, 256, 0, s>>>(qkv, d_o, lse2, delta, dqkv, N, H);
  return check_launch(who);
}

}  // namespace
}  // namespace avf
