// attn_f32_mfma.hip - the parity-mode attention core (attn_parity_kernel.hpp) on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
//
// fp32 operands, fp32 products, fp32 accumulation: the arithmetic of attn_f32.hip's one-lane-per-query VALU kernels (which took
// 13.4 ms of a 27.8 ms step at C2, 9 TFLOP/s) on the f32-input MFMA, whose product-sum is a k-ordered fmaf chain: same precision
// class, different summation order.  No token mask, fp32 storage and raw q only (the masked, the bf16-storage and a pre-scaled
// call stay on attn_f32.hip), dim_head 32, 64 or 128.
#include "attn_dispatch.hpp"
#include "attn_parity_kernel.hpp"

namespace avf {

namespace {

#define AVF_MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// The reduction index of the first product is permuted - k-step (c, e) of lane group g carries d = 16 c + 4 g + e - so that a
// lane fetches its four k-steps of a chunk with ONE 16-byte LDS read; both operands use the same permutation.
// LDS images: a row-fragment copy with row stride DH + 4 floats (16-byte reads of 16 consecutive rows: conflict-free) and, where a
// tile is also read transposed, a second copy with row stride DH + 16 (4-byte reads of 4 rows x 16 columns: conflict-free).
template <int DH_>
struct ParityF32Mfma {
  static constexpr int DH = DH_, MT = kParityTile, LR = DH + 4, LT = DH + 16;
  template <int I, int N, bool TR>
  __device__ __forceinline__ static float* image() {  // one array per image
    __shared__ __attribute__((aligned(16))) float img[MT * (TR ? LT : LR)];
    return img;
  }
  static constexpr bool kDeltaInDq = false;

  // this lane's fragment registers of one of its wave's 16 rows: f[c][e] = x[row][16 c + 4 lg + e] * scale (zeros past the end)
  using RowFrags = float[DH / 16][4];
  __device__ __forceinline__ static void load_row(RowFrags& f, const float* row, bool valid, int lg, float scale) {
#pragma unroll
    for (int c = 0; c < DH / 16; ++c) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) v = *reinterpret_cast<const float4*>(row + 16 * c + 4 * lg);
      f[c][0] = v.x * scale; f[c][1] = v.y * scale; f[c][2] = v.z * scale; f[c][3] = v.w * scale;
    }
  }

  // a tile goes global -> LDS between the barriers: fetch only records where it is, commit copies MT rows x DH floats
  struct TileRegs {
    const float* src;
    int64_t ld;
  };
  __device__ __forceinline__ static TileRegs fetch(const float* src, int64_t ld, int, int) { return TileRegs{src, ld}; }
  template <bool ROWIMG, bool TRIMG>
  __device__ __forceinline__ static void commit(const TileRegs& t, int row0, int nvalid, float* rowimg, float* trimg) {
    constexpr int V = DH / 4;
    for (int i = threadIdx.x; i < MT * V; i += 256) {
      const int r = i / V, c = (i - r * V) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nvalid) v = *reinterpret_cast<const float4*>(t.src + (int64_t)(row0 + r) * t.ld + c);
      if constexpr (ROWIMG) *reinterpret_cast<float4*>(rowimg + r * LR + c) = v;
      if constexpr (TRIMG) *reinterpret_cast<float4*>(trimg + r * LT + c) = v;
    }
  }

  // acc[b] (16 x 16, transposed: acc[b][r] of lane (li, lg) = sum_d img[16 b + 4 lg + r][d] * f[lane's row li][d]) for the two
  // 16-row blocks of a staged tile: A operand = the tile's rows (one 16-byte read per chunk), B operand = the lane's registers
  __device__ __forceinline__ static void tile_dot(f32x4_t (&acc)[2], const float* rowimg, const RowFrags& f, int li, int lg) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DH / 16; ++c) {
        const float4 a = *reinterpret_cast<const float4*>(rowimg + (16 * b + li) * LR + 16 * c + 4 * lg);
        acc[b] = AVF_MFMA_F32(a.x, f[c][0], acc[b]);
        acc[b] = AVF_MFMA_F32(a.y, f[c][1], acc[b]);
        acc[b] = AVF_MFMA_F32(a.z, f[c][2], acc[b]);
        acc[b] = AVF_MFMA_F32(a.w, f[c][3], acc[b]);
      }
    }
  }

  // A 16 x 16 block of P (or dS) becomes the B operand of the next product by the 4 x 4 transpose between the register index
  // and the lane group (tr4x4: two v_permlane16_swap + two v_permlane32_swap): register m of lane (li, lg) then holds
  // P[key 4 m + lg][query li], exactly what k-step m (keys 4 m .. 4 m + 3) of   O^T += V^T P   asks of that lane.
  __device__ __forceinline__ static void as_operand(f32x4_t& v) {
    uint32_t a[4] = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    tr4x4(a);
    v[0] = __uint_as_float(a[0]); v[1] = __uint_as_float(a[1]); v[2] = __uint_as_float(a[2]); v[3] = __uint_as_float(a[3]);
  }

  // out[db] (transposed: out[db][r] of lane (li, lg) = column 16 db + 4 lg + r of this lane's row li) += sum over the tile's 32
  // rows of trimg[row][column] * w[row][lane's row li], w given as the two TRANSPOSED 16 x 16 blocks wt[b] (as_operand)
  __device__ __forceinline__ static void tile_acc(f32x4_t (&out)[DH / 16], const float* trimg, const f32x4_t (&wt)[2], int li, int lg) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int db = 0; db < DH / 16; ++db)
          out[db] = AVF_MFMA_F32(trimg[(16 * b + 4 * m + lg) * LT + 16 * db + li], wt[b][m], out[db]);
  }
};

}  // namespace

// shapes these kernels take: fp32 storage, no token mask, q not pre-scaled, dim_head 32, 64 or 128, 16-byte aligned rows
bool attn_f32_mfma_takes(int dtype, int dh, bool masked, int H, bool aligned16, bool q_prescaled) {
  return dtype == AVF_F32 && !masked && !q_prescaled && (dh == 32 || dh == 64 || dh == 128) && aligned16 && ((H * dh) % 4) == 0;
}
bool attn_f32_mfma_ok(int dtype, int dh, const void* keep, int H, const void* qkv, const void* other, bool q_prescaled) {
  return attn_f32_mfma_takes(dtype, dh, keep != nullptr, H, attn_aligned16(qkv, other), q_prescaled);
}

int attn_fwd_f32_mfma(const float* qkv, float* o, float* lse2, int B, int N, int H, int dh, hipStream_t s) {
  return with_mfma_dim_head(dh, "attn_fwd_f32_mfma", [&](auto d) {
    return attn_parity_fwd<ParityF32Mfma<decltype(d)::value>>("attn_fwd_parity_kernel (f32 MFMA)", qkv, o, lse2, B, N, H, s);
  });
}

int attn_bwd_f32_mfma(const float* qkv, const float* d_o, const float* lse2, const float* delta, float* dqkv, int B, int N, int H,
                      int dh, hipStream_t s) {
  return with_mfma_dim_head(dh, "attn_bwd_f32_mfma", [&](auto d) {  // (delta is only read: kDeltaInDq is false)
    return attn_parity_bwd<ParityF32Mfma<decltype(d)::value>>("attn_dq / dkv_parity_kernel (f32 MFMA)", qkv, nullptr, d_o, lse2,
                                                              const_cast<float*>(delta), dqkv, B, N, H, s);
  });
}

}  // namespace avf
