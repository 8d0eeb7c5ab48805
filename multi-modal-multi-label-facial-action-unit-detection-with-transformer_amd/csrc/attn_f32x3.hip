// attn_f32x3.hip - the parity-mode attention core (attn_parity_kernel.hpp) on the bf16 matrix pipe with three-product operands.
//
// Same arithmetic contract as gemm_f32.hip's bf16x3 GEMM (bf16x3.hpp): every fp32 operand of a matrix product is split x = hi + lo
// and a b ~ hi hi + hi lo + lo hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: <= 3 * 2^-16 = 4.6e-5 relative error per
// product in the worst case (4e-6 typical), 3 MFMAs of 16 cycles where the f32-input MFMA kernels of attn_f32_mfma.hip spend 8 of
// 32.  P and dS are split like any other operand.  fp32 storage, no token mask, dim_head 64, q not pre-scaled (the masked /
// bf16-storage / dim_head 32 calls stay on the f32 kernels).  A dim_head-128 parity-mode attention takes the f32-input MFMA
// kernels (attn_f32_mfma.hip) under this arithmetic too: at least as accurate.
#include "attn_parity_kernel.hpp"
#include "bf16x3.hpp"

namespace avf {

namespace {

// The second product needs P (or dS) as the MFMA's B operand: lane (query li, group lg) supplies 8 consecutive k-slots.  The
// reduction index of an MFMA may be permuted freely as long as both operands agree, so k-slot (lg, e) is DEFINED as key
// 16 (e >> 2) + 4 lg + (e & 3): the lane's eight accumulator registers of the two 16-key blocks ARE its B operand - no shuffle,
// no LDS round trip (as_operand is empty).  The other operand (V^T, K^T, Q^T, dO^T) is staged as a transposed image [d][k-slot]
// in that slot order.
// LDS images (bf16; hi, then lo behind it): "row" [32][64] (128-byte rows, fragment = 16 bytes of one row) and "transposed"
// [64][32] (64-byte rows, sw_off); 16-byte chunks XOR-swizzled for ds_read_b128's four non-contiguous 16-lane groups
// (MI355X_MICROARCH.md, LDS).  A tile is split while it is staged.
struct ParityBf16x3 {
  static constexpr int DH = 64, MT = kParityTile, IMG = MT * DH;  // IMG: bf16 elements of one image (4 KiB)
  template <int N>
  __device__ __forceinline__ static uint16_t* images() {  // one array per kernel; an image is its hi and its lo part
    __shared__ __attribute__((aligned(16))) uint16_t lds[N * 2 * IMG];
    return lds;
  }
  template <int I, int N, bool TR>
  __device__ __forceinline__ static uint16_t* image() { return images<N>() + I * 2 * IMG; }
  static constexpr bool kDeltaInDq = true;

  // row image: element offset of 16-byte chunk c8 (8 d) of row r.  Two rows share a 256-byte bank line; a ds_read_b128 group holds
  // the 16 rows of a block at chunk g (rows 0-3, 12-15) or g ^ 1 (rows 4-11): XOR with (r >> 1) ^ [4 <= r < 12] gives the eight
  // rows of one parity eight distinct chunks
  __device__ __forceinline__ static int row_off(int r, int c8) {
    const int q = r & 15;
    return r * DH + ((c8 ^ ((q >> 1) ^ (((q + 4) >> 3) & 1))) << 3);
  }

  // this lane's two fragments (d = 0..31, 32..63) of one row: f[c] = x[row][32 c + 8 lg ..] * scale
  using RowFrags = Frag2[2];
  __device__ __forceinline__ static void load_row(RowFrags& f, const float* row, bool valid, int lg, float scale) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (valid) {
        const float4 a = *reinterpret_cast<const float4*>(row + 32 * c + 8 * lg);
        const float4 b = *reinterpret_cast<const float4*>(row + 32 * c + 8 * lg + 4);
        v[0] = a.x * scale; v[1] = a.y * scale; v[2] = a.z * scale; v[3] = a.w * scale;
        v[4] = b.x * scale; v[5] = b.y * scale; v[6] = b.z * scale; v[7] = b.w * scale;
      }
      f[c] = split8(v);
    }
  }

  // One tile: MT rows x 64 floats of a row-major matrix (row stride ld), loaded in fetch and held in registers over the tile in
  // front.  A thread owns two adjacent rows (2 kp, 2 kp + 1) x four columns: 64-byte row segments per four lanes in the global
  // loads, (row, row + 1) pairs = adjacent k-slots of the transposed image.
  struct TileRegs {
    float4 v0, v1;
  };
  __device__ __forceinline__ static TileRegs fetch(const float* src, int64_t ld, int row0, int nvalid) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int kp = lane >> 2, d0 = 16 * w + 4 * (lane & 3);
    TileRegs t;
    t.v0 = t.v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (2 * kp < nvalid) t.v0 = *reinterpret_cast<const float4*>(src + (int64_t)(row0 + 2 * kp) * ld + d0);
    if (2 * kp + 1 < nvalid) t.v1 = *reinterpret_cast<const float4*>(src + (int64_t)(row0 + 2 * kp + 1) * ld + d0);
    return t;
  }
  template <bool ROWIMG, bool TRIMG>
  __device__ __forceinline__ static void commit(const TileRegs& t, int, int, uint16_t* rowimg, uint16_t* trimg) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int kp = lane >> 2, d0 = 16 * w + 4 * (lane & 3);
    if constexpr (ROWIMG) {
      uint2 h, l;
      split2(t.v0.x, t.v0.y, h.x, l.x);
      split2(t.v0.z, t.v0.w, h.y, l.y);
      int off = row_off(2 * kp, d0 >> 3) + (d0 & 7);
      *reinterpret_cast<uint2*>(rowimg + off) = h;
      *reinterpret_cast<uint2*>(rowimg + IMG + off) = l;
      split2(t.v1.x, t.v1.y, h.x, l.x);
      split2(t.v1.z, t.v1.w, h.y, l.y);
      off = row_off(2 * kp + 1, d0 >> 3) + (d0 & 7);
      *reinterpret_cast<uint2*>(rowimg + off) = h;
      *reinterpret_cast<uint2*>(rowimg + IMG + off) = l;
    }
    if constexpr (TRIMG) {
      // rows 2 kp, 2 kp + 1 -> k-slots: block kb = row >> 4, lane group (row & 15) >> 2, register r = row & 3 (0 or 2 here)
      const int kb = kp >> 3, g = (kp & 7) >> 1, r = 2 * (kp & 1);
      const float a[4] = {t.v0.x, t.v0.y, t.v0.z, t.v0.w}, b[4] = {t.v1.x, t.v1.y, t.v1.z, t.v1.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t h, l;
        split2(a[i], b[i], h, l);
        const int off = sw_off(d0 + i, g) + 4 * kb + r;
        *reinterpret_cast<uint32_t*>(trimg + off) = h;
        *reinterpret_cast<uint32_t*>(trimg + IMG + off) = l;
      }
    }
  }

  // acc[b] (transposed: register r of lane (li, lg) = sum_d img[16 b + 4 lg + r][d] * f[lane's row li][d]) for the two 16-row
  // blocks of a staged row image
  __device__ __forceinline__ static void tile_dot(f32x4_t (&acc)[2], const uint16_t* rowimg, const RowFrags& f, int li, int lg) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int off = row_off(16 * b + li, 4 * c + lg);
        Frag2 a;
        a.h = *reinterpret_cast<const bf16x8_t*>(rowimg + off);
        a.l = *reinterpret_cast<const bf16x8_t*>(rowimg + IMG + off);
        acc[b] = mma_x3(a, f[c], acc[b]);
      }
    }
  }

  __device__ __forceinline__ static void as_operand(f32x4_t&) {}

  // out[db] (transposed: register r of lane (li, lg) = column 16 db + 4 lg + r of this lane's row li) += sum over the tile's 32
  // rows of img^T[column][row] * w[row][lane's row li]; w = the lane's eight accumulator registers of the two blocks, as they stand
  __device__ __forceinline__ static void tile_acc(f32x4_t (&out)[4], const uint16_t* trimg, const f32x4_t (&w)[2], int li, int lg) {
    const float v[8] = {w[0][0], w[0][1], w[0][2], w[0][3], w[1][0], w[1][1], w[1][2], w[1][3]};
    const Frag2 b = split8(v);
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const int off = sw_off(16 * db + li, lg);
      Frag2 a;
      a.h = *reinterpret_cast<const bf16x8_t*>(trimg + off);
      a.l = *reinterpret_cast<const bf16x8_t*>(trimg + IMG + off);
      out[db] = mma_x3(a, b, out[db]);
    }
  }
};

}  // namespace

// calls these kernels take: the bf16x3 arithmetic asked for, fp32 storage, no token mask, dim_head 64, q not pre-scaled, 16-byte rows
bool attn_f32x3_takes(int dtype, int dh, bool masked, int /*H*/, bool aligned16, bool q_prescaled, int arith) {
  return arith == 1 && dtype == AVF_F32 && !masked && !q_prescaled && dh == ParityBf16x3::DH && aligned16;
}
bool attn_f32x3_ok(int dtype, int dh, const void* keep, int H, const void* qkv, const void* other, bool q_prescaled, int arith) {
  return attn_f32x3_takes(dtype, dh, keep != nullptr, H, attn_aligned16(qkv, other), q_prescaled, arith);
}

int attn_fwd_f32x3(const float* qkv, float* o, float* lse2, int B, int N, int H, hipStream_t s) {
  return attn_parity_fwd<ParityBf16x3>("attn_fwd_parity_kernel (bf16x3)", qkv, o, lse2, B, N, H, s);
}

int attn_bwd_f32x3(const float* qkv, const float* o, const float* d_o, const float* lse2, float* delta, float* dqkv, int B, int N,
                   int H, hipStream_t s) {
  return attn_parity_bwd<ParityBf16x3>("attn_dq / dkv_parity_kernel (bf16x3)", qkv, o, d_o, lse2, delta, dqkv, B, N, H, s);
}

}  // namespace avf
