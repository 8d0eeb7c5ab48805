// clip_kernels.hpp - the device code that clip.hip (an assembled clip) and clip_bank.hip (a resident frame bank) share: the
// normalise kernel as a template over the frame source (clip_source.hpp).  clip.hip describes the kernel.
#pragma once
#include "clip_source.hpp"

namespace avf {
namespace {

constexpr int CLIP_THREADS = 256;
constexpr int CLIP_TILE = 2048;                  // pixels per workgroup
constexpr int CLIP_STAGE = CLIP_TILE * 4 + 32;   // bytes: C <= 4, + the shift (< 16) rounded up to whole chunks at both ends
constexpr int CLIP_MAX_C = 4;

template <typename T>
__device__ __forceinline__ void store_vec(T* p, const float* x);
template <>
__device__ __forceinline__ void store_vec<float>(float* p, const float* x) {
  *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
}
template <>
__device__ __forceinline__ void store_vec<bf16>(bf16* p, const float* x) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]),
                                            pack_bf16x2(x[6], x[7]));
}
template <typename T>
__device__ __forceinline__ void load_vec(const T* p, float* x);
template <>
__device__ __forceinline__ void load_vec<float>(const float* p, float* x) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
}
template <>
__device__ __forceinline__ void load_vec<bf16>(const bf16* p, float* x) {
  float v[8];
  unpack8(*reinterpret_cast<const uint4*>(p), v);
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = v[i];
}

// elements in front of the first 16-byte aligned one of p (p is aligned to its element), at most n
template <typename T>
__device__ __forceinline__ int head_elems(const T* p, int n) {
  const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(T));
  return h < n ? h : n;
}

template <typename OutT, typename Source>
__global__ __launch_bounds__(CLIP_THREADS) void clip_normalize_kernel(
    const Source src, OutT* __restrict__ dst, const float* __restrict__ lut,
    const uint8_t* __restrict__ flip, int64_t T, int64_t H, int64_t W, int C, int k, int rows_per_tile, int cols_per_tile,
    int row_tiles, int col_tiles, int layout) {
  constexpr int VEC = 16 / (int)sizeof(OutT);
  __shared__ __attribute__((aligned(16))) uint8_t stage[CLIP_STAGE];
  __shared__ float lut_s[CLIP_MAX_C * 256];
  const int tid = threadIdx.x;
  const unsigned tiles_per_frame = (unsigned)row_tiles * (unsigned)col_tiles;
  const int64_t frame = blockIdx.x / tiles_per_frame;
  const int tile = (int)(blockIdx.x % tiles_per_frame);
  const int rt = tile / col_tiles, ct = tile - rt * col_tiles;
  const int64_t r0 = (int64_t)rt * rows_per_tile, w0 = (int64_t)ct * cols_per_tile;
  const int nr = (int)(H - r0 < rows_per_tile ? H - r0 : rows_per_tile);
  const int s = (int)(W - w0 < cols_per_tile ? W - w0 : cols_per_tile);   // pixels of one row of the tile
  const int n = nr * s;                                                   // <= CLIP_TILE (more than one row: s == W)
  if (n <= 0) return;   // (never: the host's tiling leaves no empty tile; uniform over the workgroup)
  const int64_t b = frame / T, t = frame - b * T;
  const bool mirrored = flip != nullptr && flip[b] != 0;
  const int64_t out0 = r0 * W + w0;                                       // first pixel of the tile in an output plane
  const int64_t in0 = r0 * W + (mirrored ? W - w0 - s : w0);              // ... and in the source frame

  for (int i = tid; i < k * 256; i += CLIP_THREADS) lut_s[i] = lut[(C - k) * 256 + i];

  // the tile's source bytes, or zeros for a black slot (its pixels are lut[c][0]); nothing of a black slot is read
  const uint8_t* fr = src.frame(b, t, T, H * W * C);
  const uint8_t* first = fr + in0 * C;
  const int shift = fr != nullptr ? (int)(reinterpret_cast<uintptr_t>(first) & 15u) : 0;
  const int chunks = (shift + n * C + 15) >> 4;
  if (fr != nullptr)
    stage_chunks<CLIP_THREADS>(stage, first, chunks, src.base(), src.bytes(), tid);
  else
    zero_chunks<CLIP_THREADS>(stage, chunks, tid);
  __syncthreads();

  const int64_t plane_elems = H * W;
  for (int ci = 0; ci < k; ++ci) {
    const int64_t plane = layout == AVF_CLIP_CTHW ? (b * k + ci) * T + t : (b * T + t) * k + ci;
    OutT* __restrict__ o = dst + plane * plane_elems + out0;
    const float* lt = lut_s + ci * 256;
    const uint8_t* sg = stage + shift + (C - k + ci);
    // source pixel (local to the tile) of output pixel j: the same, or the same row read backwards
    auto one = [&](int j) -> float {
      int sl = j;
      if (mirrored) {
        const int r = j / s;
        sl = r * s + (s - 1 - (j - r * s));
      }
      return lt[sg[sl * C]];
    };
    const int head = head_elems(o, n);
    const int nvec = (n - head) / VEC, tail = (n - head) - nvec * VEC;
    if (tid < head) o[tid] = from_f32<OutT>(one(tid));
    if (tid < tail) o[head + nvec * VEC + tid] = from_f32<OutT>(one(head + nvec * VEC + tid));
    if (!mirrored) {
      for (int v = tid; v < nvec; v += CLIP_THREADS) {
        const int j0 = head + v * VEC;
        float x[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) x[i] = lt[sg[(j0 + i) * C]];
        store_vec<OutT>(o + j0, x);
      }
    } else {
      for (int v = tid; v < nvec; v += CLIP_THREADS) {
        const int j0 = head + v * VEC;
        const int r = j0 / s;
        int wl = j0 - r * s, row = r * s;   // a vector may run over the end of a row
        float x[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          x[i] = lt[sg[(row + s - 1 - wl) * C]];
          if (++wl == s) {
            wl = 0;
            row += s;
          }
        }
        store_vec<OutT>(o + j0, x);
      }
    }
  }
}

// what both entry points ask of the clip's shape; frames * (H * W) * 16 bytes must fit int64
int clip_shape_ok(const char* who, int64_t B, int64_t T, int64_t H, int64_t W, int C) {
  AVF_REQUIRE(B >= 1, "%s: B is %lld, below 1", who, (long long)B);
  AVF_REQUIRE(T >= 1, "%s: T is %lld, below 1", who, (long long)T);
  AVF_REQUIRE(H >= 1, "%s: H is %lld, below 1", who, (long long)H);
  AVF_REQUIRE(W >= 1, "%s: W is %lld, below 1", who, (long long)W);
  AVF_REQUIRE(C >= 1 && C <= CLIP_MAX_C, "%s: C is %d, outside 1..%d", who, C, CLIP_MAX_C);
  const int64_t lim = 1LL << 31;
  AVF_REQUIRE(B < lim && T < lim && H < lim && W < lim && B * T < lim, "%s: B / T / H / W is too large", who);
  AVF_REQUIRE(B * T <= (INT64_MAX / 16) / (H * W), "%s: B * T * H * W is too large", who);
  return 0;
}

// what every entry point that writes planes asks of its output side
int clip_output_ok(const char* who, int C, int k, const void* dst, int out_dtype, int layout) {
  AVF_REQUIRE(k >= 1 && k <= C, "%s: k is %d, outside 1..C = %d", who, k, C);
  AVF_REQUIRE(out_dtype == AVF_F32 || out_dtype == AVF_BF16, "%s: out_dtype is %d, neither AVF_F32 nor AVF_BF16", who,
              out_dtype);
  AVF_REQUIRE(layout == AVF_CLIP_CTHW || layout == AVF_CLIP_TCHW, "%s: layout is %d, neither cthw (0) nor tchw (1)", who,
              layout);
  AVF_REQUIRE(((uintptr_t)dst & (out_dtype == AVF_F32 ? 3u : 1u)) == 0, "%s: dst is not aligned to its element", who);
  return 0;
}

// the checks of the output side, the tiling and the launch, for either source (the caller has checked its pointers and the shape)
template <typename Source>
int clip_normalize_launch(const char* who, const Source& from, int64_t B, int64_t T, int64_t H, int64_t W, int C, int k,
                          const float* lut, const uint8_t* flip, void* dst, int out_dtype, int layout, hipStream_t s) {
  AVF_TRY(clip_output_ok(who, C, k, dst, out_dtype, layout));
  // whole rows per tile where a row fits (then rows are contiguous in the source and in the planes), else row segments
  int rows_per_tile = 1, cols_per_tile, row_tiles, col_tiles = 1;
  if (W <= CLIP_TILE) {
    const int64_t fit = CLIP_TILE / W;
    row_tiles = (int)ceil_div(H, fit);
    rows_per_tile = (int)ceil_div(H, row_tiles);
    cols_per_tile = (int)W;
  } else {
    row_tiles = (int)H;
    col_tiles = (int)ceil_div(W, CLIP_TILE);
    cols_per_tile = (int)ceil_div(W, col_tiles);
  }
  const int64_t tiles = (int64_t)row_tiles * col_tiles;
  AVF_REQUIRE(tiles < (1LL << 31), "%s: H * W gives too many tiles", who);
  const int64_t blocks = B * T * tiles;
  AVF_REQUIRE(blocks < (1LL << 31), "%s: B * T * H * W gives too many tiles", who);
  if (out_dtype == AVF_F32)
    clip_normalize_kernel<float><<<(unsigned)blocks, CLIP_THREADS, 0, s>>>(from, (float*)dst, lut, flip, T, H, W, C, k,
                                                                           rows_per_tile, cols_per_tile, row_tiles, col_tiles, layout);
  else
    clip_normalize_kernel<bf16><<<(unsigned)blocks, CLIP_THREADS, 0, s>>>(from, (bf16*)dst, lut, flip, T, H, W, C, k,
                                                                          rows_per_tile, cols_per_tile, row_tiles, col_tiles, layout);
  return check_launch("clip_normalize_kernel");
}

}  // namespace
}  // namespace avf
