// clip.hip - the video stream's wire format on the device: uint8 clips [B, T, H, W, C] <-> normalised planes
// (dataloader/clip_transforms.py:31-45 NumpyToTensor, 59-93 Normalize, 111-128 RandomClipFlip; aff2compdataset.py:69-77;
// the model's clip[:, -num_channels:] and permute(0, 2, 1, 3, 4), models/sformer.py:365-373).
//
// avf_clip_normalize, one launch.  A workgroup owns one tile of one frame: up to CLIP_TILE pixels that are contiguous both in
// the interleaved source and in every output plane - whole rows where a row fits the tile (W <= CLIP_TILE), else a segment of
// one row.  It
//   1. copies the k * 256 table entries it needs into LDS;
//   2. stages the tile's n * C source bytes in LDS with aligned 16-byte loads.  The byte range starts wherever it starts
//      (W * C is rarely a multiple of 16): the loads cover the 16-byte chunks around it and the range keeps its offset
//      (`shift`) inside the staging buffer.  Only the first and the last chunk of the WHOLE tensor can reach outside it; those
//      two are read byte by byte with a bounds check;
//   3. per kept channel, stores the plane segment: each lane 16 bytes (4 fp32 / 8 bf16 pixels) of ONE plane, consecutive
//      lanes consecutive addresses.  The plane segment starts wherever it starts too (H * W, W need not be multiples of the
//      vector): up to VEC - 1 scalar stores in front of the first aligned vector and behind the last.
// A mirrored clip (flip[b] != 0, read on the device) changes the source range of a row segment and reverses the READ index
// within each row of the tile; its stores are the same as an unmirrored clip's.  cthw and tchw differ in the plane's base.
// The value is lut[channel][byte], nothing is computed: the table is the caller's, built with the reference's op sequence.
//
// avf_clip_denormalize, one launch, the other way round: vector loads of each plane segment,
// trunc(clamp(((x * std) + mean) * 255, 0, 255)) with three separately rounded operations (#pragma clang fp contract(off):
// no fused multiply-add), bytes interleaved in LDS, aligned 16-byte stores of the tile's byte range (partial chunks byte by byte).
//
// gfx950 resources (hipcc -O3, --save-temps): see DESIGN.md section 9.
#include "common.hpp"

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

template <typename OutT>
__global__ __launch_bounds__(CLIP_THREADS) void clip_normalize_kernel(
    const uint8_t* __restrict__ src, int64_t src_bytes, OutT* __restrict__ dst, const float* __restrict__ lut,
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

  const uint8_t* first = src + (frame * H * W + in0) * C;
  const int shift = (int)(reinterpret_cast<uintptr_t>(first) & 15u);
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(first) - (uintptr_t)shift;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(src), hi = lo + (uintptr_t)src_bytes;
  const int chunks = (shift + n * C + 15) >> 4;
  for (int i = tid; i < chunks; i += CLIP_THREADS) {
    const uintptr_t a = a0 + 16u * (uintptr_t)i;
    uint4 v;
    if (a >= lo && a + 16u <= hi) {
      v = *reinterpret_cast<const uint4*>(a);
    } else {  // the first or the last chunk of the whole tensor: only the bytes that belong to it
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (a + q >= lo && a + q < hi) w[q >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t*>(a + q)) << (8 * (q & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(stage + 16 * i) = v;
  }
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

__device__ __forceinline__ uint8_t denorm_one(float x, float sd, float m) {
  // mul_, add_, mul(255): three roundings.  hipcc contracts a * b + c into one fused multiply-add by default - also through
  // __fmul_rn / __fadd_rn, which its headers define as plain operators - so contraction is switched off for this function
#pragma clang fp contract(off)
  float v = ((x * sd) + m) * 255.0f;
  v = v > 0.0f ? v : 0.0f;                                        // NaN -> 0
  v = v < 255.0f ? v : 255.0f;
  return (uint8_t)(int)v;
}

template <typename InT>
__global__ __launch_bounds__(CLIP_THREADS) void clip_denormalize_kernel(const InT* __restrict__ src, uint8_t* __restrict__ dst,
                                                                        const float* __restrict__ mean,
                                                                        const float* __restrict__ std, int64_t T, int64_t P,
                                                                        int C, int tiles_per_frame, int layout) {
  constexpr int VEC = 16 / (int)sizeof(InT);
  __shared__ __attribute__((aligned(16))) uint8_t stage[CLIP_STAGE];
  const int tid = threadIdx.x;
  const int64_t frame = blockIdx.x / (unsigned)tiles_per_frame;
  const int64_t p0 = (int64_t)(blockIdx.x % (unsigned)tiles_per_frame) * CLIP_TILE;
  const int n = (int)(P - p0 < CLIP_TILE ? P - p0 : CLIP_TILE);
  const int64_t b = frame / T, t = frame - b * T;
  uint8_t* first = dst + (frame * P + p0) * C;
  const int shift = (int)(reinterpret_cast<uintptr_t>(first) & 15u);

  for (int c = 0; c < C; ++c) {
    const int64_t plane = layout == AVF_CLIP_CTHW ? (b * C + c) * T + t : (b * T + t) * C + c;
    const InT* __restrict__ in = src + plane * P + p0;
    const float sd = std[c], m = mean[c];
    uint8_t* sg = stage + shift + c;
    const int head = head_elems(in, n);
    const int nvec = (n - head) / VEC, tail = (n - head) - nvec * VEC;
    if (tid < head) sg[tid * C] = denorm_one(to_f32<InT>(in[tid]), sd, m);
    if (tid < tail) {
      const int j = head + nvec * VEC + tid;
      sg[j * C] = denorm_one(to_f32<InT>(in[j]), sd, m);
    }
    for (int v = tid; v < nvec; v += CLIP_THREADS) {
      const int j0 = head + v * VEC;
      float x[VEC];
      load_vec<InT>(in + j0, x);
#pragma unroll
      for (int i = 0; i < VEC; ++i) sg[(j0 + i) * C] = denorm_one(x[i], sd, m);
    }
  }
  __syncthreads();

  const int nbytes = n * C;
  const int chunks = (shift + nbytes + 15) >> 4;
  uint8_t* a0 = first - shift;
  for (int i = tid; i < chunks; i += CLIP_THREADS) {
    const int off = 16 * i - shift;   // of the chunk's first byte inside the tile's byte range
    if (off >= 0 && off + 16 <= nbytes) {
      *reinterpret_cast<uint4*>(a0 + 16 * i) = *reinterpret_cast<const uint4*>(stage + 16 * i);
    } else {  // the tile's first / last chunk is shared with its neighbours: only the bytes that are this tile's
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (off + q >= 0 && off + q < nbytes) a0[16 * i + q] = stage[16 * i + q];
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

}  // namespace
}  // namespace avf

extern "C" int avf_clip_normalize(const uint8_t* src, int64_t B, int64_t T, int64_t H, int64_t W, int C, int k, const float* lut,
                                  const uint8_t* flip, void* dst, int out_dtype, int layout, void* stream) {
  using namespace avf;
  AVF_REQUIRE(src, "clip_normalize: src is null");
  AVF_REQUIRE(lut, "clip_normalize: lut is null");
  AVF_REQUIRE(dst, "clip_normalize: dst is null");
  AVF_TRY(clip_shape_ok("clip_normalize", B, T, H, W, C));
  AVF_REQUIRE(k >= 1 && k <= C, "clip_normalize: k is %d, outside 1..C = %d", k, C);
  AVF_REQUIRE(out_dtype == AVF_F32 || out_dtype == AVF_BF16, "clip_normalize: out_dtype is %d, neither AVF_F32 nor AVF_BF16",
              out_dtype);
  AVF_REQUIRE(layout == AVF_CLIP_CTHW || layout == AVF_CLIP_TCHW, "clip_normalize: layout is %d, neither cthw (0) nor tchw (1)",
              layout);
  AVF_REQUIRE(((uintptr_t)dst & (out_dtype == AVF_F32 ? 3u : 1u)) == 0, "clip_normalize: dst is not aligned to its element");
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
  AVF_REQUIRE(tiles < (1LL << 31), "clip_normalize: H * W gives too many tiles");
  const int64_t blocks = B * T * tiles;
  AVF_REQUIRE(blocks < (1LL << 31), "clip_normalize: B * T * H * W gives too many tiles");
  const int64_t src_bytes = B * T * H * W * C;
  hipStream_t s = (hipStream_t)stream;
  if (out_dtype == AVF_F32)
    clip_normalize_kernel<float><<<(unsigned)blocks, CLIP_THREADS, 0, s>>>(src, src_bytes, (float*)dst, lut, flip, T, H, W, C, k,
                                                                           rows_per_tile, cols_per_tile, row_tiles, col_tiles, layout);
  else
    clip_normalize_kernel<bf16><<<(unsigned)blocks, CLIP_THREADS, 0, s>>>(src, src_bytes, (bf16*)dst, lut, flip, T, H, W, C, k,
                                                                          rows_per_tile, cols_per_tile, row_tiles, col_tiles, layout);
  return check_launch("clip_normalize_kernel");
}

extern "C" int avf_clip_denormalize(const void* src, int in_dtype, int layout, int64_t B, int64_t T, int64_t H, int64_t W, int C,
                                    const float* mean, const float* std, uint8_t* dst, void* stream) {
  using namespace avf;
  AVF_REQUIRE(src, "clip_denormalize: src is null");
  AVF_REQUIRE(mean, "clip_denormalize: mean is null");
  AVF_REQUIRE(std, "clip_denormalize: std is null");
  AVF_REQUIRE(dst, "clip_denormalize: dst is null");
  AVF_TRY(clip_shape_ok("clip_denormalize", B, T, H, W, C));
  AVF_REQUIRE(in_dtype == AVF_F32 || in_dtype == AVF_BF16, "clip_denormalize: in_dtype is %d, neither AVF_F32 nor AVF_BF16",
              in_dtype);
  AVF_REQUIRE(layout == AVF_CLIP_CTHW || layout == AVF_CLIP_TCHW, "clip_denormalize: layout is %d, neither cthw (0) nor tchw (1)",
              layout);
  AVF_REQUIRE(((uintptr_t)src & (in_dtype == AVF_F32 ? 3u : 1u)) == 0, "clip_denormalize: src is not aligned to its element");
  const int64_t P = H * W;
  const int64_t tiles = ceil_div(P, CLIP_TILE);
  const int64_t blocks = B * T * tiles;
  AVF_REQUIRE(tiles < (1LL << 31) && blocks < (1LL << 31), "clip_denormalize: B * T * H * W gives too many tiles");
  hipStream_t s = (hipStream_t)stream;
  if (in_dtype == AVF_F32)
    clip_denormalize_kernel<float><<<(unsigned)blocks, CLIP_THREADS, 0, s>>>((const float*)src, dst, mean, std, T, P, C, (int)tiles,
                                                                             layout);
  else
    clip_denormalize_kernel<bf16><<<(unsigned)blocks, CLIP_THREADS, 0, s>>>((const bf16*)src, dst, mean, std, T, P, C, (int)tiles,
                                                                            layout);
  return check_launch("clip_denormalize_kernel");
}
