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
// The normalise kernel is a template over where a frame comes from (clip_source.hpp) and lives in clip_kernels.hpp, which
// clip_bank.hip instantiates over a resident frame bank; here the source is the assembled clip.
//
// gfx950 resources (hipcc -O3, --save-temps): see DESIGN.md section 9.
#include "clip_kernels.hpp"

namespace avf {
namespace {

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

}  // namespace
}  // namespace avf

extern "C" int avf_clip_normalize(const uint8_t* src, int64_t B, int64_t T, int64_t H, int64_t W, int C, int k, const float* lut,
                                  const uint8_t* flip, void* dst, int out_dtype, int layout, void* stream) {
  using namespace avf;
  AVF_REQUIRE(src, "clip_normalize: src is null");
  AVF_REQUIRE(lut, "clip_normalize: lut is null");
  AVF_REQUIRE(dst, "clip_normalize: dst is null");
  AVF_TRY(clip_shape_ok("clip_normalize", B, T, H, W, C));
  const ClipTensorSource from{src, B * T * H * W * C};
  return clip_normalize_launch("clip_normalize", from, B, T, H, W, C, k, lut, flip, dst, out_dtype, layout, (hipStream_t)stream);
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
