// clip_bank.hip - clips assembled on the device from a resident frame bank: bank uint8 [F, H, W, C], video_db_nr int32 [F],
// present uint8 [F] (or null) and index int64 [B] -> the clip of every sample, by the data loader's rule
// (dataloader/aff2compdataset.py:122-156; clip_source.hpp restates it and ClipBankSource::frame applies it).  Only index [B]
// travels per step; neighbouring samples share T - 1 of their T frames, which the bank holds once.
//
// avf_clip_gather              one launch: bank -> uint8 clip [B, T, H, W, C].  A workgroup owns one tile of one slot: up to
//                              GATHER_TILE consecutive bytes of the frame.  Where the tile's source and destination ranges sit
//                              alike in their 16-byte chunks, each lane copies whole chunks, load to store.  Where they do not
//                              (a frame of 75 bytes puts every second frame off a 16-byte boundary), the source range is staged in
//                              LDS with aligned 16-byte loads as clip.hip stages its tiles, and each aligned 16-byte store takes
//                              its bytes from five LDS words.  The first and last chunk of a tile, shared with the neighbouring
//                              tiles, are written byte by byte.  A black slot stores zeros and reads nothing.
// avf_clip_gather_normalize    one launch: bank -> normalised planes, clip.hip's clip_normalize_kernel with the bank as its source.
//                              No uint8 clip exists.  A black slot is lut[c][0].
// avf_clip_gather_autoaugment  one launch: bank -> augmented uint8 clip, augment.hip's clip_autoaugment_kernel with the bank as its
//                              source.  A black slot goes through its two plan slots like any other frame.
// avf_clip_gather_autoaugment_normalize
//                              one launch: bank -> augmented, mirrored, normalised planes - the reference's aug_clip_transform
//                              (dataloader/aff2compdataset.py:72-74, 163-164) -, the same kernel with the bank as its source and
//                              the planes as its sink.  No uint8 clip exists.  A black slot goes through its two plan slots and
//                              is THEN normalised: inverted it is lut[c][255].
//
// The file is compiled with -ffp-contract=off, like augment.hip.  gfx950 resources: see DESIGN.md section 9.
#include "augment_kernels.hpp"
#include "clip_kernels.hpp"

namespace avf {
namespace {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_TILE = 16384;                 // bytes per workgroup, a multiple of 16
constexpr int GATHER_STAGE = GATHER_TILE + 48;     // + the shift (< 16) in whole chunks at both ends, + the fifth word of the last read

__global__ __launch_bounds__(GATHER_THREADS) void clip_gather_kernel(const ClipBankSource src, uint8_t* __restrict__ dst, int64_t T,
                                                                     int64_t frame_bytes, int tile_bytes, int tiles) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[GATHER_STAGE];
  const int tid = threadIdx.x;
  const int64_t frame = blockIdx.x / (unsigned)tiles;
  const int64_t o0 = (int64_t)(blockIdx.x % (unsigned)tiles) * tile_bytes;
  const int n = (int)(frame_bytes - o0 < tile_bytes ? frame_bytes - o0 : tile_bytes);
  if (n <= 0) return;   // (never: the host's tiling leaves no empty tile; uniform over the workgroup)
  const int64_t b = frame / T, t = frame - b * T;
  const uint8_t* fr = src.frame(b, t, T, frame_bytes);
  uint8_t* out = dst + frame * frame_bytes + o0;
  const int dshift = (int)(reinterpret_cast<uintptr_t>(out) & 15u);
  uint8_t* a0 = out - dshift;
  const int chunks = (dshift + n + 15) >> 4;

  if (fr == nullptr) {
    for (int i = tid; i < chunks; i += GATHER_THREADS) {
      const int off = 16 * i - dshift;   // of the chunk's first byte inside the tile's byte range
      if (off >= 0 && off + 16 <= n) {
        *reinterpret_cast<uint4*>(a0 + 16 * i) = make_uint4(0u, 0u, 0u, 0u);
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (off + q >= 0 && off + q < n) a0[16 * i + q] = 0;
      }
    }
    return;
  }

  const uint8_t* in = fr + o0;
  const int sshift = (int)(reinterpret_cast<uintptr_t>(in) & 15u);
  if (sshift == dshift) {
    const uint8_t* s0 = in - sshift;
    for (int i = tid; i < chunks; i += GATHER_THREADS) {
      const int off = 16 * i - dshift;
      if (off >= 0 && off + 16 <= n) {   // the whole chunk is inside the tile, on both sides
        *reinterpret_cast<uint4*>(a0 + 16 * i) = *reinterpret_cast<const uint4*>(s0 + 16 * i);
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (off + q >= 0 && off + q < n) a0[16 * i + q] = s0[16 * i + q];
      }
    }
    return;
  }

  stage_chunks<GATHER_THREADS>(stage, in, (sshift + n + 15) >> 4, src.base(), src.bytes(), tid);   // byte j at stage[sshift + j]
  __syncthreads();
  const uint32_t* words = reinterpret_cast<const uint32_t*>(stage);
  for (int i = tid; i < chunks; i += GATHER_THREADS) {
    const int off = 16 * i - dshift;
    if (off >= 0 && off + 16 <= n) {
      const int p = sshift + off;        // the chunk's 16 bytes start at stage[p]: words p / 4 .. p / 4 + 4, shifted by p % 4 bytes
      const int w0 = p >> 2, r = 8 * (p & 3);
      uint32_t x[5], y[4];
#pragma unroll
      for (int j = 0; j < 5; ++j) x[j] = words[w0 + j];                    // 4 * (w0 + 5) <= sshift + n + 4 < GATHER_STAGE
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = (uint32_t)((((uint64_t)x[j + 1] << 32) | (uint64_t)x[j]) >> r);
      *reinterpret_cast<uint4*>(a0 + 16 * i) = make_uint4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (off + q >= 0 && off + q < n) a0[16 * i + q] = stage[sshift + off + q];
    }
  }
}

// what the entry points ask of the bank, the index and the rule; fills the source
int bank_source(const char* who, const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present, const int64_t* index,
                int64_t F, int64_t T, int64_t d, int64_t H, int64_t W, int C, ClipBankSource* out) {
  AVF_REQUIRE(bank, "%s: bank is null", who);
  AVF_REQUIRE(video_db_nr, "%s: video_db_nr is null", who);
  AVF_REQUIRE(index, "%s: index is null", who);
  AVF_REQUIRE(((uintptr_t)video_db_nr & 3u) == 0, "%s: video_db_nr is not aligned to its element", who);
  AVF_REQUIRE(((uintptr_t)index & 7u) == 0, "%s: index is not aligned to its element", who);
  AVF_REQUIRE(F >= 1, "%s: F is %lld, below 1", who, (long long)F);
  AVF_REQUIRE(d >= 1, "%s: d is %lld, below 1", who, (long long)d);
  const int64_t lim = 1LL << 31;
  AVF_REQUIRE(d < lim, "%s: d is too large", who);                          // with T < 2^31: d * T < 2^62
  AVF_REQUIRE(F <= (INT64_MAX / 16) / (H * W), "%s: F * H * W is too large", who);
  *out = ClipBankSource{bank, video_db_nr, present, index, F, d, F * H * W * C};
  return 0;
}

// dst [n bytes] must not touch the bank
int apart(const char* who, const uint8_t* bank, int64_t bank_bytes, const void* dst, int64_t n) {
  const uintptr_t b0 = (uintptr_t)bank, d0 = (uintptr_t)dst;
  AVF_REQUIRE(d0 + (uintptr_t)n <= b0 || b0 + (uintptr_t)bank_bytes <= d0, "%s: dst overlaps the bank", who);
  return 0;
}

}  // namespace
}  // namespace avf

extern "C" int avf_clip_gather(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present, const int64_t* index,
                               int64_t F, int64_t B, int64_t T, int64_t d, int64_t H, int64_t W, int C, uint8_t* dst, void* stream) {
  using namespace avf;
  const char* who = "clip_gather";
  AVF_REQUIRE(dst, "%s: dst is null", who);
  AVF_TRY(clip_shape_ok(who, B, T, H, W, C));
  ClipBankSource from;
  AVF_TRY(bank_source(who, bank, video_db_nr, present, index, F, T, d, H, W, C, &from));
  const int64_t frame_bytes = H * W * C;
  AVF_TRY(apart(who, bank, from.total_bytes, dst, B * T * frame_bytes));
  const int64_t tiles = ceil_div(frame_bytes, GATHER_TILE);
  const int64_t tile_bytes = ceil_div(ceil_div(frame_bytes, tiles), 16) * 16;   // <= GATHER_TILE, no tile is empty
  const int64_t blocks = B * T * tiles;
  AVF_REQUIRE(tiles < (1LL << 31) && blocks < (1LL << 31), "%s: B * T * H * W gives too many tiles", who);
  clip_gather_kernel<<<(unsigned)blocks, GATHER_THREADS, 0, (hipStream_t)stream>>>(from, dst, T, frame_bytes, (int)tile_bytes,
                                                                                    (int)tiles);
  return check_launch("clip_gather_kernel");
}

extern "C" int avf_clip_gather_normalize(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present,
                                         const int64_t* index, int64_t F, int64_t B, int64_t T, int64_t d, int64_t H, int64_t W, int C,
                                         int k, const float* lut, const uint8_t* flip, void* dst, int out_dtype, int layout,
                                         void* stream) {
  using namespace avf;
  const char* who = "clip_gather_normalize";
  AVF_REQUIRE(lut, "%s: lut is null", who);
  AVF_REQUIRE(dst, "%s: dst is null", who);
  AVF_TRY(clip_shape_ok(who, B, T, H, W, C));
  ClipBankSource from;
  AVF_TRY(bank_source(who, bank, video_db_nr, present, index, F, T, d, H, W, C, &from));
  return clip_normalize_launch(who, from, B, T, H, W, C, k, lut, flip, dst, out_dtype, layout, (hipStream_t)stream);
}

extern "C" int avf_clip_gather_autoaugment(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present,
                                           const int64_t* index, int64_t F, int64_t B, int64_t T, int64_t d, int64_t H, int64_t W,
                                           int C, const int32_t* plan, uint8_t* dst, void* stream) {
  using namespace avf;
  const char* who = "clip_gather_autoaugment";
  AVF_REQUIRE(dst, "%s: dst is null", who);
  AVF_REQUIRE(plan, "%s: plan is null", who);
  AVF_REQUIRE(((uintptr_t)plan & 3u) == 0, "%s: plan is not aligned to its element", who);
  AVF_TRY(aug_shape_ok(who, B, T, H, W, C));
  ClipBankSource from;
  AVF_TRY(bank_source(who, bank, video_db_nr, present, index, F, T, d, H, W, C, &from));
  AVF_TRY(apart(who, bank, from.total_bytes, dst, B * T * H * W * C));
  return aug_bytes_launch(who, from, dst, B, T, H, W, C, plan, (hipStream_t)stream);
}

extern "C" int avf_clip_gather_autoaugment_normalize(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present,
                                                     const int64_t* index, int64_t F, int64_t B, int64_t T, int64_t d, int64_t H,
                                                     int64_t W, int C, const int32_t* plan, int k, const float* lut,
                                                     const uint8_t* flip, void* dst, int out_dtype, int layout, void* stream) {
  using namespace avf;
  const char* who = "clip_gather_autoaugment_normalize";
  AVF_REQUIRE(plan, "%s: plan is null", who);
  AVF_REQUIRE(((uintptr_t)plan & 3u) == 0, "%s: plan is not aligned to its element", who);
  AVF_REQUIRE(lut, "%s: lut is null", who);
  AVF_REQUIRE(dst, "%s: dst is null", who);
  AVF_TRY(aug_shape_ok(who, B, T, H, W, C));
  AVF_TRY(aug_planes_ok(who, C, k, lut, dst, out_dtype, layout));
  ClipBankSource from;
  AVF_TRY(bank_source(who, bank, video_db_nr, present, index, F, T, d, H, W, C, &from));
  AVF_TRY(apart(who, bank, from.total_bytes, dst, aug_planes_bytes(B, T, H, W, k, out_dtype)));
  return aug_planes_launch(who, from, B, T, H, W, C, plan, k, lut, flip, dst, out_dtype, layout, (hipStream_t)stream);
}
