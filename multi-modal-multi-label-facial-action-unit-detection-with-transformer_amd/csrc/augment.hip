// augment.hip - clip AutoAugment on the device: the reference's ImageNetPolicy (dataloader/autoaugment.py:19-49, 104-112;
// dataloader/ops.py) on uint8 clips [B, T, H, W, C], byte for byte what Pillow computes.
//
// avf_clip_autoaugment, one launch, ONE WORKGROUP PER FRAME.  The host has resolved the random draws and every constant that
// needs Python's double arithmetic into the frame's plan: two slots [op_code, p0 .. p6] (augment.py documents the encoding).
// The workgroup
//   1. stages the frame's H * W * C bytes in LDS with aligned 16-byte loads.  The byte range starts wherever it starts: it
//      keeps the offset (`shift`) that the DESTINATION range has inside its first 16-byte chunk, so that the stores of step 3
//      are aligned; where the source range sits differently in its chunks (a view with an odd offset written to a fresh
//      tensor), the frame is staged byte by byte instead;
//   2. runs slot 1 and then slot 2 on the LDS copy, channels 0..2 only:
//        posterize, solarize, invert            a 256-entry table, applied four bytes at a time
//        autocontrast, equalize                 per-channel histograms (LDS atomics; a wave whose lanes all hold one value adds
//                                               its count once), one wave per channel builds the table - equalize with a wave
//                                               scan -, applied as above
//        contrast                               the grey mean reduced over the workgroup, then the table blend(mean, v)
//        color                                  per pixel, in place: blend(grey, v)
//        sharpness, rotate, shearX              read neighbours / other positions: written into the second frame buffer,
//                                               which then becomes the current one
//   3. writes the frame with aligned 16-byte stores (the first and last chunk, shared with the neighbouring frames, byte by
//      byte).  dst == src is allowed: a workgroup reads all it uses of its frame before it writes.
// A frame whose two op codes are 0 (or outside 1..10) is copied; with dst == src its workgroup returns at once.
//
// avf_clip_autoaugment_normalize, one launch: the same kernel with another step 3 (the kernel is a template over its sink,
// augment_kernels.hpp) - ImageNetPolicy, RandomClipFlip, NumpyToTensor and Normalize, the reference's aug_clip_transform
// (dataloader/aff2compdataset.py:72-74, 163-164), without a uint8 clip in between.  Step 1 keeps the SOURCE's offset (there is
// no byte destination), so it always loads aligned 16-byte chunks.  Step 3 is the store phase of clip.hip's normalise kernel on
// the LDS frame: per kept channel each lane stores 16 bytes (4 fp32 / 8 bf16 pixels) of one plane, value lut[channel][byte],
// scalar stores in front of the first aligned vector and behind the last; a mirrored clip (flip[b], read on the device)
// reverses the read index within each row.  The k * 256 table entries sit in the frame buffer that does not hold the result,
// so the launch asks for no more LDS than avf_clip_autoaugment does (79200 B at 112 x 112 x 3, two workgroups per CU); a
// frame of fewer than k * 1024 bytes reads the table from global memory.
//
// Arithmetic: integers wherever Pillow's are integers; fp32 for Image.blend, fp64 for the autocontrast table and the bicubic
// of shearX, each operation rounded on its own (#pragma clang fp contract(off) in every function with floating-point
// arithmetic - see clip.hip - and -ffp-contract=off for the file); float / double -> byte conversions truncate.
// Every LDS read index of rotate and shearX is range-checked or clamped before the load, whatever the plan holds.
//
// The kernel is a template over where a frame comes from (clip_source.hpp) and lives in augment_kernels.hpp, which
// clip_bank.hip instantiates over a resident frame bank; here the source is the assembled clip.
//
// gfx950 resources (hipcc -O3, --save-temps): see DESIGN.md section 9.
#include "augment_kernels.hpp"

extern "C" int64_t avf_clip_autoaugment_max_pixels(void) { return avf::AUG_MAX_PIXELS; }

extern "C" int avf_clip_autoaugment(const uint8_t* src, uint8_t* dst, int64_t B, int64_t T, int64_t H, int64_t W, int C,
                                    const int32_t* plan, void* stream) {
  using namespace avf;
  AVF_REQUIRE(src, "clip_autoaugment: src is null");
  AVF_REQUIRE(dst, "clip_autoaugment: dst is null");
  AVF_REQUIRE(plan, "clip_autoaugment: plan is null");
  AVF_REQUIRE(((uintptr_t)plan & 3u) == 0, "clip_autoaugment: plan is not aligned to its element");
  AVF_TRY(aug_shape_ok("clip_autoaugment", B, T, H, W, C));
  const int64_t bytes = B * T * H * W * C;                          // < 2^31 * 2^17
  AVF_REQUIRE(dst == src || dst + bytes <= src || src + bytes <= dst, "clip_autoaugment: dst overlaps src without being src");
  const ClipTensorSource from{src, bytes};
  return aug_bytes_launch("clip_autoaugment", from, dst, B, T, H, W, C, plan, (hipStream_t)stream);
}

extern "C" int avf_clip_autoaugment_normalize(const uint8_t* src, int64_t B, int64_t T, int64_t H, int64_t W, int C,
                                              const int32_t* plan, int k, const float* lut, const uint8_t* flip, void* dst,
                                              int out_dtype, int layout, void* stream) {
  using namespace avf;
  const char* who = "clip_autoaugment_normalize";
  AVF_REQUIRE(src, "%s: src is null", who);
  AVF_REQUIRE(plan, "%s: plan is null", who);
  AVF_REQUIRE(((uintptr_t)plan & 3u) == 0, "%s: plan is not aligned to its element", who);
  AVF_REQUIRE(lut, "%s: lut is null", who);
  AVF_REQUIRE(dst, "%s: dst is null", who);
  AVF_TRY(aug_shape_ok(who, B, T, H, W, C));
  AVF_TRY(aug_planes_ok(who, C, k, lut, dst, out_dtype, layout));
  const int64_t bytes = B * T * H * W * C;
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  AVF_REQUIRE(d0 + (uintptr_t)aug_planes_bytes(B, T, H, W, k, out_dtype) <= s0 || s0 + (uintptr_t)bytes <= d0, "%s: dst overlaps src",
              who);
  const ClipTensorSource from{src, bytes};
  return aug_planes_launch(who, from, B, T, H, W, C, plan, k, lut, flip, dst, out_dtype, layout, (hipStream_t)stream);
}
