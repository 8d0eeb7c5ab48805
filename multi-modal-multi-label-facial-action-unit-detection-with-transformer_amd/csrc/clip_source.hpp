// clip_source.hpp - where the kernels of clip.hip, augment.hip and clip_bank.hip find the frame in slot t of clip b, and how
// they stage a byte range of it in LDS.  The kernels are templates over the source:
//
//   ClipTensorSource   an assembled clip [B, T, H, W, C]: frame b * T + t of it
//   ClipBankSource     a resident frame bank [F, H, W, C] and index[B]: the data loader's rule
//                      (dataloader/aff2compdataset.py:122-156; testset.py:84-113 repeats the loop).  Slot t of sample `index` is
//                      frame a = index - d * (T - 1 - t) - range(index - T * d + d, index - T * d + d * (T + 1), d), the last slot
//                      is `index` itself - and it is BLACK (all bytes 0) where a < 0 or a >= F (129), where
//                      video_db_nr[a] != video_db_nr[index] (129), or where the frame is marked absent (the try / except: pass
//                      of 142-155 around a failed decode).  An index outside [0, F) gives an all-black clip and reads nothing of
//                      the bank (the reference would raise; nothing on the device can).
//
// frame() returns the frame's first byte, or nullptr for a black slot.  Every load in it has an address that depends on the
// workgroup's frame alone: it is uniform over the workgroup.  base() .. base() + bytes() is what may be read.
#pragma once
#include "common.hpp"

namespace avf {
namespace {

struct ClipTensorSource {
  const uint8_t* src;
  int64_t total_bytes;
  __device__ __forceinline__ const uint8_t* frame(int64_t b, int64_t t, int64_t T, int64_t frame_bytes) const {
    return src + (b * T + t) * frame_bytes;
  }
  __device__ __forceinline__ const uint8_t* base() const { return src; }
  __device__ __forceinline__ int64_t bytes() const { return total_bytes; }
};

struct ClipBankSource {
  const uint8_t* bank;          // [F, H, W, C]
  const int32_t* video_db_nr;   // [F]
  const uint8_t* present;       // [F] or null: every frame is present
  const int64_t* index;         // [B]
  int64_t F, d;                 // d >= 1; d * T < 2^62 (the host checks)
  int64_t total_bytes;          // F * frame_bytes
  __device__ __forceinline__ const uint8_t* frame(int64_t b, int64_t t, int64_t T, int64_t frame_bytes) const {
    const int64_t i = index[b];
    if (i < 0 || i >= F) return nullptr;
    const int64_t a = i - d * (T - 1 - t);
    if (a < 0 || a >= F) return nullptr;
    if (video_db_nr[a] != video_db_nr[i]) return nullptr;
    if (present != nullptr && present[a] == 0) return nullptr;
    return bank + a * frame_bytes;
  }
  __device__ __forceinline__ const uint8_t* base() const { return bank; }
  __device__ __forceinline__ int64_t bytes() const { return total_bytes; }
};

// Stages the 16-byte chunks around the byte range [first, first + nbytes) in LDS with aligned 16-byte loads: `chunks` chunks from
// first - (first & 15) on, so byte j of the range lands at stage[(first & 15) + j].  stage is 16-byte aligned.  Only the first and
// the last chunk of the WHOLE readable range [lo, hi) can reach outside it; those two are read byte by byte with a bounds check.
template <int THREADS>
__device__ __forceinline__ void stage_chunks(uint8_t* stage, const uint8_t* first, int chunks, const uint8_t* base, int64_t bytes,
                                             int tid) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(first) & ~(uintptr_t)15u;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base), hi = lo + (uintptr_t)bytes;
  for (int i = tid; i < chunks; i += THREADS) {
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
}

// a black slot: the same chunks, zero, and nothing is read
template <int THREADS>
__device__ __forceinline__ void zero_chunks(uint8_t* stage, int chunks, int tid) {
  for (int i = tid; i < chunks; i += THREADS) *reinterpret_cast<uint4*>(stage + 16 * i) = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace
}  // namespace avf
