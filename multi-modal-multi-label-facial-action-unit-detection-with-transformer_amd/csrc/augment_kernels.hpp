// augment_kernels.hpp - the device code that augment.hip (an assembled clip) and clip_bank.hip (a resident frame bank) share:
// the AutoAugment kernel as a template over the frame source (clip_source.hpp) and over the sink, where the finished frame goes
// (AugBytesSink / AugPlanesSink below).  augment.hip describes the kernel.  A file that includes this one is compiled with
// -ffp-contract=off.
#pragma once
#include "clip_kernels.hpp"

namespace avf {
namespace {

constexpr int AUG_THREADS = 512;
constexpr int AUG_WAVES = AUG_THREADS / 64;
constexpr int AUG_SLOT_WORDS = 8;
constexpr int AUG_FILL = 128;                                   // fillcolor=(128, 128, 128), autoaugment.py:18
constexpr int AUG_LDS = 160 * 1024;                             // what one workgroup may take of a CU's LDS
constexpr int AUG_HIST_BYTES = 3 * 256 * 4, AUG_LUT_BYTES = 3 * 256, AUG_RED_BYTES = 64;
constexpr int AUG_FIXED = AUG_HIST_BYTES + AUG_LUT_BYTES + AUG_RED_BYTES;
// a frame buffer: the n bytes of the frame behind a shift of < 16, in whole 16-byte chunks
constexpr int aug_frame_buffer(int n) { return ((n + 30) >> 4) << 4; }
constexpr int AUG_MAX_FRAME_BYTES = ((AUG_LDS - AUG_FIXED) / 2 / 16) * 16 + 15 - 30;
static_assert(2 * aug_frame_buffer(AUG_MAX_FRAME_BYTES) + AUG_FIXED <= AUG_LDS, "two largest frames do not fit");
static_assert(2 * aug_frame_buffer(AUG_MAX_FRAME_BYTES + 1) + AUG_FIXED > AUG_LDS, "the frame limit is not tight");
constexpr int64_t AUG_MAX_PIXELS = AUG_MAX_FRAME_BYTES / 3;     // C = 3; C = 4: AUG_MAX_FRAME_BYTES / 4

enum AugOp { OP_NONE = 0, OP_POSTERIZE, OP_SOLARIZE, OP_INVERT, OP_AUTOCONTRAST, OP_EQUALIZE, OP_COLOR, OP_CONTRAST, OP_SHARPNESS,
             OP_ROTATE, OP_SHEARX };

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ int wave_min(int v) { return -wave_max(-v); }

// Image.blend(deg, img, alpha) on one byte.  mode 0: alpha == 0, deg; 1: alpha == 1, img; 2: 0 < alpha < 1, no clipping
// (ImagingBlend's first loop); 3: clipping (its second loop)
struct Blend {
  float alpha;
  int mode;
};
__device__ __forceinline__ Blend blend_of(int32_t alpha_bits) {
  Blend b;
  b.alpha = __int_as_float(alpha_bits);
  b.mode = b.alpha == 0.0f ? 0 : b.alpha == 1.0f ? 1 : (b.alpha >= 0.0f && b.alpha <= 1.0f) ? 2 : 3;
  return b;
}
__device__ __forceinline__ int blend_one(int deg, int img, Blend b) {
#pragma clang fp contract(off)
  if (b.mode == 0) return deg;
  if (b.mode == 1) return img;
  const float prod = b.alpha * (float)(img - deg);
  const float t = (float)deg + prod;
  if (b.mode == 2) return (int)t & 255;
  return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;   // (a NaN alpha cannot come from the host's encoder; it gives 0 here)
}

__device__ __forceinline__ int grey_of(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// ImageOps.autocontrast's table entry: int(i * scale + offset), clamped
__device__ __forceinline__ int autocontrast_entry(int i, int lo, int hi) {
#pragma clang fp contract(off)
  const double scale = 255.0 / (double)(hi - lo);
  const double off = -(double)lo * scale;
  const double prod = (double)i * scale;
  const double t = prod + off;
  const int r = (int)t;
  return r < 0 ? 0 : r > 255 ? 255 : r;
}

// ImageEnhance.Contrast's degenerate grey: int(mean + 0.5) of the L image
__device__ __forceinline__ int contrast_mean(int sum, int count) {
#pragma clang fp contract(off)
  const double mean = (double)sum / (double)count;
  return (int)(mean + 0.5);
}

// one output pixel of Image.transform(AFFINE (1, m, 0, 0, 1, 0), BICUBIC, fillcolor 128): Geometry.c affine_transform +
// bicubic_filter32RGB; the vertical pass has dy == 0 exactly and returns the row's own value
template <int C>
__device__ __forceinline__ void shear_pixel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int x, int y, int W, double m) {
#pragma clang fp contract(off)
  const uint8_t* row = in + (size_t)y * W * C;
  uint8_t* o = out + ((size_t)y * W + x) * C;
  if (C == 4) o[3] = row[x * C + 3];
  const double my = m * ((double)y + 0.5);
  double xin = ((double)x + 0.5) + my;
  if (!(xin >= 0.0 && xin < (double)W)) {
    o[0] = o[1] = o[2] = AUG_FILL;
    return;
  }
  xin = xin - 0.5;
  const double xf = floor(xin);
  const double d = xin - xf;
  const int xi = (int)xf;
  int col[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = xi - 1 + k;
    col[k] = c < 0 ? 0 : c > W - 1 ? W - 1 : c;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v1 = row[col[0] * C + c], v2 = row[col[1] * C + c], v3 = row[col[2] * C + c], v4 = row[col[3] * C + c];
    const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    double t = d * p4;
    t = p3 + t;
    t = d * t;
    t = p2 + t;
    t = d * t;
    t = p1 + t;
    o[c] = t <= 0.0 ? 0 : t >= 255.0 ? 255 : (uint8_t)(int)t;
  }
}


// Where the finished frame goes.  A sink is passed by value and tells the kernel three things: is(p) - whether it writes to p
// (a frame without operations is then already in place); shift() - where the frame's first byte sits inside its 16-byte chunk of
// LDS; store() - the last phase, from the LDS frame `res` (pixel byte j at res[shift + j]) to global memory.  `idle` is the
// frame buffer that does not hold the result: fb bytes, 16-byte aligned, free for the store phase.
//
//   AugBytesSink        the interleaved uint8 frame to dst + frame * n.  The frame is staged with the DESTINATION's offset, so
//                       the 16-byte stores are aligned; the first and last chunk, shared with the neighbouring frames, go out
//                       byte by byte.
//   AugPlanesSink<OutT> the store phase of clip_normalize_kernel (clip_kernels.hpp) on the LDS frame: the last k channels as
//                       planes of OutT = float | bf16, value lut[channel][byte], a flagged clip read backwards within each row.
//                       There is no byte destination, so the frame is staged with the SOURCE's offset (0 for a black slot) and
//                       staging always takes the aligned 16-byte path.  The k * 256 table entries are copied into the idle
//                       frame buffer - no LDS beyond what the bytes sink asks for -; a frame whose buffer is too small for them
//                       (fb < k * 1024) reads the table from global memory instead.
struct AugBytesSink {
  uint8_t* dst;
  static constexpr bool STAGES_AT_SOURCE_OFFSET = false;
  __device__ __forceinline__ bool is(const uint8_t* p) const { return dst == p; }
  __device__ __forceinline__ int shift(int64_t frame, int n, const uint8_t*) const {
    return (int)(reinterpret_cast<uintptr_t>(dst + frame * n) & 15u);
  }
  template <int C>
  __device__ __forceinline__ void store(const uint8_t* res, uint8_t*, int, int shift, int64_t frame, int64_t, int H, int W,
                                        int tid) const {
    const int n = H * W * C;
    const int chunks = (shift + n + 15) >> 4;
    uint8_t* a0 = dst + frame * n - shift;
    for (int i = tid; i < chunks; i += AUG_THREADS) {
      const int off = 16 * i - shift;   // of the chunk's first byte inside the frame's byte range
      if (off >= 0 && off + 16 <= n) {
        *reinterpret_cast<uint4*>(a0 + 16 * i) = *reinterpret_cast<const uint4*>(res + 16 * i);
      } else {  // the frame's first / last chunk is shared with its neighbours: only the bytes that are this frame's
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (off + q >= 0 && off + q < n) a0[16 * i + q] = res[16 * i + q];
      }
    }
  }
};

// the k planes of one frame: every lane 16 bytes of ONE plane, consecutive lanes consecutive addresses, up to VEC - 1 scalar
// stores in front of the first aligned vector and behind the last (a plane starts wherever it starts).  px: the frame's first
// byte; table: the k * 256 entries of the kept channels, in LDS or in global memory
template <int C, typename OutT>
__device__ __forceinline__ void store_planes(const float* __restrict__ table, const uint8_t* __restrict__ px, OutT* __restrict__ dst,
                                             int k, int layout, bool mirrored, int64_t b, int64_t t, int64_t T, int P, int W,
                                             int tid) {
  constexpr int VEC = 16 / (int)sizeof(OutT);
  for (int ci = 0; ci < k; ++ci) {
    const int64_t plane = layout == AVF_CLIP_CTHW ? (b * k + ci) * T + t : (b * T + t) * k + ci;
    OutT* __restrict__ o = dst + plane * (int64_t)P;
    const float* lt = table + ci * 256;
    const uint8_t* sg = px + (C - k + ci);
    // source pixel of output pixel j: the same, or the same row read backwards
    auto one = [&](int j) -> float {
      int sl = j;
      if (mirrored) {
        const int r = j / W;
        sl = r * W + (W - 1 - (j - r * W));
      }
      return lt[sg[sl * C]];
    };
    const int head = head_elems(o, P);
    const int nvec = (P - head) / VEC, tail = (P - head) - nvec * VEC;
    if (tid < head) o[tid] = from_f32<OutT>(one(tid));
    if (tid < tail) o[head + nvec * VEC + tid] = from_f32<OutT>(one(head + nvec * VEC + tid));
    if (!mirrored) {
      for (int v = tid; v < nvec; v += AUG_THREADS) {
        const int j0 = head + v * VEC;
        float x[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) x[i] = lt[sg[(j0 + i) * C]];
        store_vec<OutT>(o + j0, x);
      }
    } else {
      for (int v = tid; v < nvec; v += AUG_THREADS) {
        const int j0 = head + v * VEC;
        const int r = j0 / W;
        int wl = j0 - r * W, row = r * W;   // a vector may run over the end of a row
        float x[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          x[i] = lt[sg[(row + W - 1 - wl) * C]];
          if (++wl == W) {
            wl = 0;
            row += W;
          }
        }
        store_vec<OutT>(o + j0, x);
      }
    }
  }
}

template <typename OutT>
struct AugPlanesSink {
  OutT* dst;             // [B, k, T, H, W] (cthw) or [B, T, k, H, W] (tchw)
  const float* lut;      // [C, 256]
  const uint8_t* flip;   // [B] or null: no clip is mirrored
  int k, layout;
  static constexpr bool STAGES_AT_SOURCE_OFFSET = true;
  __device__ __forceinline__ bool is(const uint8_t*) const { return false; }
  __device__ __forceinline__ int shift(int64_t, int, const uint8_t* first) const {
    return first != nullptr ? (int)(reinterpret_cast<uintptr_t>(first) & 15u) : 0;
  }
  template <int C>
  __device__ __forceinline__ void store(const uint8_t* res, uint8_t* idle, int fb, int shift, int64_t frame, int64_t T, int H, int W,
                                        int tid) const {
    const int64_t b = frame / T, t = frame - b * T;
    const bool mirrored = flip != nullptr && flip[b] != 0;               // uniform over the workgroup
    const float* table = lut + (C - k) * 256;
    if (fb >= k * 256 * (int)sizeof(float)) {                            // (uniform)
      float* table_s = reinterpret_cast<float*>(idle);
      for (int i = tid; i < k * 256; i += AUG_THREADS) table_s[i] = table[i];
      __syncthreads();
      store_planes<C, OutT>(table_s, res + shift, dst, k, layout, mirrored, b, t, T, H * W, W, tid);
    } else {  // a frame of a few pixels: correct, not fast
      store_planes<C, OutT>(table, res + shift, dst, k, layout, mirrored, b, t, T, H * W, W, tid);
    }
  }
};

template <int C, typename Source, typename Sink>
__global__ __launch_bounds__(AUG_THREADS) void clip_autoaugment_kernel(const Source src, const Sink sink, int64_t T,
                                                                      const int32_t* __restrict__ plan, int H, int W, int fb) {
  extern __shared__ __attribute__((aligned(16))) uint8_t aug_lds[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(aug_lds + 2 * fb);                    // [3][256]
  uint8_t* lut = aug_lds + 2 * fb + AUG_HIST_BYTES;                                  // [3][256]
  int* red = reinterpret_cast<int*>(aug_lds + 2 * fb + AUG_HIST_BYTES + AUG_LUT_BYTES);   // [AUG_WAVES]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t frame = blockIdx.x;
  const int P = H * W, n = P * C;
  const int32_t* pl = plan + frame * (2 * AUG_SLOT_WORDS);
  int ops[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int op = pl[s * AUG_SLOT_WORDS];
    ops[s] = (op >= OP_POSTERIZE && op <= OP_SHEARX) ? op : OP_NONE;
  }
  if (ops[0] == OP_NONE && ops[1] == OP_NONE && sink.is(src.base())) return;

  const uint8_t* first = src.frame(frame / T, frame % T, T, n);   // null: a black slot
  const int shift = sink.shift(frame, n, first);
  const int chunks = (shift + n + 15) >> 4;                                          // 16 * chunks <= fb
  int cur = 0;                                                                       // which frame buffer holds the frame
  {
    uint8_t* stage = aug_lds;
    if (first == nullptr) {
      zero_chunks<AUG_THREADS>(stage, chunks, tid);
    } else if (Sink::STAGES_AT_SOURCE_OFFSET || (int)(reinterpret_cast<uintptr_t>(first) & 15u) == shift) {
      stage_chunks<AUG_THREADS>(stage, first, chunks, src.base(), src.bytes(), tid);
    } else {
      for (int k = tid; k < n; k += AUG_THREADS) stage[shift + k] = first[k];
    }
  }
  __syncthreads();

  for (int s = 0; s < 2; ++s) {
    const int op = ops[s];
    if (op == OP_NONE) continue;                                                     // (uniform over the workgroup, as all below)
    const int32_t* q = pl + s * AUG_SLOT_WORDS + 1;
    uint8_t* buf = aug_lds + cur * fb;                                               // chunk-aligned; pixel byte k at buf[shift + k]
    uint8_t* px = buf + shift;
    uint8_t* other = aug_lds + (cur ^ 1) * fb + shift;
    bool table = false;

    if (op == OP_POSTERIZE || op == OP_SOLARIZE || op == OP_INVERT) {
      const int p0 = q[0];
      if (tid < 256) {
        const int v = tid;
        const int r = op == OP_POSTERIZE ? (v & p0) : op == OP_INVERT ? 255 - v : (v < p0 ? v : 255 - v);
        lut[v] = lut[256 + v] = lut[512 + v] = (uint8_t)r;
      }
      table = true;
    } else if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
      for (int i = tid; i < 3 * 256; i += AUG_THREADS) hist[i] = 0u;
      __syncthreads();
      for (int p0 = tid - lane; p0 < P; p0 += AUG_THREADS) {                         // the trip count is the wave's
        const int p = p0 + lane;
        const bool valid = p < P;
        const unsigned long long act = __ballot(valid);
        const int lead = __ffsll((long long)act) - 1;                                // lane 0: p0 < P
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int v = valid ? (int)px[p * C + c] : -1;
          const int v0 = __shfl(v, lead);
          if (__ballot(valid && v == v0) == act) {                                   // a flat stretch: one add for the wave
            if (lane == lead) atomicAdd(&hist[c * 256 + v0], (uint32_t)__popcll(act));
          } else if (valid) {
            atomicAdd(&hist[c * 256 + v], 1u);
          }
        }
      }
      __syncthreads();
      if (wave < 3) {                                                                // wave c: the table of channel c
        const uint32_t* h = hist + wave * 256 + 4 * lane;
        const int h4[4] = {(int)h[0], (int)h[1], (int)h[2], (int)h[3]};
        int nz = 0, last = -1, lo = 256, sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (h4[j] != 0) {
            ++nz;
            last = 4 * lane + j;
            if (lo == 256) lo = 4 * lane + j;
          }
          sum += h4[j];
        }
        last = wave_max(last);                                                       // >= 0: the frame has pixels
        lo = wave_min(lo);
        uint8_t* lt = lut + wave * 256 + 4 * lane;
        if (op == OP_AUTOCONTRAST) {
#pragma unroll
          for (int j = 0; j < 4; ++j) lt[j] = (uint8_t)(last <= lo ? 4 * lane + j : autocontrast_entry(4 * lane + j, lo, last));
        } else {
          nz = wave_sum(nz);
          int before = sum;                                                          // pixels in the bins below this lane's
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(before, o);
            if (lane >= o) before += t;
          }
          before -= sum;
          const uint32_t step = (uint32_t)(P - (int)hist[wave * 256 + last]) / 255u;
          uint32_t acc = step / 2u + (uint32_t)before;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int r = 4 * lane + j;
            if (nz > 1 && step != 0u) {
              const uint32_t e = acc / step;
              r = e > 255u ? 255 : (int)e;
            }
            lt[j] = (uint8_t)r;
            acc += (uint32_t)h4[j];
          }
        }
      }
      table = true;
    } else if (op == OP_CONTRAST) {
      const Blend b = blend_of(q[0]);
      int part = 0;
      for (int p = tid; p < P; p += AUG_THREADS) part += grey_of(px[p * C], px[p * C + 1], px[p * C + 2]);   // <= 255 * P: fits
      part = wave_sum(part);
      if (lane == 0) red[wave] = part;
      __syncthreads();
      int sum = 0;
#pragma unroll
      for (int w = 0; w < AUG_WAVES; ++w) sum += red[w];
      const int mean = contrast_mean(sum, P);
      if (tid < 256) lut[tid] = lut[256 + tid] = lut[512 + tid] = (uint8_t)blend_one(mean, tid, b);
      table = true;
    } else if (op == OP_COLOR) {
      const Blend b = blend_of(q[0]);
      if (b.mode != 1) {
        for (int p = tid; p < P; p += AUG_THREADS) {
          uint8_t* o = px + p * C;
          const int r = o[0], g = o[1], bl = o[2];
          const int L = grey_of(r, g, bl);
          o[0] = (uint8_t)blend_one(L, r, b);
          o[1] = (uint8_t)blend_one(L, g, b);
          o[2] = (uint8_t)blend_one(L, bl, b);
        }
      }
    } else if (op == OP_SHARPNESS) {
      const Blend b = blend_of(q[0]);
      if (b.mode != 1) {
        for (int p = tid; p < P; p += AUG_THREADS) {
          const int y = p / W, x = p - y * W;
          const bool interior = y > 0 && y < H - 1 && x > 0 && x < W - 1;            // never where H < 3 or W < 3
          const uint8_t* i0 = px + p * C;
          uint8_t* o = other + p * C;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int v = i0[c];
            int deg = v;
            if (interior) {                                                          // ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13
              int S = 4 * v;
#pragma unroll
              for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) S += i0[(dy * W + dx) * C + c];
              deg = (2 * S + 13) / 26;
            }
            o[c] = (uint8_t)blend_one(deg, v, b);
          }
          if (C == 4) o[3] = i0[3];
        }
        cur ^= 1;
      }
    } else if (op == OP_ROTATE) {
      // Geometry.c affine_fixed: C ints stepped per pixel - 32-bit wrap-around, arithmetic shift
      const uint32_t a0 = (uint32_t)q[0], a1 = (uint32_t)q[1], a2 = (uint32_t)q[2], a3 = (uint32_t)q[3], a4 = (uint32_t)q[4],
                     a5 = (uint32_t)q[5];
      for (int p = tid; p < P; p += AUG_THREADS) {
        const int y = p / W, x = p - y * W;
        const int xs = (int32_t)(a2 + a1 * (uint32_t)y + a0 * (uint32_t)x) >> 16;
        const int ys = (int32_t)(a5 + a4 * (uint32_t)y + a3 * (uint32_t)x) >> 16;
        uint8_t* o = other + p * C;
        if (xs >= 0 && xs < W && ys >= 0 && ys < H) {
          const uint8_t* i0 = px + (ys * W + xs) * C;
          o[0] = i0[0];
          o[1] = i0[1];
          o[2] = i0[2];
        } else {
          o[0] = o[1] = o[2] = AUG_FILL;
        }
        if (C == 4) o[3] = px[p * C + 3];
      }
      cur ^= 1;
    } else {  // OP_SHEARX
      const double m = __hiloint2double(q[1], q[0]);
      for (int p = tid; p < P; p += AUG_THREADS) {
        const int y = p / W, x = p - y * W;
        shear_pixel<C>(px, other, x, y, W, m);
      }
      cur ^= 1;
    }

    if (table) {
      __syncthreads();
      // four bytes at a time; byte i of the buffer is channel (i - shift) mod C (bytes outside the frame: looked up, never written out)
      uint32_t* words = reinterpret_cast<uint32_t*>(buf);
      const int nwords = (shift + n + 3) >> 2;
      for (int d = tid; d < nwords; d += AUG_THREADS) {
        const uint32_t w = words[d];
        uint32_t r = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = (4 * d + j - shift + 48) % C;                                // 48: a multiple of 3 and 4 above the shift
          const uint32_t v = (w >> (8 * j)) & 255u;
          r |= (c < 3 ? (uint32_t)lut[c * 256 + v] : v) << (8 * j);
        }
        words[d] = r;
      }
    }
    __syncthreads();
  }

  sink.template store<C>(aug_lds + cur * fb, aug_lds + (cur ^ 1) * fb, fb, shift, frame, T, H, W, tid);
}

// what both entry points ask of the clip's shape
int aug_shape_ok(const char* who, int64_t B, int64_t T, int64_t H, int64_t W, int C) {
  AVF_REQUIRE(B >= 1, "%s: B is %lld, below 1", who, (long long)B);
  AVF_REQUIRE(T >= 1, "%s: T is %lld, below 1", who, (long long)T);
  AVF_REQUIRE(H >= 1, "%s: H is %lld, below 1", who, (long long)H);
  AVF_REQUIRE(W >= 1, "%s: W is %lld, below 1", who, (long long)W);
  AVF_REQUIRE(C == 3 || C == 4, "%s: C is %d, neither 3 (RGB) nor 4 (RGB + mask)", who, C);
  const int64_t max_pixels = AUG_MAX_FRAME_BYTES / C;
  AVF_REQUIRE(H <= max_pixels && W <= max_pixels && H * W <= max_pixels,
              "%s: a frame of %lld x %lld pixels is above the limit of %lld pixels for C = %d (a workgroup keeps two "
              "copies of its frame in LDS)", who, (long long)H, (long long)W, (long long)max_pixels, C);
  const int64_t lim = 1LL << 31;
  AVF_REQUIRE(B < lim && T < lim && B * T < lim, "%s: B * T is too large", who);
  return 0;
}

template <int C, typename Source, typename Sink>
int aug_launch(const char* who, const Source& src, const Sink& sink, int64_t B, int64_t T, int H, int W, const int32_t* plan,
               hipStream_t s) {
  static PerDeviceOnce once;
  if (once.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)clip_autoaugment_kernel<C, Source, Sink>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, AUG_LDS);
    AVF_REQUIRE(e == hipSuccess, "%s: cannot raise dynamic LDS limit: %s", who, hipGetErrorString(e));
    once.mark();
  }
  const int n = H * W * C, fb = aug_frame_buffer(n);
  const int lds = 2 * fb + AUG_FIXED;
  AVF_REQUIRE(lds <= AUG_LDS, "%s: %d bytes of LDS", who, lds);
  clip_autoaugment_kernel<C, Source, Sink><<<(unsigned)(B * T), AUG_THREADS, (uint32_t)lds, s>>>(src, sink, T, plan, H, W, fb);
  return check_launch("clip_autoaugment_kernel");
}

// the bytes sink, for either source
template <typename Source>
int aug_bytes_launch(const char* who, const Source& src, uint8_t* dst, int64_t B, int64_t T, int64_t H, int64_t W, int C,
                     const int32_t* plan, hipStream_t s) {
  const AugBytesSink to{dst};
  return C == 3 ? aug_launch<3>(who, src, to, B, T, (int)H, (int)W, plan, s) : aug_launch<4>(who, src, to, B, T, (int)H, (int)W, plan, s);
}

// what the planes sink asks of its output side: the checks of clip_normalize_launch, and the table's alignment
int aug_planes_ok(const char* who, int C, int k, const float* lut, const void* dst, int out_dtype, int layout) {
  AVF_TRY(clip_output_ok(who, C, k, dst, out_dtype, layout));
  AVF_REQUIRE(((uintptr_t)lut & 3u) == 0, "%s: lut is not aligned to its element", who);
  return 0;
}

// the planes sink, for either source.  The caller has checked its pointers, the shape (aug_shape_ok), the output side
// (aug_planes_ok) and that dst is apart from what the source reads.
template <typename Source>
int aug_planes_launch(const char* who, const Source& src, int64_t B, int64_t T, int64_t H, int64_t W, int C, const int32_t* plan,
                      int k, const float* lut, const uint8_t* flip, void* dst, int out_dtype, int layout, hipStream_t s) {
  if (out_dtype == AVF_F32) {
    const AugPlanesSink<float> to{(float*)dst, lut, flip, k, layout};
    return C == 3 ? aug_launch<3>(who, src, to, B, T, (int)H, (int)W, plan, s) : aug_launch<4>(who, src, to, B, T, (int)H, (int)W, plan, s);
  }
  const AugPlanesSink<bf16> to{(bf16*)dst, lut, flip, k, layout};
  return C == 3 ? aug_launch<3>(who, src, to, B, T, (int)H, (int)W, plan, s) : aug_launch<4>(who, src, to, B, T, (int)H, (int)W, plan, s);
}

// bytes of the planes of B clips (after aug_planes_ok)
int64_t aug_planes_bytes(int64_t B, int64_t T, int64_t H, int64_t W, int k, int out_dtype) {
  return B * k * T * H * W * (out_dtype == AVF_F32 ? 4 : 2);
}

}  // namespace
}  // namespace avf
