// mel_kernels.hpp - mel_power_kernel, the waveform -> mel power launch of mel.hip and mel_bank.hip, as a template over where a row's
// samples come from (mel.hip's header describes the kernel itself).  The source answers, uniformly over the workgroup,
//
//   src.row(r, hop) -> Row { samples, frames, load(i) }
//
// samples: the length of row r; frames = 1 + samples / hop of it carry a value and sit right-aligned in the out_frames columns of
// the output, the columns in front are zero; load(i), 0 <= i < samples, is sample i as fp32.  A row with frames == 0 is silent:
// every column is a zero column and load() is never called.
//
//   MelDenseSource   audio fp32 [rows, samples]: row r starts at r * samples; every row has the same length (mel.hip)
//   MelBankSource    a resident waveform bank and index[B]: the data loader's window rule (mel_bank.hip)
#pragma once
#include "common.hpp"

namespace avf {
namespace {

constexpr int MEL_NFFT = 1024;
constexpr int MEL_HALF = MEL_NFFT / 2;        // points of the complex FFT; also the reflect padding on either side
constexpr int MEL_BINS = MEL_HALF + 1;
constexpr int MEL_MAX_MELS = 128;
constexpr int MEL_THREADS = 256;
constexpr int MEL_WAVES = MEL_THREADS / 64;
constexpr int MEL_FPW = 4;                    // frames per wave
constexpr int MEL_TILE = MEL_WAVES * MEL_FPW; // frames per workgroup
constexpr int MEL_XS1 = 72;                   // exchange 1: [k0][8 b + c], 64 values per row + 8 (the half-wave reads 4 rows)
constexpr int MEL_XS2 = 68;                   // exchange 2: [c][8 k1 + k0]
constexpr int MEL_XCH = 8 * MEL_XS1;          // float2 per wave (>= 8 * MEL_XS2, >= MEL_HALF)
constexpr int MEL_PS = 516;                   // floats per power row
constexpr int MEL_TS = MEL_TILE + 1;          // floats per tile row

struct c32 {
  float r, i;
};
__device__ __forceinline__ c32 operator+(c32 a, c32 b) { return {a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ c32 operator-(c32 a, c32 b) { return {a.r - b.r, a.i - b.i}; }
__device__ __forceinline__ c32 cmul(c32 a, float2 w) { return {a.r * w.x - a.i * w.y, a.r * w.y + a.i * w.x}; }
__device__ __forceinline__ c32 mul_mi(c32 a) { return {a.i, -a.r}; }  // a * (-i)

// 4-point DFT of b[0..3] (forward sign) into out[0], out[2], out[4], out[6]
__device__ __forceinline__ void dft4(const c32* b, c32* out) {
  const c32 c0 = b[0] + b[2], c2 = b[0] - b[2], c1 = b[1] + b[3], c3 = mul_mi(b[1] - b[3]);
  out[0] = c0 + c1;
  out[4] = c0 - c1;
  out[2] = c2 + c3;
  out[6] = c2 - c3;
}

// v <- DFT8(v), natural order in and out: one radix-2 decimation-in-frequency step, then two 4-point transforms
__device__ __forceinline__ void dft8(c32* v) {
  constexpr float R = 0.70710678118654752440f;
  c32 a[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = v[i] + v[i + 4];
    a[i + 4] = v[i] - v[i + 4];
  }
  a[5] = {(a[5].r + a[5].i) * R, (a[5].i - a[5].r) * R};   // * W8^1
  a[6] = mul_mi(a[6]);                                     // * W8^2
  a[7] = {(a[7].i - a[7].r) * R, (-a[7].r - a[7].i) * R};  // * W8^3
  dft4(a, v);          // even outputs
  dft4(a + 4, v + 1);  // odd outputs
}

struct MelDenseSource {
  const float* audio;  // [rows, samples]
  int64_t samples;
  int frames;          // 1 + samples / hop (the host computes it)
  struct Row {
    const float* __restrict__ x;
    int64_t samples;
    int frames;
    __device__ __forceinline__ float load(int64_t i) const { return x[i]; }
  };
  __device__ __forceinline__ Row row(int64_t r, int /*hop*/) const { return {audio + r * samples, samples, frames}; }
};

template <class Source>
__global__ __launch_bounds__(MEL_THREADS) void mel_power_kernel(const Source src, const float* __restrict__ window, int win_length,
                                                                int hop, const float* __restrict__ fb,
                                                                const int* __restrict__ bin_lo, const int* __restrict__ bin_hi,
                                                                int n_mels, int out_frames, int tiles, int rows_per_clip,
                                                                float* __restrict__ mel, unsigned int* __restrict__ peak) {
  __shared__ float2 tw512[MEL_HALF];
  __shared__ float2 tw1024[MEL_HALF];
  __shared__ float2 xch_all[MEL_WAVES * MEL_XCH];
  __shared__ float power[MEL_TILE * MEL_PS];
  __shared__ float tile[MEL_MAX_MELS * MEL_TS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x % tiles) * MEL_TILE;
  const typename Source::Row x = src.row(row, hop);  // uniform over the workgroup
  const int64_t samples = x.samples;
  const int pad = out_frames - x.frames;  // zero frames in front of a short clip
  float* __restrict__ out = mel + row * n_mels * (int64_t)out_frames;

  if (tile0 + MEL_TILE <= pad) {  // the whole tile lies in the padding (uniform over the workgroup)
    for (int idx = tid; idx < n_mels * MEL_TILE; idx += MEL_THREADS)
      out[(int64_t)(idx / MEL_TILE) * out_frames + tile0 + (idx % MEL_TILE)] = 0.0f;
    return;
  }

  for (int j = tid; j < MEL_HALF; j += MEL_THREADS) {
    float s, c;
    sincospif(-(float)j * (1.0f / 256.0f), &s, &c);
    tw512[j] = make_float2(c, s);
    sincospif(-(float)j * (1.0f / 512.0f), &s, &c);
    tw1024[j] = make_float2(c, s);
  }
  __syncthreads();
  // the twiddles of a lane are the same for every frame: W512^(lane k0) after pass 1, W512^(8 c k1) after pass 2 and
  // W1024^(lane + 64 k2) in the split
  float2 t1[8], t2[8], t3[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    t1[k] = tw512[lane * k];
    t2[k] = tw512[8 * (lane & 7) * k];
    t3[k] = tw1024[lane + 64 * k];
  }

  // the window values of this lane's sixteen samples: z[64 a + lane] = x[128 a + 2 lane] + i x[128 a + 2 lane + 1]
  const int woff = (MEL_NFFT - win_length) / 2;
  float wr[8], wi[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int q = 128 * a + 2 * lane - woff;
    wr[a] = (q >= 0 && q < win_length) ? window[q] : 0.0f;
    wi[a] = (q + 1 >= 0 && q + 1 < win_length) ? window[q + 1] : 0.0f;
  }

  float2* xch = xch_all + wave * MEL_XCH;
  c32 v[8];
#pragma unroll 1
  for (int f = 0; f < MEL_FPW; ++f) {
    const int fi = wave * MEL_FPW + f;
    const int of = tile0 + fi;
    const int t = of - pad;
    const bool live = of < out_frames && t >= 0;  // uniform over the wave; the barriers below are passed either way
    float* prow = power + fi * MEL_PS;
    if (live) {
      const int64_t base = (int64_t)t * hop - MEL_HALF;
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        float s2[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          int64_t i = base + 128 * a + 2 * lane + e;
          i = i < 0 ? -i : i;
          i = i >= samples ? 2 * (samples - 1) - i : i;
          i = i < 0 ? 0 : (i >= samples ? samples - 1 : i);
          s2[e] = x.load(i);
        }
        v[a] = {s2[0] * wr[a], s2[1] * wi[a]};
      }
      dft8(v);  // over a: lane = 8 b + c now holds k0 = 0..7
#pragma unroll
      for (int k0 = 0; k0 < 8; ++k0) {
        const c32 y = k0 == 0 ? v[0] : cmul(v[k0], t1[k0]);
        xch[k0 * MEL_XS1 + lane] = make_float2(y.r, y.i);
      }
    }
    __syncthreads();
    if (live) {
      const int k0 = lane >> 3, c = lane & 7;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const float2 y = xch[k0 * MEL_XS1 + 8 * b + c];
        v[b] = {y.x, y.y};
      }
      dft8(v);  // over b: lane = 8 k0 + c now holds k1 = 0..7
    }
    __syncthreads();
    if (live) {
      const int k0 = lane >> 3, c = lane & 7;
#pragma unroll
      for (int k1 = 0; k1 < 8; ++k1) {
        const c32 y = k1 == 0 ? v[0] : cmul(v[k1], t2[k1]);
        xch[c * MEL_XS2 + 8 * k1 + k0] = make_float2(y.r, y.i);
      }
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float2 y = xch[c * MEL_XS2 + lane];
        v[c] = {y.x, y.y};
      }
      dft8(v);  // over c: lane = k0 + 8 k1 now holds Z[lane + 64 k2]
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) xch[lane + 64 * k2] = make_float2(v[k2].r, v[k2].i);
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) {
        const int k = lane + 64 * k2;
        const float2 p = xch[(MEL_HALF - k) & (MEL_HALF - 1)];  // Z[512 - k]; Z[0] for k = 0
        const c32 xe = {0.5f * (v[k2].r + p.x), 0.5f * (v[k2].i - p.y)};
        const c32 xo = {0.5f * (v[k2].i + p.y), -0.5f * (v[k2].r - p.x)};  // -i (Z[k] - Z*[512-k]) / 2
        const c32 X = xe + cmul(xo, t3[k2]);
        prow[k] = X.r * X.r + X.i * X.i;
      }
      if (lane == 0) {  // bin 512: W1024^512 = -1, Z[512] = Z[0]
        const float X = v[0].r - v[0].i;
        prow[MEL_HALF] = X * X;
      }
    } else {
      for (int k = lane; k < MEL_BINS; k += 64) prow[k] = 0.0f;
    }
    __syncthreads();  // the exchange buffer is free for the next frame; the power row is complete
  }

  // mel projection of the wave's four frames
  for (int m = lane; m < n_mels; m += 64) {
    int lo = bin_lo[m], hi = bin_hi[m];
    lo = lo < 0 ? 0 : (lo > MEL_BINS ? MEL_BINS : lo);
    hi = hi < lo ? lo : (hi > MEL_BINS ? MEL_BINS : hi);
    float acc[MEL_FPW] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* p0 = power + wave * MEL_FPW * MEL_PS;
    for (int k = lo; k < hi; ++k) {
      const float w = fb[(int64_t)k * n_mels + m];
#pragma unroll
      for (int f = 0; f < MEL_FPW; ++f) acc[f] = fmaf(p0[f * MEL_PS + k], w, acc[f]);
    }
#pragma unroll
    for (int f = 0; f < MEL_FPW; ++f) tile[m * MEL_TS + wave * MEL_FPW + f] = acc[f];
  }
  __syncthreads();

  float mx = 0.0f;
  for (int idx = tid; idx < n_mels * MEL_TILE; idx += MEL_THREADS) {
    const int m = idx / MEL_TILE, fi = idx % MEL_TILE;
    if (tile0 + fi < out_frames) {
      const float val = tile[m * MEL_TS + fi];
      out[(int64_t)m * out_frames + tile0 + fi] = val;
      mx = fmaxf(mx, val);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if (lane == 0 && mx > 0.0f) atomicMax(peak + row / rows_per_clip, __float_as_uint(mx));
}

// what avf_mel_power and avf_mel_power_bank ask of the transform's own arguments
inline int mel_args_ok(const char* who, const float* window, int win_length, int n_fft, int hop, const float* fb,
                       const int32_t* bin_lo, const int32_t* bin_hi, int n_mels, const float* mel, const uint32_t* peak) {
  AVF_REQUIRE(window, "%s: window is null", who);
  AVF_REQUIRE(fb, "%s: fb is null", who);
  AVF_REQUIRE(bin_lo && bin_hi, "%s: bin_lo / bin_hi is null", who);
  AVF_REQUIRE(mel, "%s: mel is null", who);
  AVF_REQUIRE(peak, "%s: peak is null", who);
  AVF_REQUIRE(n_fft == MEL_NFFT, "%s: n_fft is %d, only %d is built", who, n_fft, MEL_NFFT);
  AVF_REQUIRE(win_length >= 1 && win_length <= n_fft, "%s: win_length is %d, outside 1..n_fft", who, win_length);
  AVF_REQUIRE(n_mels >= 1 && n_mels <= MEL_MAX_MELS, "%s: n_mels is %d, outside 1..%d", who, n_mels, MEL_MAX_MELS);
  AVF_REQUIRE(hop >= 1, "%s: hop is %d, below 1", who, hop);
  return 0;
}

}  // namespace
}  // namespace avf
