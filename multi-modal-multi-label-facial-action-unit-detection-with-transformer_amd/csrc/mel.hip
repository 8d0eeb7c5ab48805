// mel.hip - the audio stream's wire format on the device: waveform -> mel power -> normalised log-mel spectrogram
// (dataloader/aff2compdataset.py:47-68, 214-247; dataloader/clip_transforms.py:59-108; audio.py restates the transforms).
//
// mel_power_kernel, ONE launch: a workgroup of four waves makes MEL_TILE = 16 consecutive output frames of one waveform row;
// each wave makes four of them, one after the other.  Nothing but the waveform is read and nothing but the mel tile is written:
//   * framing, the reflect padding, the window and the zero frames in front of a short clip are index arithmetic.  Frame t
//     covers padded samples [t hop, t hop + 1024); padded index p is sample i = p - 512, -i for i < 0, 2 (S - 1) - i for
//     i >= S (S > 512 keeps both inside the row; the index is clamped to the row all the same).  Output frame `of` is frame
//     of - (out_frames - frames); a negative one is a zero column.
//   * the real 1024-point FFT is a 512-point complex FFT of z[n] = x[2n] + i x[2n+1].  512 = 8 * 8 * 8: with n = 64 a + 8 b + c
//     and k = k0 + 8 k1 + 64 k2,
//         Z[k] = sum_c W8^(c k2) W512^(8 c k1) [ sum_b W8^(b k1) W512^((8 b + c) k0) [ sum_a W8^(a k0) z[n] ] ],
//     three radix-8 passes with eight complex values per lane in registers: lane 8 b + c transforms over a, lane 8 k0 + c over
//     b, lane k0 + 8 k1 over c, so that lane L ends with Z[L + 64 k2].  Two exchanges through the wave's LDS buffer lie between
//     the passes, a third one serves the real-FFT split X[k] = (Z[k] + Z*[512-k]) / 2 - i W1024^k (Z[k] - Z*[512-k]) / 2.
//   * the twiddles W512^j and W1024^j (j < 512) are two LDS tables built once per workgroup by sincospif from arguments
//     -j/256 and -j/512, which fp32 holds exactly; a lane keeps the 22 it needs in registers over its frames.  All arithmetic
//     is fp32 on the vector pipe: a loud bin leaks into a bin 80 dB below it by rounding error alone, and top_db shows
//     exactly that.
//   * |X[k]|^2 of the wave's four frames goes to LDS; lane m (and m + 64) then sums power[k] * fb[k, m] over its filter's own
//     bins [lo_m, hi_m) for the four frames at once, reading each weight once.  fb is the module's dense fp32 filterbank and
//     lo / hi come from its non-zeros, so both backends of audio.MelFrontEnd use the same weights.
//   * the n_mels x 16 tile is staged in LDS and stored with the frames contiguous; its maximum goes to peak[row / rows_per_clip]
//     by atomicMax on the bit pattern (power >= 0: unsigned order is float order; a maximum does not depend on the order).
// LDS: 8 KiB of tables + 4 x 4.5 KiB exchange + 32.25 KiB of power + 8.5 KiB of tile = 66.75 KiB, two workgroups per CU;
// 144 VGPRs, no scratch.
//
// mel_db_norm_kernel, ONE launch, in place: (max(10 log10(max(x, 1e-10)), 10 log10(max(peak, 1e-10)) - top_db) - mean) / std.
// The logarithm and the normalisation are fp64 with one rounding to fp32 at the store (the pass is bound by its 8 bytes per
// element, not by the fp64 pipe).  A workgroup takes 4096 consecutive elements of ONE clip: scalar elements up to the first
// 16-byte boundary, 16-byte accesses over the body, scalar elements behind it.
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

__global__ __launch_bounds__(MEL_THREADS) void mel_power_kernel(const float* __restrict__ audio, int64_t samples,
                                                                const float* __restrict__ window, int win_length, int hop,
                                                                const float* __restrict__ fb, const int* __restrict__ bin_lo,
                                                                const int* __restrict__ bin_hi, int n_mels, int frames,
                                                                int out_frames, int tiles, int rows_per_clip,
                                                                float* __restrict__ mel, unsigned int* __restrict__ peak) {
  __shared__ float2 tw512[MEL_HALF];
  __shared__ float2 tw1024[MEL_HALF];
  __shared__ float2 xch_all[MEL_WAVES * MEL_XCH];
  __shared__ float power[MEL_TILE * MEL_PS];
  __shared__ float tile[MEL_MAX_MELS * MEL_TS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x % tiles) * MEL_TILE;
  const int pad = out_frames - frames;  // zero frames in front of a short clip
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

  const float* __restrict__ x = audio + row * samples;
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
          s2[e] = x[i];
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

constexpr int DBN_ITEM = 4096;  // elements per workgroup
constexpr int DBN_THREADS = 256;

__device__ __forceinline__ float db_norm_one(float x, double floor_db, double mean, double std) {
  const double xd = (double)x;
  double db = 10.0 * log10(xd > 1e-10 ? xd : 1e-10);
  db = db > floor_db ? db : floor_db;
  return (float)((db - mean) / std);
}

__global__ __launch_bounds__(DBN_THREADS) void mel_db_norm_kernel(float* __restrict__ mel,
                                                                  const unsigned int* __restrict__ peak,
                                                                  int64_t clip_elems, int items_per_clip, double top_db,
                                                                  double mean, double std) {
  const int64_t clip = blockIdx.x / items_per_clip;
  const int64_t first = (int64_t)(blockIdx.x % items_per_clip) * DBN_ITEM;
  const int64_t left = clip_elems - first;
  const int len = left < DBN_ITEM ? (int)left : DBN_ITEM;
  float* __restrict__ p = mel + clip * clip_elems + first;
  const double pk = (double)__uint_as_float(peak[clip]);
  const double floor_db = 10.0 * log10(pk > 1e-10 ? pk : 1e-10) - top_db;
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  head = head < len ? head : len;
  const int nvec = (len - head) >> 2, tail = (len - head) & 3;
  float4* __restrict__ pv = reinterpret_cast<float4*>(p + head);
  const int tid = threadIdx.x;
  if (tid < head) p[tid] = db_norm_one(p[tid], floor_db, mean, std);
  float4 v[DBN_ITEM / 4 / DBN_THREADS];
#pragma unroll
  for (int i = 0; i < DBN_ITEM / 4 / DBN_THREADS; ++i) {
    const int j = tid + i * DBN_THREADS;
    if (j < nvec) v[i] = pv[j];
  }
#pragma unroll
  for (int i = 0; i < DBN_ITEM / 4 / DBN_THREADS; ++i) {
    const int j = tid + i * DBN_THREADS;
    if (j < nvec)
      pv[j] = make_float4(db_norm_one(v[i].x, floor_db, mean, std), db_norm_one(v[i].y, floor_db, mean, std),
                          db_norm_one(v[i].z, floor_db, mean, std), db_norm_one(v[i].w, floor_db, mean, std));
  }
  if (tid < tail) {
    float* q = p + head + 4 * nvec + tid;
    *q = db_norm_one(*q, floor_db, mean, std);
  }
}

}  // namespace
}  // namespace avf

extern "C" int avf_mel_power(const float* audio, int64_t rows, int64_t samples, const float* window, int win_length, int n_fft,
                             int hop, const float* fb, const int32_t* bin_lo, const int32_t* bin_hi, int n_mels,
                             int full_frames, int rows_per_clip, float* mel, uint32_t* peak, void* stream) {
  using namespace avf;
  AVF_REQUIRE(audio, "mel_power: audio is null");
  AVF_REQUIRE(window, "mel_power: window is null");
  AVF_REQUIRE(fb, "mel_power: fb is null");
  AVF_REQUIRE(bin_lo && bin_hi, "mel_power: bin_lo / bin_hi is null");
  AVF_REQUIRE(mel, "mel_power: mel is null");
  AVF_REQUIRE(peak, "mel_power: peak is null");
  AVF_REQUIRE(n_fft == MEL_NFFT, "mel_power: n_fft is %d, only %d is built", n_fft, MEL_NFFT);
  AVF_REQUIRE(samples > n_fft / 2, "mel_power: samples is %lld, the reflect padding needs more than n_fft / 2 = %d",
              (long long)samples, n_fft / 2);
  AVF_REQUIRE(win_length >= 1 && win_length <= n_fft, "mel_power: win_length is %d, outside 1..n_fft", win_length);
  AVF_REQUIRE(n_mels >= 1 && n_mels <= MEL_MAX_MELS, "mel_power: n_mels is %d, outside 1..%d", n_mels, MEL_MAX_MELS);
  AVF_REQUIRE(hop >= 1, "mel_power: hop is %d, below 1", hop);
  AVF_REQUIRE(rows >= 1, "mel_power: rows is %lld, below 1", (long long)rows);
  AVF_REQUIRE(rows_per_clip >= 1 && rows % rows_per_clip == 0, "mel_power: rows_per_clip is %d, no divisor of rows = %lld",
              rows_per_clip, (long long)rows);
  AVF_REQUIRE(full_frames >= 0, "mel_power: full_frames is %d, below 0", full_frames);
  const int64_t frames = 1 + samples / hop;
  const int64_t out_frames = frames > full_frames ? frames : full_frames;
  const int64_t tiles = (out_frames + MEL_TILE - 1) / MEL_TILE;
  AVF_REQUIRE(out_frames < (1LL << 30) && rows * tiles < (1LL << 31), "mel_power: samples / rows give too many frames");
  hipStream_t s = (hipStream_t)stream;
  const int64_t clips = rows / rows_per_clip;
  const hipError_t e = hipMemsetAsync(peak, 0, (size_t)clips * sizeof(uint32_t), s);
  if (e != hipSuccess) {
    set_error("mel_power: zeroing peak: %s", hipGetErrorString(e));
    return 2;
  }
  mel_power_kernel<<<(unsigned)(rows * tiles), MEL_THREADS, 0, s>>>(audio, samples, window, win_length, hop, fb, bin_lo, bin_hi,
                                                                     n_mels, (int)frames, (int)out_frames, (int)tiles,
                                                                     rows_per_clip, mel, peak);
  return check_launch("mel_power_kernel");
}

extern "C" int avf_mel_db_norm(float* mel, const uint32_t* peak, int64_t rows, int n_mels, int64_t frames, int rows_per_clip,
                               double top_db, double mean, double std, void* stream) {
  using namespace avf;
  AVF_REQUIRE(mel, "mel_db_norm: mel is null");
  AVF_REQUIRE(peak, "mel_db_norm: peak is null");
  AVF_REQUIRE(n_mels >= 1 && n_mels <= MEL_MAX_MELS, "mel_db_norm: n_mels is %d, outside 1..%d", n_mels, MEL_MAX_MELS);
  AVF_REQUIRE(rows >= 1 && frames >= 1 && frames < (1LL << 30), "mel_db_norm: rows / frames is below 1 (or frames too large)");
  AVF_REQUIRE(rows_per_clip >= 1 && rows % rows_per_clip == 0, "mel_db_norm: rows_per_clip is %d, no divisor of rows = %lld",
              rows_per_clip, (long long)rows);
  AVF_REQUIRE(std != 0.0, "mel_db_norm: std is 0");
  AVF_REQUIRE(((uintptr_t)mel & 3u) == 0, "mel_db_norm: mel is not 4-byte aligned");
  const int64_t clips = rows / rows_per_clip;
  const int64_t clip_elems = (int64_t)rows_per_clip * n_mels * frames;
  const int64_t items = (clip_elems + DBN_ITEM - 1) / DBN_ITEM;
  AVF_REQUIRE(items < (1LL << 31) && clips * items < (1LL << 31), "mel_db_norm: rows / frames give too many elements");
  mel_db_norm_kernel<<<(unsigned)(clips * items), DBN_THREADS, 0, (hipStream_t)stream>>>(mel, peak, clip_elems, (int)items,
                                                                                         top_db, mean, std);
  return check_launch("mel_db_norm_kernel");
}
