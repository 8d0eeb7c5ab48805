// mel.hip - the audio stream's wire format on the device: waveform -> mel power -> normalised log-mel spectrogram
// (dataloader/aff2compdataset.py:47-68, 214-247; dataloader/clip_transforms.py:59-108; audio.py restates the transforms).
//
// mel_power_kernel (mel_kernels.hpp: a template over the source of a row's samples; here the dense [rows, samples] tensor),
// ONE launch: a workgroup of four waves makes MEL_TILE = 16 consecutive output frames of one waveform row;
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
#include "mel_kernels.hpp"

namespace avf {
namespace {

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
  AVF_TRY(mel_args_ok("mel_power", window, win_length, n_fft, hop, fb, bin_lo, bin_hi, n_mels, mel, peak));
  AVF_REQUIRE(samples > n_fft / 2, "mel_power: samples is %lld, the reflect padding needs more than n_fft / 2 = %d",
              (long long)samples, n_fft / 2);
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
  const MelDenseSource from{audio, samples, (int)frames};
  mel_power_kernel<<<(unsigned)(rows * tiles), MEL_THREADS, 0, s>>>(from, window, win_length, hop, fb, bin_lo, bin_hi, n_mels,
                                                                     (int)out_frames, (int)tiles, rows_per_clip, mel, peak);
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
