// mel_bank.hip - audio windows assembled on the device from a resident waveform bank: wave fp32 / int16 [total] (the wavs of a
// data set split, one after the other), wav_start / wav_len int64 [V], wav_of int32 [F] (the wav of every sample), end_sample
// int64 [F] and index int64 [B] -> the window of every sample, by the data loader's rule (dataloader/aff2compdataset.py:214-247;
// testset.py:164-198 repeats it).  Only index [B] travels per step.
//
// The rule, in integers.  N = sample_len_secs * sample_rate, w = int(window_size * sample_rate) (= win_length), shift =
// audio_shift_secs * sample_rate, half = n_fft / 2.  For sample i = index[b] with E = end_sample[i], whose wav has L samples:
//     num = min(N, max(E, w))                 (220-223)  torchaudio.load(num_frames=...)
//     off = max(E - N + shift, 0)             (224-226)  torchaudio.load(offset=...)
//     got = max(0, min(num, L - off))                    a load past the end of the file returns what is there
//   got > half:   the clip is wav[off : off + got]; 1 + got / hop frames of mel power, computed on exactly these samples with
//                 the reflect padding at THEIR ends (228), right-aligned in full_frames columns, zero columns in front (234-238);
//                 `audio` is the same samples right-aligned in N zeros (243-246).
//   got <= half:  the transform raises and the except branch takes N zeros (229-232): every column is 0 power, audio is all 0.
// This project's definitions (the reference would raise before its try; nothing on the device can): an index outside [0, F)
// and a sample whose wav is absent (L == 0) are silent.  A table entry that points outside its array (wav_of outside [0, V),
// wav_start / wav_len outside wave) is silent as well: nothing outside [wave, wave + total) is ever read.
// An int16 sample x is worth x * 2^-15, exact in fp32.
//
// avf_mel_power_bank  one memset of peak + ONE launch: mel.hip's mel_power_kernel (mel_kernels.hpp) with the bank as its source.
//                     The source's row() is two dependent loads, index[b], then end_sample / wav_of, then wav_start / wav_len,
//                     all with addresses that are uniform over the workgroup; load(i) converts int16.  A silent row has no
//                     frames: every tile of it writes zero columns and reads nothing of the bank.
// avf_wave_gather     ONE launch: bank -> audio fp32 [B, N].  A workgroup takes 4096 consecutive output elements of ONE row:
//                     scalar stores up to the first 16-byte boundary of the destination, 16-byte stores over the body, scalar
//                     stores behind it.  The source is read element by element (a lane's four are neighbours), so source and
//                     destination need not sit alike in their 16-byte chunks; an element in front of the window is 0 and reads
//                     nothing.
//
// gfx950 resources: DESIGN.md section 9.
#include "mel_kernels.hpp"

namespace avf {
namespace {

struct WaveTables {
  const int64_t* wav_start;   // [V]
  const int64_t* wav_len;     // [V]
  const int32_t* wav_of;      // [F]
  const int64_t* end_sample;  // [F]
  const int64_t* index;       // [B]
  int64_t F, V, total;        // total: elements of wave
  int64_t N, w, shift;        // 1 <= w, 0 <= shift, 1 <= N, all below 2^40 (the host checks)
};

struct WaveWindow {
  int64_t first;  // of the window in wave
  int64_t got;    // 0: silent
};

// the rule above for row b; every load has an address that depends on b alone
__device__ __forceinline__ WaveWindow wave_window(const WaveTables& t, int64_t b) {
  const int64_t i = t.index[b];
  if (i < 0 || i >= t.F) return {0, 0};
  const int64_t v = t.wav_of[i];
  int64_t E = t.end_sample[i];
  if (v < 0 || v >= t.V) return {0, 0};
  const int64_t s0 = t.wav_start[v], L = t.wav_len[v];
  if (s0 < 0 || L < 0 || s0 > t.total || L > t.total - s0) return {0, 0};
  const int64_t lim = (int64_t)1 << 60;
  E = E < -lim ? -lim : (E > lim ? lim : E);  // E - N + shift cannot overflow
  int64_t num = E > t.w ? E : t.w;
  num = num < t.N ? num : t.N;
  int64_t off = E - t.N + t.shift;
  off = off > 0 ? off : 0;
  const int64_t got = num < L - off ? num : L - off;
  if (got <= MEL_HALF) return {0, 0};
  return {s0 + off, got};
}

__device__ __forceinline__ float wave_value(float x) { return x; }
__device__ __forceinline__ float wave_value(int16_t x) { return (float)x * (1.0f / 32768.0f); }

template <class T>
struct MelBankSource {
  const T* wave;
  WaveTables t;
  struct Row {
    const T* __restrict__ x;
    int64_t samples;
    int frames;
    __device__ __forceinline__ float load(int64_t i) const { return wave_value(x[i]); }
  };
  __device__ __forceinline__ Row row(int64_t b, int hop) const {
    const WaveWindow win = wave_window(t, b);
    return {wave + win.first, win.got, win.got > 0 ? (int)(1 + win.got / hop) : 0};
  }
};

constexpr int WG_ITEM = 4096;  // elements per workgroup
constexpr int WG_THREADS = 256;

template <class T>
__global__ __launch_bounds__(WG_THREADS) void wave_gather_kernel(const T* __restrict__ wave, const WaveTables t,
                                                                 float* __restrict__ dst, int items_per_row) {
  const int64_t b = blockIdx.x / items_per_row;
  const int64_t first = (int64_t)(blockIdx.x % items_per_row) * WG_ITEM;
  const int64_t left = t.N - first;
  const int len = left < WG_ITEM ? (int)left : WG_ITEM;
  const WaveWindow win = wave_window(t, b);
  // element j of this item is sample j - lead of the window, lead = (N - got) - first; first + j < N keeps it below got
  const int64_t lead = t.N - win.got - first;
  const T* __restrict__ x = wave + win.first;
  float* __restrict__ p = dst + b * t.N + first;
  auto value = [&](int j) -> float { return j >= lead ? wave_value(x[j - lead]) : 0.0f; };
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  head = head < len ? head : len;
  const int nvec = (len - head) >> 2, tail = (len - head) & 3;
  float4* __restrict__ pv = reinterpret_cast<float4*>(p + head);
  const int tid = threadIdx.x;
  if (tid < head) p[tid] = value(tid);
#pragma unroll
  for (int i = 0; i < WG_ITEM / 4 / WG_THREADS; ++i) {
    const int j = tid + i * WG_THREADS;
    if (j < nvec) {
      const int e = head + 4 * j;
      pv[j] = make_float4(value(e), value(e + 1), value(e + 2), value(e + 3));
    }
  }
  if (tid < tail) {
    const int e = head + 4 * nvec + tid;
    p[e] = value(e);
  }
}

// what the two entry points ask of the bank, the tables and the rule; fills the tables
int wave_tables(const char* who, const void* wave, int wave_dtype, int64_t total, const int64_t* wav_start, const int64_t* wav_len,
                int64_t V, const int32_t* wav_of, const int64_t* end_sample, int64_t F, const int64_t* index, int64_t B, int64_t N,
                int64_t w, int64_t shift, WaveTables* out) {
  AVF_REQUIRE(wave, "%s: wave is null", who);
  AVF_REQUIRE(wave_dtype == 0 || wave_dtype == 1, "%s: wave_dtype is %d, neither 0 (fp32) nor 1 (int16)", who, wave_dtype);
  AVF_REQUIRE(wav_start && wav_len, "%s: wav_start / wav_len is null", who);
  AVF_REQUIRE(wav_of, "%s: wav_of is null", who);
  AVF_REQUIRE(end_sample, "%s: end_sample is null", who);
  AVF_REQUIRE(index, "%s: index is null", who);
  AVF_REQUIRE(((uintptr_t)wave & (wave_dtype == 0 ? 3u : 1u)) == 0, "%s: wave is not aligned to its element", who);
  AVF_REQUIRE((((uintptr_t)wav_start | (uintptr_t)wav_len | (uintptr_t)end_sample | (uintptr_t)index) & 7u) == 0 &&
                  ((uintptr_t)wav_of & 3u) == 0,
              "%s: a table is not aligned to its element", who);
  const int64_t lim = (int64_t)1 << 40;
  AVF_REQUIRE(total >= 1 && total < ((int64_t)1 << 60), "%s: total is %lld, below 1 (or too large)", who, (long long)total);
  AVF_REQUIRE(V >= 1 && F >= 1 && B >= 1, "%s: V / F / B is below 1", who);
  AVF_REQUIRE(N >= 1 && N < lim, "%s: N is %lld, outside 1..2^40", who, (long long)N);
  AVF_REQUIRE(w >= 1 && w < lim, "%s: w is %lld, outside 1..2^40", who, (long long)w);
  AVF_REQUIRE(shift >= 0 && shift < lim, "%s: shift is %lld, outside 0..2^40", who, (long long)shift);
  *out = WaveTables{wav_start, wav_len, wav_of, end_sample, index, F, V, total, N, w, shift};
  return 0;
}

// dst [n bytes] must not touch the bank
int wave_apart(const char* who, const void* wave, int wave_dtype, int64_t total, const void* dst, int64_t n) {
  const uintptr_t b0 = (uintptr_t)wave, b1 = b0 + (uintptr_t)total * (wave_dtype == 0 ? 4u : 2u), d0 = (uintptr_t)dst;
  AVF_REQUIRE(d0 + (uintptr_t)n <= b0 || b1 <= d0, "%s: dst overlaps the bank", who);
  return 0;
}

}  // namespace
}  // namespace avf

extern "C" int avf_mel_power_bank(const void* wave, int wave_dtype, int64_t total, const int64_t* wav_start, const int64_t* wav_len,
                                  int64_t V, const int32_t* wav_of, const int64_t* end_sample, int64_t F, const int64_t* index,
                                  int64_t B, int64_t N, int64_t shift, const float* window, int win_length, int n_fft, int hop,
                                  const float* fb, const int32_t* bin_lo, const int32_t* bin_hi, int n_mels, int full_frames,
                                  float* mel, uint32_t* peak, void* stream) {
  using namespace avf;
  const char* who = "mel_power_bank";
  AVF_TRY(mel_args_ok(who, window, win_length, n_fft, hop, fb, bin_lo, bin_hi, n_mels, mel, peak));
  WaveTables t;
  AVF_TRY(wave_tables(who, wave, wave_dtype, total, wav_start, wav_len, V, wav_of, end_sample, F, index, B, N, win_length, shift, &t));
  AVF_REQUIRE(full_frames >= 1 + N / hop, "%s: full_frames is %d, a window of N = %lld samples has %lld frames", who, full_frames,
              (long long)N, (long long)(1 + N / hop));
  const int64_t out_frames = full_frames;
  const int64_t tiles = (out_frames + MEL_TILE - 1) / MEL_TILE;
  AVF_REQUIRE(out_frames < (1LL << 30) && B < (1LL << 31) && B * tiles < (1LL << 31), "%s: N / B give too many frames", who);
  AVF_TRY(wave_apart(who, wave, wave_dtype, total, mel, B * n_mels * out_frames * 4));
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(peak, 0, (size_t)B * sizeof(uint32_t), s);
  if (e != hipSuccess) {
    set_error("%s: zeroing peak: %s", who, hipGetErrorString(e));
    return 2;
  }
  if (wave_dtype == 0) {
    const MelBankSource<float> from{(const float*)wave, t};
    mel_power_kernel<<<(unsigned)(B * tiles), MEL_THREADS, 0, s>>>(from, window, win_length, hop, fb, bin_lo, bin_hi, n_mels,
                                                                    (int)out_frames, (int)tiles, 1, mel, peak);
  } else {
    const MelBankSource<int16_t> from{(const int16_t*)wave, t};
    mel_power_kernel<<<(unsigned)(B * tiles), MEL_THREADS, 0, s>>>(from, window, win_length, hop, fb, bin_lo, bin_hi, n_mels,
                                                                    (int)out_frames, (int)tiles, 1, mel, peak);
  }
  return check_launch("mel_power_kernel (bank)");
}

extern "C" int avf_wave_gather(const void* wave, int wave_dtype, int64_t total, const int64_t* wav_start, const int64_t* wav_len,
                               int64_t V, const int32_t* wav_of, const int64_t* end_sample, int64_t F, const int64_t* index, int64_t B,
                               int64_t N, int64_t w, int64_t shift, float* dst, void* stream) {
  using namespace avf;
  const char* who = "wave_gather";
  AVF_REQUIRE(dst, "%s: dst is null", who);
  AVF_REQUIRE(((uintptr_t)dst & 3u) == 0, "%s: dst is not 4-byte aligned", who);
  WaveTables t;
  AVF_TRY(wave_tables(who, wave, wave_dtype, total, wav_start, wav_len, V, wav_of, end_sample, F, index, B, N, w, shift, &t));
  const int64_t items = ceil_div(N, WG_ITEM);
  AVF_REQUIRE(B < (1LL << 31) && B * items < (1LL << 31), "%s: B * N gives too many elements", who);   // B * N < 2^43
  AVF_TRY(wave_apart(who, wave, wave_dtype, total, dst, B * N * 4));
  hipStream_t s = (hipStream_t)stream;
  if (wave_dtype == 0)
    wave_gather_kernel<<<(unsigned)(B * items), WG_THREADS, 0, s>>>((const float*)wave, t, dst, (int)items);
  else
    wave_gather_kernel<<<(unsigned)(B * items), WG_THREADS, 0, s>>>((const int16_t*)wave, t, dst, (int)items);
  return check_launch("wave_gather_kernel");
}
