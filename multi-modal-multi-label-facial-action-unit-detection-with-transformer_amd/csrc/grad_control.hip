// grad_control.hip - what the training loop decides about a step BEFORE Adam runs, on the device: the global gradient norm, the
// clipping multiplier derived from it (opts.py --grad_clip: torch.nn.utils.clip_grad_norm_) and the learning-rate multiplier of
// this update (opts.py --n_warmup_steps, and the user's own scale for the epoch decays of train()).  The results land in a
// four-float control block the Adam kernel reads at run time (optim.hip: AdamBatch::ctl), so a captured step follows the
// warm-up and a changed scale without being re-captured, and nothing is copied to the host.
//
//   ctl[0]  learning-rate multiplier of this update: ctl[3] * min(1, step / n_warmup_steps)        (output)
//   ctl[1]  gradient multiplier: min(1, max_norm / (norm + 1e-6)), 1 when clipping is off          (output)
//   ctl[2]  the total gradient norm before clipping, 0 when clipping is off                        (output)
//   ctl[3]  the caller's learning-rate scale                                                       (input)
//
// Two stages.  grad_sumsq_kernel: the tensors are cut into work items of 4096 elements (one workgroup each, found by a binary
// search over a by-value descriptor table, as adam_layer_kernel does); a workgroup squares and sums its elements in fp64 -
// every fp32 and every square of one is exact there, and the kernel waits on memory, not on the fp64 pipe - and stores ONE
// partial to ws[item].  grad_control_finalize_kernel: one workgroup folds the partials and writes the control block.  Every sum
// has a fixed order (lane-strided, butterfly over the wave, waves in index order) and nothing is accumulated with atomics or
// relies on a cleared buffer: the same gradients give the same bits, call after call.
#include "common.hpp"

namespace avf {
namespace {

constexpr int GC_ITEM = 4096;     // elements per work item
constexpr int GC_THREADS = 256;
constexpr int GC_WAVES = GC_THREADS / 64;
constexpr int GC_MAX = 143;       // descriptors per launch (the table is a 3.4 KB kernel argument)

struct GradDesc {
  const float* g;
  int64_t n;
  int item0;  // first work item of this tensor in this launch
};

struct GradTable {
  GradDesc d[GC_MAX];
  int count;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// sum over the workgroup, valid in thread 0: butterfly inside each wave, then the waves in index order
__device__ __forceinline__ double block_sum_f64(double v, double* part) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < GC_WAVES; ++w) s += part[w];
  return s;
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(GC_THREADS) void grad_sumsq_kernel(GradTable t, double* __restrict__ ws) {
  __shared__ double part[GC_WAVES];
  int di = 0;
  {  // the last descriptor whose first work item is <= this one (item0 ascends)
    int hi = t.count - 1;
#pragma unroll 1
    while (di < hi) {
      const int mid = (di + hi + 1) >> 1;
      if ((int)blockIdx.x >= t.d[mid].item0) di = mid;
      else hi = mid - 1;
    }
  }
  const GradDesc d = t.d[di];
  const int64_t base = (int64_t)((int)blockIdx.x - d.item0) * GC_ITEM;
  const float* __restrict__ p = d.g + base;
  const int64_t left = d.n - base;
  const int len = left < GC_ITEM ? (int)left : GC_ITEM;
  // tensors are views at any 4-byte offset of a bucket and of any length: scalar elements up to the first 16-byte boundary,
  // 16-byte loads over the body, scalar elements behind it
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  head = head < len ? head : len;
  const int nvec = (len - head) >> 2, tail = (len - head) & 3;
  const float4* __restrict__ pv = reinterpret_cast<const float4*>(p + head);
  const int tid = threadIdx.x;
  double acc = 0.0;
  if (tid < head) acc += sq(p[tid]);
  // an item has at most 1024 vectors: the (up to) four loads of a lane are issued together
  float4 v[GC_ITEM / 4 / GC_THREADS];
#pragma unroll
  for (int i = 0; i < GC_ITEM / 4 / GC_THREADS; ++i) {
    const int j = tid + i * GC_THREADS;
    v[i] = j < nvec ? pv[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < GC_ITEM / 4 / GC_THREADS; ++i) acc += (sq(v[i].x) + sq(v[i].y)) + (sq(v[i].z) + sq(v[i].w));
  if (tid < tail) acc += sq(p[head + 4 * nvec + tid]);
  const double s = block_sum_f64(acc, part);
  if (tid == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(GC_THREADS) void grad_control_finalize_kernel(const double* __restrict__ ws, int items,
                                                                           float max_norm, int n_warmup_steps,
                                                                           const float* __restrict__ step,
                                                                           float* __restrict__ ctl) {
  __shared__ double part[GC_WAVES];
  double acc = 0.0;
  for (int i = threadIdx.x; i < items; i += GC_THREADS) acc += ws[i];
  const double sum = block_sum_f64(acc, part);
  if (threadIdx.x != 0) return;
  float coef = 1.0f, norm = 0.0f;
  if (max_norm > 0.0f) {
    norm = (float)sqrt(sum);
    // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) in fp32.  The comparison (not fminf) lets a NaN norm
    // through as a NaN multiplier; an infinite norm gives 0.
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  float warm = 1.0f;
  if (n_warmup_steps > 0) {  // LambdaLR(lambda s: min(1, (s + 1) / n)): `step` is the number of THIS update, from 1
    const float w = (step ? step[0] : 1.0f) / (float)n_warmup_steps;
    warm = w < 1.0f ? w : 1.0f;
  }
  ctl[0] = ctl[3] * warm;
  ctl[1] = coef;
  ctl[2] = norm;
}

int64_t items_of(int64_t numel) { return numel > 0 ? (numel + GC_ITEM - 1) / GC_ITEM : 0; }

}  // namespace
}  // namespace avf

extern "C" size_t avf_grad_control_workspace_bytes(int count, const int64_t* numel) {
  using namespace avf;
  if (count < 0 || (count > 0 && !numel)) {
    set_error("grad_control_workspace_bytes: bad arguments");
    return 0;
  }
  int64_t items = 0;
  for (int i = 0; i < count; ++i) items += items_of(numel[i]);
  return (size_t)items * sizeof(double);
}

extern "C" int avf_grad_control(int count, const float* const* g, const int64_t* numel, float max_norm, int n_warmup_steps,
                                const float* step, float* ctl, void* ws, void* stream) {
  using namespace avf;
  AVF_REQUIRE(ctl && count >= 0 && n_warmup_steps >= 0, "grad_control: bad arguments");
  AVF_REQUIRE(n_warmup_steps == 0 || step, "grad_control: a warm-up needs the device step counter");
  hipStream_t s = (hipStream_t)stream;
  int64_t items = 0;  // partials written so far
  if (max_norm > 0.0f) {
    AVF_REQUIRE(count == 0 || (g && numel), "grad_control: null pointer");
    GradTable t;
    t.count = 0;
    int pending = 0;  // work items of the table being collected
    auto flush = [&]() -> int {
      if (t.count == 0) return 0;
      grad_sumsq_kernel<<<pending, GC_THREADS, 0, s>>>(t, reinterpret_cast<double*>(ws) + items);
      items += pending;
      t.count = 0;
      pending = 0;
      return check_launch("grad_sumsq_kernel");
    };
    for (int i = 0; i < count; ++i) {
      if (!g[i] || numel[i] <= 0) continue;
      AVF_REQUIRE(ws, "grad_control: workspace missing");
      AVF_REQUIRE((reinterpret_cast<uintptr_t>(g[i]) & 3u) == 0, "grad_control: gradient %d is not 4-byte aligned", i);
      const int64_t it = items_of(numel[i]);
      AVF_REQUIRE(items + pending + it < (1LL << 31), "grad_control: too many elements");
      if (t.count == GC_MAX) AVF_TRY(flush());
      GradDesc& d = t.d[t.count++];
      d.g = g[i];
      d.n = numel[i];
      d.item0 = pending;
      pending += (int)it;
    }
    AVF_TRY(flush());
  }
  grad_control_finalize_kernel<<<1, GC_THREADS, 0, s>>>(reinterpret_cast<const double*>(ws), (int)items, max_norm, n_warmup_steps,
                                                        step, ctl);
  return check_launch("grad_control_finalize_kernel");
}
