// eval_metrics.hip - the evaluation half of the reference's epoch (train.py:106-169: evaluate) on the model's [rows, 21] output
// row.  The reference copies three prediction arrays to the host per validation batch and runs numpy / sklearn on the stacked
// arrays at the end; every one of its metrics is a function of plain sums over rows, so here ONE launch per batch adds the
// batch's sufficient statistics into a 128-word fp64 state on the device, and one more launch turns the state into the scores:
//
//   EX  AccF1Metric (accf1.py:20-42)      7 x 7 confusion counts [label][argmax]   -> accuracy, macro F1 over sklearn's label set
//   AU  MultiLabelAccF1 (accf1.py:45-77)  tp, fp, fn, correct, labelled per unit   -> accuracy, mean binary F1
//   VA  CCCMetric (cccmetric.py:4-89)     n, sum x, y, x^2, y^2, x y per column    -> CCC with biased moments
//
// Structure: a single workgroup of 16 waves walks the rows 1024 at a time.  Counts are integers all the way: the AU and VA
// counts are wave ballots whose population counts lane 0 adds to LDS, the EX confusion entry is one LDS integer add per row.
// The ten fp64 moments are summed per lane, folded over the lanes of a wave by a butterfly and over the waves in index order
// by the thread that owns the slot - a fixed order, so a sequence of calls always gives the same words.  No floating-point
// atomics, no workspace, no host synchronisation.
#include "common.hpp"

namespace avf {
namespace {

constexpr int EM_THREADS = 1024;
constexpr int EM_WAVES = EM_THREADS / 64;
constexpr int NEX = AVF_TASK_LOSS_EX_CLASSES;  // 7
constexpr int NAU = AVF_TASK_LOSS_AU_UNITS;    // 12
constexpr int NCONF = NEX * NEX;               // 49
constexpr int NCNT = NCONF + 5 * NAU + 2;      // integer counts of one batch: confusion, AU statistics, VA n
constexpr int NMOM = 10;                       // (sum x, y, x^2, y^2, x y) x 2 columns
static_assert(AVF_EVAL_AU_STATS == NCONF && AVF_EVAL_VA_MOMENTS == NCONF + 5 * NAU && AVF_EVAL_LOSS_SUM == AVF_EVAL_VA_MOMENTS + 12 &&
              AVF_EVAL_LOSS_STEPS < AVF_EVAL_STATE_WORDS, "state layout");

// torch.argmax over the seven logits: the first maximal index, a NaN counting as maximal
__device__ __forceinline__ int argmax7(const float* __restrict__ z) {
  float best = z[0];
  int idx = 0;
#pragma unroll
  for (int j = 1; j < NEX; ++j) {
    const float v = z[j];
    const bool take = !(best != best) && (v > best || v != v);
    best = take ? v : best;
    idx = take ? j : idx;
  }
  return idx;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(EM_THREADS) void eval_update_kernel(const float* __restrict__ out, int64_t ldo,
                                                                 const int64_t* __restrict__ y_ex,
                                                                 const float* __restrict__ y_au, int64_t ld_au,
                                                                 const float* __restrict__ y_va, int64_t ld_va,
                                                                 const float* __restrict__ loss, const avf_eval_cfg c, int rows,
                                                                 double* __restrict__ state, uint8_t* __restrict__ pred_au,
                                                                 int64_t* __restrict__ pred_ex, float* __restrict__ pred_va) {
  __shared__ unsigned cnt[NCNT];
  __shared__ double mom[EM_WAVES][NMOM];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool do_ex = state && y_ex, do_au = state && y_au, do_va = state && y_va;
  for (int i = tid; i < NCNT; i += EM_THREADS) cnt[i] = 0u;
  __syncthreads();

  unsigned* const au = cnt + NCONF;  // [5][NAU]
  double m[NMOM];
#pragma unroll
  for (int k = 0; k < NMOM; ++k) m[k] = 0.0;

  // every wave makes the same number of steps as its lanes do: the ballots below sit in uniform control flow
  for (int r0 = wave * 64; r0 < rows; r0 += EM_THREADS) {
    const int r = r0 + lane;
    const bool in = r < rows;
    const float* o = out + (int64_t)(in ? r : 0) * ldo;
    if (in && (do_ex || pred_ex)) {
      const int p = argmax7(o + c.ex_col);
      if (pred_ex) pred_ex[r] = p;
      if (do_ex) {
        const int64_t t = y_ex[r];
        if (t != c.ex_ignore && t >= 0 && t < NEX) atomicAdd(&cnt[(int)t * NEX + p], 1u);
      }
    }
    if (do_au || pred_au) {
#pragma unroll
      for (int u = 0; u < NAU; ++u) {
        const bool p = in && o[c.au_col + u] > 0x1p-23f;
        if (in && pred_au) pred_au[(int64_t)r * NAU + u] = p ? 1 : 0;
        if (do_au) {
          const float y = in ? y_au[(int64_t)r * ld_au + u] : c.au_ignore;
          const bool keep = in && y != c.au_ignore;
          const unsigned long long K = __ballot(keep), P = __ballot(keep && p), T = __ballot(keep && y == 1.0f),
                                   Z = __ballot(keep && y == 0.0f);
          if (lane == 0) {  // the wave's counts of this step, one LDS integer add each
            const unsigned tp = __popcll(P & T);
            atomicAdd(&au[u], tp);
            atomicAdd(&au[NAU + u], (unsigned)__popcll(P & ~T));
            atomicAdd(&au[2 * NAU + u], (unsigned)__popcll(~P & T));
            atomicAdd(&au[3 * NAU + u], tp + (unsigned)__popcll(~P & Z));
            atomicAdd(&au[4 * NAU + u], (unsigned)__popcll(K));
          }
        }
      }
    }
    if (do_va || pred_va) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float x = 0.f;
        if (in) {
          x = o[c.va_col + j];
          x = c.va_tanh ? tanhf(x) : x;
          if (pred_va) pred_va[(int64_t)r * 2 + j] = x;
        }
        if (do_va) {
          const float y = in ? y_va[(int64_t)r * ld_va + j] : c.va_ignore;
          const bool ok = in && y != c.va_ignore;
          const unsigned long long V = __ballot(ok);
          if (lane == 0) atomicAdd(&cnt[NCONF + 5 * NAU + j], (unsigned)__popcll(V));
          if (ok) {
            const double dx = x, dy = y;
            m[5 * j] += dx;
            m[5 * j + 1] += dy;
            m[5 * j + 2] += dx * dx;
            m[5 * j + 3] += dy * dy;
            m[5 * j + 4] += dx * dy;
          }
        }
      }
    }
  }
  if (!state) return;

  if (do_va) {
#pragma unroll
    for (int k = 0; k < NMOM; ++k) {
      const double s = wave_sum_f64(m[k]);
      if (lane == 0) mom[wave][k] = s;
    }
  }
  __syncthreads();

  // one thread per state word: read, add, write
  if (tid < AVF_EVAL_VA_MOMENTS) {
    if (tid < NCONF ? do_ex : do_au) state[tid] += (double)cnt[tid];
  } else if (tid < AVF_EVAL_LOSS_SUM) {
    if (do_va) {
      const int j = (tid - AVF_EVAL_VA_MOMENTS) / 6, k = (tid - AVF_EVAL_VA_MOMENTS) % 6;
      double s;
      if (k == 0) {
        s = (double)cnt[NCONF + 5 * NAU + j];
      } else {
        s = 0.0;
        for (int w = 0; w < EM_WAVES; ++w) s += mom[w][5 * j + k - 1];
      }
      state[tid] += s;
    }
  } else if (tid == AVF_EVAL_LOSS_SUM) {
    if (loss) state[tid] += (double)loss[0];
  } else if (tid == AVF_EVAL_LOSS_STEPS) {
    if (loss) state[tid] += 1.0;
  }
}

__global__ __launch_bounds__(AVF_EVAL_STATE_WORDS) void eval_scores_kernel(const double* __restrict__ state,
                                                                           double* __restrict__ scores) {
  __shared__ double s[AVF_EVAL_STATE_WORDS];
  s[threadIdx.x] = state[threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  // EX
  double kept = 0.0, hit = 0.0, f1_sum = 0.0, present = 0.0;
  for (int cl = 0; cl < NEX; ++cl) {
    double as_label = 0.0, as_pred = 0.0;
    for (int k = 0; k < NEX; ++k) {
      as_label += s[AVF_EVAL_EX_CONF + cl * NEX + k];
      as_pred += s[AVF_EVAL_EX_CONF + k * NEX + cl];
    }
    const double tp = s[AVF_EVAL_EX_CONF + cl * NEX + cl];
    kept += as_label;
    hit += tp;
    if (as_label + as_pred > 0.0) {
      f1_sum += 2.0 * tp / (as_label + as_pred);
      present += 1.0;
    }
  }
  const double ex_acc = kept > 0.0 ? hit / kept : nan, ex_f1 = present > 0.0 ? f1_sum / present : nan;
  // AU
  const double* a = s + AVF_EVAL_AU_STATS;
  double correct = 0.0, labelled = 0.0, au_f1 = 0.0;
  for (int u = 0; u < NAU; ++u) {
    const double den = 2.0 * a[u] + a[NAU + u] + a[2 * NAU + u];
    au_f1 += den > 0.0 ? 2.0 * a[u] / den : 0.0;
    correct += a[3 * NAU + u];
    labelled += a[4 * NAU + u];
  }
  au_f1 /= (double)NAU;
  const double au_acc = labelled > 0.0 ? correct / labelled : nan;
  // VA
  double ccc[2];
  for (int j = 0; j < 2; ++j) {
    const double* v = s + AVF_EVAL_VA_MOMENTS + 6 * j;
    const double n = v[0];
    ccc[j] = 0.0;
    if (n > 1.0) {
      const double mx = v[1] / n, my = v[2] / n;
      const double var_x = v[3] / n - mx * mx, var_y = v[4] / n - my * my, cov = v[5] / n - mx * my, dm = mx - my;
      ccc[j] = 2.0 * cov / (var_x + var_y + dm * dm + 1e-8);
    }
  }
  scores[0] = ex_acc;
  scores[1] = ex_f1;
  scores[2] = 0.67 * ex_f1 + 0.33 * ex_acc;
  scores[3] = au_acc;
  scores[4] = au_f1;
  scores[5] = 0.5 * au_f1 + 0.5 * au_acc;
  scores[6] = ccc[0];
  scores[7] = ccc[1];
  scores[8] = (ccc[0] + ccc[1]) / 2.0;
  scores[9] = s[AVF_EVAL_LOSS_STEPS] > 0.0 ? s[AVF_EVAL_LOSS_SUM] / s[AVF_EVAL_LOSS_STEPS] : nan;
  scores[10] = kept;
  scores[11] = labelled;
}

}  // namespace
}  // namespace avf

extern "C" size_t avf_sizeof_eval_cfg(void) { return sizeof(avf_eval_cfg); }

extern "C" int avf_eval_update(const float* out, int64_t ld_out, const int64_t* y_ex, const float* y_au, int64_t ld_au,
                               const float* y_va, int64_t ld_va, const float* loss, const avf_eval_cfg* cfg, int rows,
                               double* state, uint8_t* pred_au, int64_t* pred_ex, float* pred_va, void* stream) {
  using namespace avf;
  AVF_REQUIRE(out && cfg && rows > 0, "eval_update: bad arguments");
  AVF_REQUIRE(state || pred_au || pred_ex || pred_va, "eval_update: neither a state nor a prediction buffer");
  AVF_REQUIRE(cfg->ex_col >= 0 && cfg->ex_col + NEX <= ld_out && cfg->au_col >= 0 && cfg->au_col + NAU <= ld_out &&
              cfg->va_col >= 0 && cfg->va_col + 2 <= ld_out, "eval_update: a column block lies outside the %lld-float row",
              (long long)ld_out);
  AVF_REQUIRE((!y_au || ld_au >= NAU) && (!y_va || ld_va >= 2), "eval_update: label stride too small");
  eval_update_kernel<<<1, EM_THREADS, 0, (hipStream_t)stream>>>(out, ld_out, y_ex, y_au, ld_au, y_va, ld_va, loss, *cfg, rows,
                                                                state, pred_au, pred_ex, pred_va);
  return check_launch("eval_update_kernel");
}

extern "C" int avf_eval_scores(const double* state, const avf_eval_cfg* cfg, double* scores, void* stream) {
  using namespace avf;
  AVF_REQUIRE(state && cfg && scores, "eval_scores: bad arguments");
  eval_scores_kernel<<<1, AVF_EVAL_STATE_WORDS, 0, (hipStream_t)stream>>>(state, scores);
  return check_launch("eval_scores_kernel");
}
