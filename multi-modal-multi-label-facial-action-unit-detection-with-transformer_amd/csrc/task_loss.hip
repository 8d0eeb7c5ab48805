// task_loss.hip - the three task losses of the reference's multi-task step (train.py:146,229: get_mt_loss) on the model's
// [rows, 21] output row in ONE single-workgroup launch: expression (columns 12..18), action units (0..11), valence /
// arousal (19..20).  The column blocks are disjoint, so one kernel writes the three values and one [rows, width] gradient
// whose block k is d losses[k] / d out; a second, elementwise kernel scales the blocks by the three incoming gradients.
//
//   EX  cross-entropy:  sum_valid w[t] (lse(z) - z[t]) / sum_valid w[t]                      (nn.CrossEntropyLoss)
//       focal:          p = softmax(z)[t'] + smooth, t' = valid ? t : 0 (ignored rows gather class 0 and are masked);
//                       sum valid * (-alpha[t'] (1-p)^gamma log p) / (rows * valid rows)     (loss.py:448-463)
//   AU  rows whose FIRST label equals `ignore` are dropped (loss.py:85-88, 170-173);
//       BCE:            mean over kept rows x 12 of the pos-weighted BCE-with-logits          (AULoss, as au_loss_kernel)
//       Dice + 5 BCE:   sum_c [1 - (2 sum p y + 1) / (sum p + sum y + 1)] + 5 x that mean     (DiceAULoss; the Dice term unweighted)
//   VA  per column, on x = tanh(out) and the rows whose label differs from `ignore`, n of them:
//       1 - 2 sum (x-mx)(y-my) / ((var_x + var_y + (mx-my)^2 + 1e-8) rows), unbiased variances, `rows` counted BEFORE the
//       drop; n <= 1 gives 0 with a zero gradient                                             (CCCLoss, loss.py:284-311)
//
// The batch-wide sums are workgroup reductions (DPP wave sums, then four partials through LDS); rows are walked in a strided
// loop.  The CCC moments are taken mean first, then centred sums.  No host synchronisation: the launch can be captured.
#include "common.hpp"

namespace avf {
namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_WAVES = TL_THREADS / 64;
constexpr int NEX = AVF_TASK_LOSS_EX_CLASSES;  // 7
constexpr int NAU = AVF_TASK_LOSS_AU_UNITS;    // 12

// sums v[0..K) over the workgroup; every thread returns with the totals.  `lds` holds TL_WAVES * K floats.
template <int K>
__device__ __forceinline__ void block_sum(float (&v)[K], float* lds) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float s = wave_sum(v[k]);
    if (lane == 0) lds[wave * K + k] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (lds[k] + lds[K + k]) + (lds[2 * K + k] + lds[3 * K + k]);
  __syncthreads();  // lds is reused by the next reduction
}

struct ExRow {
  float lse;
  int t;       // gathered class (0 for a masked row)
  bool valid;
};

// a label outside 0..6 that is not the ignore index has no logit to gather: the row is masked like an ignored one
__device__ __forceinline__ ExRow ex_row(const float* __restrict__ z, int64_t label, const avf_task_loss_cfg& c) {
  ExRow r;
  r.valid = !(c.ex_use_ignore && label == c.ex_ignore) && label >= 0 && label < NEX;
  r.t = r.valid ? (int)label : 0;
  float m = z[0];
#pragma unroll
  for (int j = 1; j < NEX; ++j) m = fmaxf(m, z[j]);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NEX; ++j) s += expf(z[j] - m);
  r.lse = m + logf(s);
  return r;
}

__device__ __forceinline__ float pow_gamma(float x, float g) { return g == 2.0f ? x * x : (g == 1.0f ? x : (g == 0.0f ? 1.0f : powf(x, g))); }

// softplus(-z) = max(-z, 0) + log1p(exp(-|z|))
__device__ __forceinline__ float bce_elem(float z, float y, float w) {
  const float sp = fmaxf(-z, 0.f) + log1pf(expf(-fabsf(z)));
  return (1.f - y) * z + (1.f + (w - 1.f) * y) * sp;
}

constexpr int K1 = 3 + 3 + 3 * NAU + 6;  // EX (sum, valid, weight) + AU (bce, kept, labels) + Dice (I, P, T per unit) + VA (n, sx, sy) x 2
constexpr int VA0 = 6 + 3 * NAU;             // first VA slot of pass 1
constexpr int K2 = 6;                    // VA centred sums (sxx, syy, sxy) x 2

__global__ __launch_bounds__(TL_THREADS) void task_loss_kernel(const float* __restrict__ out, int64_t ldo,
                                                               const int64_t* __restrict__ y_ex,
                                                               const float* __restrict__ y_au, int64_t ld_au,
                                                               const float* __restrict__ y_va, int64_t ld_va,
                                                               const avf_task_loss_cfg c, int rows, int width,
                                                               float* __restrict__ losses, float* __restrict__ counts,
                                                               float* __restrict__ grad) {
  __shared__ float lds[TL_WAVES * K1];
  __shared__ float tot[3 * NAU];  // the Dice sums, indexed by the column in the gradient loop
  const bool dice = c.au_mode == AVF_AU_DICE_BCE, focal = c.ex_mode == AVF_EX_FOCAL;
  const int nva = y_va ? c.va_ncols : 0;

  // ---- pass 1: plain sums, one row per thread and step ----
  float a[K1];
#pragma unroll
  for (int k = 0; k < K1; ++k) a[k] = 0.f;
  for (int r = threadIdx.x; r < rows; r += TL_THREADS) {
    const float* o = out + (int64_t)r * ldo;
    if (y_ex) {
      const float* z = o + c.ex_col;
      const ExRow e = ex_row(z, y_ex[r], c);
      if (focal) {
        const float p = expf(z[e.t] - e.lse) + c.smooth;
        const float l = -c.ex_weight[e.t] * pow_gamma(1.0f - p, c.gamma) * logf(p);
        a[0] += e.valid ? l : 0.f;
      } else if (e.valid) {
        a[0] += c.ex_weight[e.t] * (e.lse - z[e.t]);
        a[2] += c.ex_weight[e.t];
      }
      a[1] += e.valid ? 1.f : 0.f;
    }
    if (y_au) {
      const float* z = o + c.au_col;
      const float* y = y_au + (int64_t)r * ld_au;
      const bool keep = y[0] != c.au_ignore;
      a[4] += keep ? 1.f : 0.f;
#pragma unroll
      for (int u = 0; u < NAU; ++u) {
        const float yy = y[u];
        a[5] += yy != c.au_ignore ? 1.f : 0.f;
        if (keep) {
          const float zz = z[u];
          a[3] += bce_elem(zz, yy, c.pos_weight[u]);
          if (dice) {
            const float p = 1.0f / (1.0f + expf(-zz));
            a[6 + u] += p * yy;
            a[6 + NAU + u] += p;
            a[6 + 2 * NAU + u] += yy;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j < nva) {
        const float yy = y_va[(int64_t)r * ld_va + j];
        if (yy != c.va_ignore) {
          const float x = c.va_tanh ? tanhf(o[c.va_col + j]) : o[c.va_col + j];
          a[VA0 + 3 * j] += 1.f;
          a[VA0 + 3 * j + 1] += x;
          a[VA0 + 3 * j + 2] += yy;
        }
      }
    }
  }
  block_sum<K1>(a, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3 * NAU; ++k) tot[k] = a[6 + k];
  }  // (published by the barriers of the next reduction)
  const float n_j[2] = {a[VA0], a[VA0 + 3]};

  // ---- pass 2: the CCC moments, centred on the means of pass 1 ----
  const float mx[2] = {a[VA0 + 1] / n_j[0], a[VA0 + 4] / n_j[1]}, my[2] = {a[VA0 + 2] / n_j[0], a[VA0 + 5] / n_j[1]};
  float m2[K2] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = threadIdx.x; r < rows && nva > 0; r += TL_THREADS) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j < nva) {
        const float yy = y_va[(int64_t)r * ld_va + j];
        if (yy != c.va_ignore) {
          const float ov = out[(int64_t)r * ldo + c.va_col + j];
          const float dx = (c.va_tanh ? tanhf(ov) : ov) - mx[j], dy = yy - my[j];
          m2[3 * j] += dx * dx;
          m2[3 * j + 1] += dy * dy;
          m2[3 * j + 2] += dx * dy;
        }
      }
    }
  }
  block_sum<K2>(m2, lds);

  // ---- the three values and their scales ----
  const float frows = (float)rows;
  const float n_ex = y_ex ? (c.ex_use_ignore ? a[1] : frows) : 0.f, n_au = a[5], n_va = n_j[0] + n_j[1];
  // normalize (get_mt_loss(normalize=True), sformer.py:427-447): each value over its count of valid labels, 0 for a count of 0
  const float nrm_ex = c.normalize ? (n_ex > 0.f ? 1.0f / n_ex : 0.f) : 1.0f;
  const float nrm_au = c.normalize ? (n_au > 0.f ? 1.0f / n_au : 0.f) : 1.0f;
  const float nrm_va = c.normalize ? (n_va > 0.f ? 1.0f / n_va : 0.f) : 1.0f;

  // EX: focal 'mean' is sum / (rows x valid rows) with an ignore index, sum / rows without (loss.py:460-463)
  const float ex_inv = focal ? 1.0f / (c.ex_use_ignore ? frows * a[1] : frows) : 1.0f / a[2];
  const float l_ex = a[0] * ex_inv;  // 0/0 -> NaN when every row is ignored (as the reference)
  // AU
  const float bce_inv = (dice ? 5.0f : 1.0f) / (a[4] * (float)NAU);
  float l_au = a[3] * bce_inv;       // 0/0 -> NaN when every row is dropped
  if (dice) {
    float d = 0.f;
#pragma unroll
    for (int u = 0; u < NAU; ++u) d += 1.0f - (2.0f * a[6 + u] + 1.0f) / (a[6 + NAU + u] + a[6 + 2 * NAU + u] + 1.0f);
    l_au += d;
  }
  // VA
  float l_va = 0.f, den[2] = {1.f, 1.f};
  bool live[2] = {false, false};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    live[j] = j < nva && n_j[j] > 1.f;  // at most one row left: 0, no gradient (loss.py:293-295)
    if (live[j]) {
      const float dm = mx[j] - my[j];
      den[j] = m2[3 * j] / (n_j[j] - 1.f) + m2[3 * j + 1] / (n_j[j] - 1.f) + dm * dm + 1e-8f;
      l_va += c.va_weight[j] * (1.0f - 2.0f * m2[3 * j + 2] / (den[j] * frows));
    }
  }
  if (threadIdx.x == 0) {
    losses[0] = y_ex ? (c.normalize && n_ex <= 0.f ? 0.f : l_ex * nrm_ex) : 0.f;
    losses[1] = y_au ? (c.normalize && n_au <= 0.f ? 0.f : l_au * nrm_au) : 0.f;
    losses[2] = y_va ? l_va * nrm_va : 0.f;
    counts[0] = n_ex;
    counts[1] = n_au;
    counts[2] = n_va;
  }

  // ---- the gradient, one element per thread and step; every element of [rows, width] is written ----
  const int total = rows * width;
  for (int i = threadIdx.x; i < total; i += TL_THREADS) {
    const int r = i / width, col = i - r * width;
    const float* o = out + (int64_t)r * ldo;
    float g = 0.f;
    if (y_ex && col >= c.ex_col && col < c.ex_col + NEX) {
      if (!(c.normalize && n_ex <= 0.f)) {
        const float* z = o + c.ex_col;
        const int j = col - c.ex_col;
        const ExRow e = ex_row(z, y_ex[r], c);
        const float sj = expf(z[j] - e.lse), hot = j == e.t ? 1.f : 0.f;
        if (focal) {
          const float st = expf(z[e.t] - e.lse), p = st + c.smooth, om = 1.0f - p;
          // d/dp of -alpha (1-p)^gamma log p
          const float dldp = -c.ex_weight[e.t] * (pow_gamma(om, c.gamma) / p - c.gamma * pow_gamma(om, c.gamma - 1.0f) * logf(p));
          // the mask multiplies BEFORE the scale: with no valid row the scale is 1/0 and the gradient NaN, as autograd's is
          g = (e.valid ? 1.f : 0.f) * (dldp * st * (hot - sj)) * ex_inv * nrm_ex;
        } else if (e.valid) {
          g = c.ex_weight[e.t] * (sj - hot) * ex_inv * nrm_ex;
        }
      }
    } else if (y_au && col >= c.au_col && col < c.au_col + NAU) {
      const float* y = y_au + (int64_t)r * ld_au;
      if (y[0] != c.au_ignore) {
        const int u = col - c.au_col;
        const float zz = o[col], yy = y[u], w = c.pos_weight[u];
        const float sg = 1.0f / (1.0f + expf(-zz));
        g = (sg * (1.f - yy + w * yy) - w * yy) * bce_inv;
        if (dice) {
          const float s = tot[NAU + u] + tot[2 * NAU + u] + 1.0f;
          g -= (2.0f * yy * s - (2.0f * tot[u] + 1.0f)) / (s * s) * sg * (1.0f - sg);
        }
        g *= nrm_au;
      }
    } else if (col >= c.va_col && col < c.va_col + nva) {
      const bool second = col != c.va_col;
      const float yy = y_va[(int64_t)r * ld_va + (second ? 1 : 0)];
      if ((second ? live[1] : live[0]) && yy != c.va_ignore) {
        const float n = second ? n_j[1] : n_j[0], mxj = second ? mx[1] : mx[0], myj = second ? my[1] : my[0];
        const float dj = second ? den[1] : den[0], sxy = second ? m2[5] : m2[2], wj = second ? c.va_weight[1] : c.va_weight[0];
        const float x = c.va_tanh ? tanhf(o[col]) : o[col];
        const float dden = 2.0f * (x - mxj) / (n - 1.f) + 2.0f * (mxj - myj) / n;
        g = -2.0f / frows * ((yy - myj) / dj - sxy * dden / (dj * dj));
        g *= wj * nrm_va * (c.va_tanh ? 1.0f - x * x : 1.0f);
      }
    }
    grad[i] = g;
  }
}

// dout[r, col] = grad_wide[r, col] * g[block of col]; a null g, and every column outside the three blocks, gives 0
__global__ __launch_bounds__(TL_THREADS) void task_loss_bwd_kernel(const float* __restrict__ grad_wide,
                                                                   const float* __restrict__ g_ex,
                                                                   const float* __restrict__ g_au,
                                                                   const float* __restrict__ g_va, int ex_col, int au_col,
                                                                   int va_col, int va_ncols, int64_t total, int width,
                                                                   float* __restrict__ dout) {
  const float ge = g_ex ? g_ex[0] : 0.f, ga = g_au ? g_au[0] : 0.f, gv = g_va ? g_va[0] : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * TL_THREADS) {
    const int col = (int)(i % width);
    float v = 0.f;
    if (g_ex && col >= ex_col && col < ex_col + NEX) v = grad_wide[i] * ge;
    else if (g_au && col >= au_col && col < au_col + NAU) v = grad_wide[i] * ga;
    else if (g_va && col >= va_col && col < va_col + va_ncols) v = grad_wide[i] * gv;
    dout[i] = v;
  }
}

bool blocks_ok(const avf_task_loss_cfg& c, bool ex, bool au, bool va, int width) {
  if (ex && (c.ex_col < 0 || c.ex_col + NEX > width)) return false;
  if (au && (c.au_col < 0 || c.au_col + NAU > width)) return false;
  if (va && (c.va_col < 0 || c.va_col + c.va_ncols > width)) return false;
  // the blocks that are live must not overlap
  const int lo[3] = {c.ex_col, c.au_col, c.va_col}, n[3] = {NEX, NAU, c.va_ncols};
  const bool on[3] = {ex, au, va};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (on[i] && on[j] && lo[i] < lo[j] + n[j] && lo[j] < lo[i] + n[i]) return false;
  return true;
}

}  // namespace
}  // namespace avf

extern "C" size_t avf_sizeof_task_loss_cfg(void) { return sizeof(avf_task_loss_cfg); }

extern "C" int avf_task_loss(const float* out, int64_t ld_out, const int64_t* y_ex, const float* y_au, int64_t ld_au,
                             const float* y_va, int64_t ld_va, const avf_task_loss_cfg* cfg, int rows, int width,
                             float* losses, float* counts, float* grad_wide, void* stream) {
  using namespace avf;
  AVF_REQUIRE(out && cfg && losses && counts && grad_wide && rows > 0 && width > 0 && ld_out >= width,
              "task_loss: bad arguments");
  AVF_REQUIRE((int64_t)rows * width <= INT32_MAX, "task_loss: rows * width exceeds the 32-bit element index");
  AVF_REQUIRE(cfg->va_ncols == 1 || cfg->va_ncols == 2, "task_loss: va_ncols must be 1 or 2");
  AVF_REQUIRE((cfg->ex_mode == AVF_EX_CROSS_ENTROPY || cfg->ex_mode == AVF_EX_FOCAL) &&
              (cfg->au_mode == AVF_AU_BCE || cfg->au_mode == AVF_AU_DICE_BCE), "task_loss: unknown ex_mode / au_mode");
  AVF_REQUIRE(blocks_ok(*cfg, y_ex != nullptr, y_au != nullptr, y_va != nullptr, width),
              "task_loss: a column block lies outside the %d-wide row or overlaps another", width);
  AVF_REQUIRE((!y_au || ld_au >= AVF_TASK_LOSS_AU_UNITS) && (!y_va || ld_va >= cfg->va_ncols), "task_loss: label stride too small");
  task_loss_kernel<<<1, TL_THREADS, 0, (hipStream_t)stream>>>(out, ld_out, y_ex, y_au, ld_au, y_va, ld_va, *cfg, rows, width,
                                                              losses, counts, grad_wide);
  return check_launch("task_loss_kernel");
}

extern "C" int avf_task_loss_bwd(const float* grad_wide, const float* g_ex, const float* g_au, const float* g_va,
                                 const avf_task_loss_cfg* cfg, int rows, int width, float* dout, void* stream) {
  using namespace avf;
  AVF_REQUIRE(grad_wide && cfg && dout && rows > 0 && width > 0, "task_loss_bwd: bad arguments");
  AVF_REQUIRE(blocks_ok(*cfg, g_ex != nullptr, g_au != nullptr, g_va != nullptr, width),
              "task_loss_bwd: a column block lies outside the %d-wide row or overlaps another", width);
  const int64_t total = (int64_t)rows * width;
  const int64_t blocks = (total + TL_THREADS - 1) / TL_THREADS;
  task_loss_bwd_kernel<<<(unsigned)(blocks < 256 ? blocks : 256), TL_THREADS, 0, (hipStream_t)stream>>>(
      grad_wide, g_ex, g_au, g_va, cfg->ex_col, cfg->au_col, cfg->va_col, cfg->va_ncols, total, width, dout);
  return check_launch("task_loss_bwd_kernel");
}
