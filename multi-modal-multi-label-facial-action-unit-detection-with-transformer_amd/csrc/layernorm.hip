// layernorm.hip - LayerNorm forward / backward, HBM-bound (wavefront reductions): the six ln_* kernel templates, one typed
// launcher per template, and the host entry points layernorm_fwd / layernorm_bwd / layernorm_bwd_ws (common.hpp).
//
// Reference math: models/heads.py:178-185 (PreNorm/nn.LayerNorm).
#include <algorithm>
#include <type_traits>

#include "common.hpp"

namespace avf {

// The runtime -> compile-time step of the row width, written once for each column layout.  f is a generic lambda; the
// instantiations of a kernel template are exactly the calls the dispatch below makes through these two.
template <typename F>
static int ln_nv(int dim, F&& f) {  // NV: float4 chunks per lane (one per 256 columns), dim <= 1536
  switch ((dim + 255) / 256) {
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    case 3: return f(int_c<3>{});
    case 4: return f(int_c<4>{});
    default: return f(int_c<6>{});
  }
}
template <typename F>
static int ln_nv8(int dim, F&& f) {  // NV8: 8-column chunks per lane (one per 512 columns); RU: rows in flight per wave in the
  switch ((dim + 511) / 512) {       // backward - what the register file allows at two waves per SIMD or more
    case 1: return f(int_c<1>{}, int_c<4>{});
    case 2: return f(int_c<2>{}, int_c<2>{});
    default: return f(int_c<3>{}, int_c<1>{});
  }
}

// =============================================================================================
// LayerNorm forward: one wavefront per row; fp32 statistics; output fp32 or bf16.
// Algorithmic bytes per row: 4*D read + sizeof(out)*D written + 8 (mean, rstd).
// =============================================================================================
template <typename OutT>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, OutT* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     int64_t rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * D;
  OutT* yr = y + row * D;
  float s = 0.f;
  if ((D & 3) == 0) {
    for (int c = lane * 4; c < D; c += 256) {
      float4 v = *reinterpret_cast<const float4*>(xr + c);
      s += (v.x + v.y) + (v.z + v.w);
    }
  } else {
    for (int c = lane; c < D; c += 64) s += xr[c];
  }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
  if ((D & 3) == 0) {
    for (int c = lane * 4; c < D; c += 256) {
      float4 v = *reinterpret_cast<const float4*>(xr + c);
      float a = v.x - mu, b = v.y - mu, cc = v.z - mu, d = v.w - mu;
      q += (a * a + b * b) + (cc * cc + d * d);
    }
  } else {
    for (int c = lane; c < D; c += 64) {
      float a = xr[c] - mu;
      q += a * a;
    }
  }
  const float var = wave_sum(q) / (float)D;
  const float rs = 1.0f / sqrtf(var + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
  if ((D & 3) == 0) {
    for (int c = lane * 4; c < D; c += 256) {
      float4 v = *reinterpret_cast<const float4*>(xr + c);
      float4 g = *reinterpret_cast<const float4*>(gamma + c);
      float4 b = *reinterpret_cast<const float4*>(beta + c);
      float4 o;
      o.x = (v.x - mu) * rs * g.x + b.x;
      o.y = (v.y - mu) * rs * g.y + b.y;
      o.z = (v.z - mu) * rs * g.z + b.z;
      o.w = (v.w - mu) * rs * g.w + b.w;
      store4<OutT>(yr + c, o);
    }
  } else {
    for (int c = lane; c < D; c += 64) yr[c] = from_f32<OutT>((xr[c] - mu) * rs * gamma[c] + beta[c]);
  }
}

// D % 4 == 0 and D <= 256*NV: the row lives in registers (one HBM read, no re-reads from cache)
// MX: also emit the MX-FP8 image of the row (common.hpp mx8_encode4: D % 32 == 0, so the 8 lanes of a block are
// live together) - the A operand of the following forward GEMM in the fp8 mode (layer.hip)
template <typename OutT, int NV, bool MX = false, typename InT = float>
__global__ __launch_bounds__(256) void ln_fwd_reg_kernel(const InT* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, OutT* __restrict__ y,
                                                         float* __restrict__ mean, float* __restrict__ rstd,
                                                         int64_t rows, int D, float eps, uint8_t* __restrict__ yq = nullptr,
                                                         uint8_t* __restrict__ ys = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane * 4 + 256 * i;
    v[i] = c < D ? load4<InT>(x + row * D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane * 4 + 256 * i;
    if (c < D) {
      const float a = v[i].x - mu, b = v[i].y - mu, cc = v[i].z - mu, d = v[i].w - mu;
      q += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float rs = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane * 4 + 256 * i;
    if (c < D) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + c);
      const float4 b = *reinterpret_cast<const float4*>(beta + c);
      const float4 o = make_float4((v[i].x - mu) * rs * g.x + b.x, (v[i].y - mu) * rs * g.y + b.y,
                                   (v[i].z - mu) * rs * g.z + b.z, (v[i].w - mu) * rs * g.w + b.w);
      store4<OutT>(y + row * D + c, o);
      if (MX) {
        const float ov[4] = {o.x, o.y, o.z, o.w};
        uint32_t sb;
        const uint32_t qw = mx8_encode4(ov, &sb);
        *reinterpret_cast<uint32_t*>(yq + row * D + c) = qw;
        if ((lane & 7) == 0) ys[row * (D >> 5) + (c >> 5)] = (uint8_t)sb;
      }
    }
  }
}

static int ln_row8_on() {
  static const int on = tuning_int("AVF_LN_ROW8", 1);  // tuning / A-B aid: 0 = the one-row-per-wave kernels
  return on;
}

// ---- the bf16 residual stream's kernels (bf16 in, bf16 out, D % 8 == 0, D <= 512 * NV8) -----------------------------
// A lane owns 8 consecutive columns per 512 (one 16-byte access); a wave works on RU rows at once with all their loads in
// flight before the first reduction: 4 x 4 rows per workgroup, ~10 waves per CU x RU KiB per stream in flight (the
// one-row-per-wave form had 1 KiB per wave and ran at 2.5 TB/s; DESIGN_HISTORY.md section 14).
// MX: also the MX-FP8 image of the rows (D % 32 == 0: a 32-block is the 8 columns of the four lanes of a quad)
// Src: where a row comes from.  LnRowBf16: the bf16 residual stream.  LnRowEmbed (the bottom layer of a fused stack): row b * T + t
// is bf16(clip[b, t] or audio[b, t - Tv], + pos[t]) - fuse_tokens_kernel<bf16>'s values and rounding (one fp32 add, pack8) - and is
// also stored as x0, the stream the rest of the layer reads; the statistics are those of the rounded values, so x0, y, mean and
// rstd are the bits the two launches gave (one pass over the fp32 inputs instead of a bf16 round trip through memory).
struct LnRowBf16 {
  static constexpr bool kStoresRow = false;
  const bf16* __restrict__ x;
  struct Row { const bf16* p; };
  __device__ __forceinline__ Row row(int64_t r, int D) const { return Row{x + r * D}; }
  __device__ __forceinline__ uint4 load(const Row& r, int c) const { return *reinterpret_cast<const uint4*>(r.p + c); }
  __device__ __forceinline__ void store_row(int64_t, int, int, uint4) const {}
};
struct LnRowEmbed {
  static constexpr bool kStoresRow = true;
  const float* __restrict__ clip;
  const float* __restrict__ audio;
  const float* __restrict__ pos;
  bf16* __restrict__ x0;
  int Tv, Ta;
  struct Row { const float *p, *e; };
  __device__ __forceinline__ Row row(int64_t r, int D) const {
    const int T = Tv + Ta;
    const int64_t b = r / T;
    const int t = (int)(r - b * T);
    return Row{t < Tv ? clip + (b * Tv + t) * D : audio + (b * Ta + (t - Tv)) * D, pos + (int64_t)t * D};
  }
  __device__ __forceinline__ uint4 load(const Row& r, int c) const {
    float4 v0 = *reinterpret_cast<const float4*>(r.p + c), v1 = *reinterpret_cast<const float4*>(r.p + c + 4);
    const float4 p0 = *reinterpret_cast<const float4*>(r.e + c), p1 = *reinterpret_cast<const float4*>(r.e + c + 4);
    v0.x += p0.x; v0.y += p0.y; v0.z += p0.z; v0.w += p0.w;
    v1.x += p1.x; v1.y += p1.y; v1.z += p1.z; v1.w += p1.w;
    const float o[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    return pack8(o);
  }
  __device__ __forceinline__ void store_row(int64_t r, int D, int c, uint4 v) const { store_out16(x0 + r * D + c, v); }
};
template <int NV8, int RU, bool MX = false, typename Src = LnRowBf16>
__global__ __launch_bounds__(256) void ln_fwd_row8_kernel(const Src src, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, bf16* __restrict__ y,
                                                          float* __restrict__ mean, float* __restrict__ rstd, int64_t rows,
                                                          int D, float eps, uint8_t* __restrict__ yq = nullptr,
                                                          uint8_t* __restrict__ ys = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RU;
  if (row0 >= rows) return;
  uint4 raw[RU][NV8];
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    const int64_t row = row0 + r < rows ? row0 + r : rows - 1;  // (rows past the end re-read the last one; nothing is stored)
    const typename Src::Row sr = src.row(row, D);
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      const int c = lane * 8 + 512 * i;
      raw[r][i] = c < D ? src.load(sr, c) : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  float gm[NV8][8], bt[NV8][8];
#pragma unroll
  for (int i = 0; i < NV8; ++i) {
    const int c = lane * 8 + 512 * i;
    if (c < D) {
      load8f(gamma + c, gm[i]);
      load8f(beta + c, bt[i]);
    }
  }
  const float invD = 1.0f / (float)D;
  float mu[RU], rs[RU];
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      float v[8];
      unpack8(raw[r][i], v);
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    mu[r] = wave_sum(s) * invD;
  }
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      if (lane * 8 + 512 * i < D) {
        float v[8];
        unpack8(raw[r][i], v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float a = v[k] - mu[r];
          q = fmaf(a, a, q);
        }
      }
    }
    rs[r] = 1.0f / sqrtf(wave_sum(q) * invD + eps);
  }
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    if (row0 + r >= rows) break;
    if (lane == 0) {
      store_out4(mean + row0 + r, mu[r]);
      store_out4(rstd + row0 + r, rs[r]);
    }
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      const int c = lane * 8 + 512 * i;
      if (c < D) {
        float v[8], o[8];
        unpack8(raw[r][i], v);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (v[k] - mu[r]) * rs[r] * gm[i][k] + bt[i][k];
        store_out16(y + (row0 + r) * D + c, pack8(o));
        if constexpr (Src::kStoresRow) src.store_row(row0 + r, D, c, raw[r][i]);
        if constexpr (MX) {  // (c < D is uniform over a quad: D % 32 == 0)
          const MxBlock mb = mx8_encode(o);
          *reinterpret_cast<uint2*>(yq + (row0 + r) * D + c) = mb.q;
          if ((lane & 3) == 0) ys[(row0 + r) * (D >> 5) + (c >> 5)] = (uint8_t)mb.scale;
        }
      }
    }
  }
}

// ---- launchers: one per kernel template (grid, launch inside the timing scope, launch check) ----
template <typename OutT>
static int launch_ln_fwd(const TimingScope* ts, hipStream_t s, const float* x, const float* gamma, const float* beta, OutT* y,
                         float* mean, float* rstd, int64_t rows, int D, float eps) {
  launch_in_scope(ts, ln_fwd_kernel<OutT>, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, gamma, beta, y, mean, rstd, rows,
                  D, eps);
  return check_launch("ln_fwd_kernel");
}

template <int NV, bool MX, typename InT, typename OutT>
static int launch_ln_fwd_reg(const TimingScope* ts, hipStream_t s, const InT* x, const float* gamma, const float* beta, OutT* y,
                             float* mean, float* rstd, int64_t rows, int D, float eps, uint8_t* yq, uint8_t* ys) {
  launch_in_scope(ts, ln_fwd_reg_kernel<OutT, NV, MX, InT>, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, gamma, beta, y,
                  mean, rstd, rows, D, eps, yq, ys);
  return check_launch(sizeof(InT) == 2 ? "ln_fwd_reg_kernel(bf16 in)" : MX ? "ln_fwd_reg_kernel(mx)" : "ln_fwd_kernel");
}

template <int NV8, bool MX, typename Src>
static int launch_ln_fwd_row8(const TimingScope* ts, hipStream_t s, const Src& src, const float* gamma, const float* beta, bf16* y,
                              float* mean, float* rstd, int64_t rows, int D, float eps, uint8_t* yq, uint8_t* ys) {
  // four rows per wave, 16-byte accesses; two where the rows are built from the fp32 inputs (twice the bytes in flight per row:
  // C2's embed launch 13.5 us at two rows, 17.1 at four - the two launches it stands for took 10.4 + 7.7)
  constexpr int RU = Src::kStoresRow ? 2 : 4;
  launch_in_scope(ts, ln_fwd_row8_kernel<NV8, RU, MX, Src>, dim3((unsigned)ceil_div(rows, 4 * RU)), dim3(256), 0, s, src, gamma, beta,
                  y, mean, rstd, rows, D, eps, yq, ys);
  return check_launch(Src::kStoresRow ? "ln_fwd_row8_kernel(embed)" : "ln_fwd_row8_kernel");
}

int layernorm_fwd(const void* xv, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                  float* rstd, int64_t rows, int dim, float eps, hipStream_t s, void* mx_q, void* mx_s, int x_dtype) {
  AVF_REQUIRE(rows > 0 && dim > 0, "layernorm_fwd: bad shape rows=%lld dim=%d", (long long)rows, dim);
  AVF_REQUIRE(y_dtype == AVF_F32 || y_dtype == AVF_BF16, "layernorm_fwd: bad dtype %d", y_dtype);
  AVF_REQUIRE(x_dtype == AVF_F32 || (x_dtype == AVF_BF16 && y_dtype == AVF_BF16 && dim % 4 == 0 && dim <= 1536),
              "layernorm_fwd: a bf16 input needs a bf16 output, dim %% 4 == 0 and dim <= 1536 (dim=%d)", dim);
  const float* x = (const float*)xv;
  const bf16* xb = (const bf16*)xv;
  uint8_t *yq = (uint8_t*)mx_q, *ys = mx_q ? (uint8_t*)mx_s : nullptr;  // the MX-FP8 image: both or neither
  TimingScope ts(KC_LAYERNORM, 0.0, (double)rows * dim * ((x_dtype == AVF_BF16 ? 2.0 : 4.0) + (y_dtype == AVF_BF16 ? 2.0 : 4.0) +
                                                         (mx_q ? 1.03125 : 0.0)), s, /*per_kernel=*/true);
  // the register kernel: storage types from the pointers, MX (std::true_type / std::false_type) and NV at compile time
  auto reg = [&](auto mx, auto* xp, auto* yp) {
    return ln_nv(dim, [&](auto nv) {
      return launch_ln_fwd_reg<decltype(nv)::value, decltype(mx)::value>(&ts, s, xp, gamma, beta, yp, mean, rstd, rows, dim, eps, yq, ys);
    });
  };
  if (x_dtype == AVF_BF16 && dim % 8 == 0 && (!mx_q || (mx_s && dim % 32 == 0)) && ln_row8_on()) {
    return ln_nv8(dim, [&](auto nv8, auto) {
      if (mx_q) return launch_ln_fwd_row8<decltype(nv8)::value, true>(&ts, s, LnRowBf16{xb}, gamma, beta, (bf16*)y, mean, rstd, rows, dim, eps, yq, ys);
      return launch_ln_fwd_row8<decltype(nv8)::value, false>(&ts, s, LnRowBf16{xb}, gamma, beta, (bf16*)y, mean, rstd, rows, dim, eps, yq, ys);
    });
  }
  if (x_dtype == AVF_BF16) {  // bf16 residual stream: bf16 in, bf16 out (+ optional MX-FP8 image)
    AVF_REQUIRE(!mx_q || (mx_s && dim % 32 == 0), "layernorm_fwd: the MX-FP8 image needs dim %% 32 == 0");
    return mx_q ? reg(std::true_type{}, xb, (bf16*)y) : reg(std::false_type{}, xb, (bf16*)y);
  }
  if (mx_q) {
    AVF_REQUIRE(mx_s && y_dtype == AVF_BF16 && dim % 32 == 0 && dim <= 1536,
                "layernorm_fwd: the MX-FP8 image needs bf16 output, dim %% 32 == 0 and dim <= 1536 (dim=%d)", dim);
    return reg(std::true_type{}, x, (bf16*)y);
  }
  if (dim % 4 == 0 && dim <= 1536) return y_dtype == AVF_F32 ? reg(std::false_type{}, x, (float*)y) : reg(std::false_type{}, x, (bf16*)y);
  if (y_dtype == AVF_F32) return launch_ln_fwd(&ts, s, x, gamma, beta, (float*)y, mean, rstd, rows, dim, eps);
  return launch_ln_fwd(&ts, s, x, gamma, beta, (bf16*)y, mean, rstd, rows, dim, eps);
}

bool layernorm_fwd_embed_ok(int dim) { return dim % 8 == 0 && dim <= 1536 && ln_row8_on(); }

// x0 = bf16(cat([clip, audio], 1) + pos) and y, mean, rstd = LayerNorm(x0) in one launch (LnRowEmbed)
int layernorm_fwd_embed(const float* clip, const float* audio, const float* pos, int batch, int t_video, int t_audio, void* x0,
                        const float* gamma, const float* beta, void* y, float* mean, float* rstd, int dim, float eps, hipStream_t s) {
  AVF_REQUIRE(batch > 0 && t_video > 0 && t_audio > 0 && clip && audio && pos && x0 && y && mean && rstd,
              "layernorm_fwd_embed: bad arguments (both token groups and the positional rows are needed)");
  AVF_REQUIRE(layernorm_fwd_embed_ok(dim), "layernorm_fwd_embed: needs dim %% 8 == 0, dim <= 1536 and the row8 kernels (dim=%d)", dim);
  AVF_REQUIRE((((uintptr_t)clip | (uintptr_t)audio | (uintptr_t)pos | (uintptr_t)x0 | (uintptr_t)y) & 15) == 0,
              "layernorm_fwd_embed: pointers must be 16-byte aligned");
  const int64_t rows = (int64_t)batch * (t_video + t_audio);
  TimingScope ts(KC_LAYERNORM, 0.0, (double)rows * dim * (4.0 + 2.0 + 2.0) + (double)(t_video + t_audio) * dim * 4.0, s, /*per_kernel=*/true);
  const LnRowEmbed src{clip, audio, pos, (bf16*)x0, t_video, t_audio};
  return ln_nv8(dim, [&](auto nv8, auto) {
    return launch_ln_fwd_row8<decltype(nv8)::value, false>(&ts, s, src, gamma, beta, (bf16*)y, mean, rstd, rows, dim, eps, nullptr, nullptr);
  });
}

// =============================================================================================
// LayerNorm backward.  One wavefront per row computes dx; the block accumulates the per-column sums
// (dgamma, dbeta, and the column sum of dx = bias gradient of the producing Linear) in LDS with
// ds_add_f32 and writes one partial per block; a second kernel folds the partials.
//   xhat = (x-mu)*rstd ; g = dy*gamma ; dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) + dres
// =============================================================================================
constexpr int LNB_ROWS_PER_BLOCK = 32;

template <typename DyT, bool VEC>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const DyT* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dres,
                                                     float* __restrict__ dx, bf16* __restrict__ dx_lo,
                                                     float* __restrict__ partial, int64_t rows, int D,
                                                     int want_colsum) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [3][D]
  float* s_dg = lds;
  float* s_db = lds + D;
  float* s_cs = lds + 2 * D;
  for (int i = threadIdx.x; i < 3 * D; i += 256) lds[i] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * LNB_ROWS_PER_BLOCK;
  const float invD = 1.0f / (float)D;
  for (int rr = wave; rr < LNB_ROWS_PER_BLOCK; rr += 4) {
    const int64_t row = row0 + rr;
    if (row >= rows) break;
    const float mu = mean[row], rs = rstd[row];
    const DyT* dyr = dy + row * D;
    const float* xr = x + row * D;
    float s1 = 0.f, s2 = 0.f;
    if (VEC) {
      for (int c = lane * 4; c < D; c += 256) {
        float4 d = load4<DyT>(dyr + c);
        float4 v = *reinterpret_cast<const float4*>(xr + c);
        float4 g = *reinterpret_cast<const float4*>(gamma + c);
        float g0 = d.x * g.x, g1 = d.y * g.y, g2 = d.z * g.z, g3 = d.w * g.w;
        s1 += (g0 + g1) + (g2 + g3);
        s2 += (g0 * (v.x - mu) + g1 * (v.y - mu)) + (g2 * (v.z - mu) + g3 * (v.w - mu));
      }
    } else {
      for (int c = lane; c < D; c += 64) {
        float g0 = to_f32<DyT>(dyr[c]) * gamma[c];
        s1 += g0;
        s2 += g0 * (xr[c] - mu);
      }
    }
    s1 = wave_sum(s1) * invD;
    s2 = wave_sum(s2) * rs * invD;  // mean(g * xhat)
    float* dxr = dx + row * D;
    if (VEC) {
      for (int c = lane * 4; c < D; c += 256) {
        float4 d = load4<DyT>(dyr + c);
        float4 v = *reinterpret_cast<const float4*>(xr + c);
        float4 g = *reinterpret_cast<const float4*>(gamma + c);
        float xh[4] = {(v.x - mu) * rs, (v.y - mu) * rs, (v.z - mu) * rs, (v.w - mu) * rs};
        float dd[4] = {d.x, d.y, d.z, d.w};
        float gg[4] = {g.x, g.y, g.z, g.w};
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (dres) {
          float4 t = *reinterpret_cast<const float4*>(dres + row * D + c);
          r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = rs * (dd[j] * gg[j] - s1 - xh[j] * s2) + r[j];
          atomicAdd(&s_dg[c + j], dd[j] * xh[j]);
          atomicAdd(&s_db[c + j], dd[j]);
          if (want_colsum) atomicAdd(&s_cs[c + j], o[j]);
        }
        *reinterpret_cast<float4*>(dxr + c) = make_float4(o[0], o[1], o[2], o[3]);
        if (dx_lo) store4<bf16>(dx_lo + row * D + c, make_float4(o[0], o[1], o[2], o[3]));
      }
    } else {
      for (int c = lane; c < D; c += 64) {
        float d = to_f32<DyT>(dyr[c]);
        float xh = (xr[c] - mu) * rs;
        float o = rs * (d * gamma[c] - s1 - xh * s2) + (dres ? dres[row * D + c] : 0.f);
        atomicAdd(&s_dg[c], d * xh);
        atomicAdd(&s_db[c], d);
        if (want_colsum) atomicAdd(&s_cs[c], o);
        dxr[c] = o;
        if (dx_lo) dx_lo[row * D + c] = from_f32<bf16>(o);
      }
    }
  }
  __syncthreads();
  float* out = partial + (int64_t)blockIdx.x * 3 * D;
  for (int i = threadIdx.x; i < 3 * D; i += 256) out[i] = lds[i];
}

// Fast path (D % 4 == 0, D <= 256*NV): every lane owns the same NV float4 column chunks for all the rows
// its wave processes, so the per-column sums (dgamma, dbeta, colsum(dx)) accumulate in registers; the
// four waves of a block are combined through LDS with plain adds (deterministic), one partial per block.
constexpr int LNR_ROWS_PER_BLOCK = 16;

// ResT: storage type of the incoming residual gradient dres (fp32, or bf16 when the gradient stream is kept in bf16:
// then dx is null and dx_lo is the stream the next LayerNorm backward reads as ITS dres)
template <typename DyT, int NV, typename ResT = float, typename XT = float>
__global__ __launch_bounds__(256) void ln_bwd_reg_kernel(const DyT* __restrict__ dy, const XT* __restrict__ x,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const ResT* __restrict__ dres, float* __restrict__ dx,
                                                         bf16* __restrict__ dx_lo, float* __restrict__ partial,
                                                         int64_t rows, int D, int want_colsum, DropCfg drop,
                                                         uint8_t* __restrict__ dxq = nullptr,
                                                         uint8_t* __restrict__ dxs = nullptr,
                                                         int rpb = LNR_ROWS_PER_BLOCK) {
  // rpb: rows per workgroup (16; 4 - one row per wave - for short inputs, where 16-row blocks leave most CUs empty and the
  //      four rows of a wave run one after the other)
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [4 waves][3][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * rpb;
  const float invD = 1.0f / (float)D;
  const uint64_t dkey = drop.thresh16 ? drop_key(drop) : 0;
  float4 g[NV], adg[NV], adb[NV], acs[NV];
  bool act[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane * 4 + 256 * i;
    act[i] = c < D;
    g[i] = act[i] ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    adg[i] = adb[i] = acs[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int rr = wave; rr < rpb; rr += 4) {
    const int64_t row = row0 + rr;
    if (row >= rows) break;
    const float mu = mean[row], rs = rstd[row];
    float4 d[NV], xh[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane * 4 + 256 * i;
      d[i] = xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (act[i]) {
        d[i] = load4<DyT>(dy + row * D + c);
        float4 v;
        if (sizeof(XT) == 4) {
          typedef float f32x4_nt __attribute__((ext_vector_type(4)));  // last use of this x row in the step: non-temporal
          const f32x4_nt xv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt*>(x + row * D + c));
          v = make_float4(xv[0], xv[1], xv[2], xv[3]);
        } else {
          typedef uint32_t u32x2_nt __attribute__((ext_vector_type(2)));
          const u32x2_nt xv = __builtin_nontemporal_load(reinterpret_cast<const u32x2_nt*>(x + row * D + c));
          v = make_float4(__uint_as_float(xv[0] << 16), __uint_as_float(xv[0] & 0xffff0000u), __uint_as_float(xv[1] << 16),
                          __uint_as_float(xv[1] & 0xffff0000u));
        }
        xh[i] = make_float4((v.x - mu) * rs, (v.y - mu) * rs, (v.z - mu) * rs, (v.w - mu) * rs);
      }
      const float g0 = d[i].x * g[i].x, g1 = d[i].y * g[i].y, g2 = d[i].z * g[i].z, g3 = d[i].w * g[i].w;
      s1 += (g0 + g1) + (g2 + g3);
      s2 += (g0 * xh[i].x + g1 * xh[i].y) + (g2 * xh[i].z + g3 * xh[i].w);
    }
    s1 = wave_sum(s1) * invD;
    s2 = wave_sum(s2) * invD;  // mean(g * xhat)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (!act[i]) continue;
      const int c = lane * 4 + 256 * i;
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (dres) r = load4<ResT>(dres + row * D + c);
      float4 o;
      o.x = rs * (d[i].x * g[i].x - s1 - xh[i].x * s2) + r.x;
      o.y = rs * (d[i].y * g[i].y - s1 - xh[i].y * s2) + r.y;
      o.z = rs * (d[i].z * g[i].z - s1 - xh[i].z * s2) + r.z;
      o.w = rs * (d[i].w * g[i].w - s1 - xh[i].w * s2) + r.w;
      if (dx) *reinterpret_cast<float4*>(dx + row * D + c) = o;
      if (drop.thresh16) {  // what the Linear behind the dropout site sees: masked, rescaled
        const float4 f = drop_factor4(drop, dkey, (uint64_t)row * D + c);
        o.x *= f.x; o.y *= f.y; o.z *= f.z; o.w *= f.w;
      }
      if (dx_lo) store4<bf16>(dx_lo + row * D + c, o);
      if (dxq) {  // wave-uniform: MX-FP8 image of the same values (D % 32 == 0: the 8 lanes of a block are live together)
        const float ov[4] = {o.x, o.y, o.z, o.w};
        uint32_t sb;
        const uint32_t qw = mx8_encode4(ov, &sb);
        *reinterpret_cast<uint32_t*>(dxq + row * D + c) = qw;
        if ((lane & 7) == 0) dxs[row * (D >> 5) + (c >> 5)] = (uint8_t)sb;
      }
      adg[i].x += d[i].x * xh[i].x; adg[i].y += d[i].y * xh[i].y; adg[i].z += d[i].z * xh[i].z; adg[i].w += d[i].w * xh[i].w;
      adb[i].x += d[i].x; adb[i].y += d[i].y; adb[i].z += d[i].z; adb[i].w += d[i].w;
      acs[i].x += o.x; acs[i].y += o.y; acs[i].z += o.z; acs[i].w += o.w;
    }
  }
  float* mine = lds + wave * 3 * D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!act[i]) continue;
    const int c = lane * 4 + 256 * i;
    *reinterpret_cast<float4*>(mine + c) = adg[i];
    *reinterpret_cast<float4*>(mine + D + c) = adb[i];
    *reinterpret_cast<float4*>(mine + 2 * D + c) = acs[i];
  }
  __syncthreads();
  float* out = partial + (int64_t)blockIdx.x * 3 * D;
  const int n = want_colsum ? 3 * D : 2 * D;
  for (int i = threadIdx.x; i < n; i += 256)
    out[i] = (lds[i] + lds[3 * D + i]) + (lds[6 * D + i] + lds[9 * D + i]);
}

// LayerNorm backward on the all-bf16 streams (dy, x, the incoming residual gradient and dx in bf16; no dropout, no MX image):
// the row8 layout of ln_fwd_row8_kernel.  A workgroup owns rpb rows = 4 waves x (rpb / 4 / RU) batches of RU rows; the per-column
// sums stay in registers and are combined through LDS in wave order, so the partial of a block - and the folded result - is
// deterministic.  rpb (lnr8_rows_per_block): 32 from 8192 rows up - two batches per wave halve the partial rows written here and
// folded later and amortise the LDS combine (C2: 12.7 -> 11.6 us per launch and the layer's fold 12.0 -> 10.4; C3: 16.7 -> 14.2 and
// 15.4 -> 12.2; 48 rows level with 32 at C2 and worse at C3, 64 and 8 worse) - 16 below (short inputs need the workgroups).
// DROP (round 5): live dropout on the all-bf16 streams.  The row gradient leaves TWICE: dx_lo = the residual-gradient stream
// (never masked: the next LayerNorm backward's dres) and dx_m = what the Linear behind the dropout site sees (masked, rescaled:
// the GEMM operand; the column sums - that Linear's bias gradient - are those of the MASKED values, as ln_bwd_reg_kernel's).
// TOK (the bottom layer of a fused stack whose clip / audio gradients nobody asks for): token-major.  The workgroup owns token
// blockIdx.x and walks that token's rows b * tokN + token over the clips b, batch (k, wave) taking clips (4 k + wave) RU ...
// + RU - 1.  The column sums of dx over those rows are row `token` of d pos_embedding: acs accumulates them over the clips and
// they leave through the same wave-ordered combine, so the row gradient itself is never stored (no dx_lo, no fp32 dx, no
// column-sum pass over it); dgamma / dbeta leave as one partial row per workgroup as before.  Deterministic like the rest.
template <int NV8, int RU, bool DROP = false, bool TOK = false>
__global__ __launch_bounds__(256) void ln_bwd_row8_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                          const float* __restrict__ gamma, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const bf16* __restrict__ dres,
                                                          bf16* __restrict__ dx_lo, float* __restrict__ partial, int64_t rows,
                                                          int D, int want_colsum, uint8_t* __restrict__ dxq = nullptr,
                                                          uint8_t* __restrict__ dxs = nullptr, float* __restrict__ dx = nullptr,
                                                          DropCfg drop = kNoDrop, bf16* __restrict__ dx_m = nullptr,
                                                          int rpb = LNR_ROWS_PER_BLOCK, int tokN = 0,
                                                          float* __restrict__ dpos = nullptr) {
  // dx (optional, wave-uniform): the fp32 copy of the row gradient (the bottom layer hands it to the caller)
  // rpb: rows per workgroup, a multiple of 4 RU (host: lnr8_rows_per_block) - a wave's rows come in whole batches of RU
  uint64_t dkey = 0;
  if constexpr (DROP) dkey = drop_key(drop);
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [4 waves][3][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float gm[NV8][8];
#pragma unroll
  for (int i = 0; i < NV8; ++i) {
    const int c = lane * 8 + 512 * i;
#pragma unroll
    for (int k = 0; k < 8; ++k) gm[i][k] = 0.f;
    if (c < D) load8f(gamma + c, gm[i]);
  }
  float adg[NV8][8], adb[NV8][8], acs[NV8][8];
#pragma unroll
  for (int i = 0; i < NV8; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k) adg[i][k] = adb[i][k] = acs[i][k] = 0.f;
  const float invD = 1.0f / (float)D;
#pragma unroll 1
  for (int batch = 0; batch < rpb / 4 / RU; ++batch) {
  // i0 .. i0 + RU - 1 of iend: the batch's rows (TOK: its clips, the row of clip i being i * tokN + this workgroup's token)
  const int64_t i0 = TOK ? (int64_t)(batch * 4 + wave) * RU : (int64_t)blockIdx.x * rpb + wave * (rpb / 4) + batch * RU;
  const int64_t iend = TOK ? rows / tokN : rows;
  const auto row_of = [&](int64_t i) { return TOK ? i * tokN + blockIdx.x : i; };
  uint4 rd[RU][NV8], rx[RU][NV8], rr[RU][NV8];
  float mu[RU], rs[RU];
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    const int64_t row = row_of(i0 + r < iend ? i0 + r : iend - 1);
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      const int c = lane * 8 + 512 * i;
      const bool ok = c < D;
      rd[r][i] = ok ? *reinterpret_cast<const uint4*>(dy + row * D + c) : make_uint4(0u, 0u, 0u, 0u);
      typedef uint32_t u32x4_nt __attribute__((ext_vector_type(4)));  // last use of this x row in the step: non-temporal
      u32x4_nt xv = {0u, 0u, 0u, 0u};
      if (ok) xv = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt*>(x + row * D + c));
      rx[r][i] = make_uint4(xv[0], xv[1], xv[2], xv[3]);
      rr[r][i] = (ok && dres) ? *reinterpret_cast<const uint4*>(dres + row * D + c) : make_uint4(0u, 0u, 0u, 0u);
    }
    mu[r] = mean[row];
    rs[r] = rstd[row];
  }
  float s1[RU], s2[RU];
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      float d[8], v[8];
      unpack8(rd[r][i], d);
      unpack8(rx[r][i], v);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float g = d[k] * gm[i][k];
        a += g;
        b = fmaf(g, (v[k] - mu[r]) * rs[r], b);
      }
    }
    s1[r] = a;
    s2[r] = b;
  }
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    s1[r] = wave_sum(s1[r]) * invD;
    s2[r] = wave_sum(s2[r]) * invD;  // mean(g * xhat)
  }
#pragma unroll
  for (int r = 0; r < RU; ++r) {
    if (i0 + r >= iend) break;
    const int64_t row = row_of(i0 + r);
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      const int c = lane * 8 + 512 * i;
      if (c >= D) continue;
      float d[8], v[8], e[8], o[8];
      unpack8(rd[r][i], d);
      unpack8(rx[r][i], v);
      unpack8(rr[r][i], e);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xh = (v[k] - mu[r]) * rs[r];
        o[k] = rs[r] * (d[k] * gm[i][k] - s1[r] - xh * s2[r]) + e[k];
        adg[i][k] = fmaf(d[k], xh, adg[i][k]);
        adb[i][k] += d[k];
        if constexpr (!DROP) acs[i][k] += o[k];
      }
      if constexpr (TOK) continue;  // (nothing of the row leaves: its column sums are the output)
      *reinterpret_cast<uint4*>(dx_lo + row * D + c) = pack8(o);
      if (dx) {
        *reinterpret_cast<float4*>(dx + row * D + c) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(dx + row * D + c + 4) = make_float4(o[4], o[5], o[6], o[7]);
      }
      if constexpr (DROP) {  // the masked image (element index = row * D + column, as every other user of this site's mask)
        const uint64_t e0 = (uint64_t)row * D + c;
        const float4 f0 = drop_factor4(drop, dkey, e0), f1 = drop_factor4(drop, dkey, e0 + 4);
        o[0] *= f0.x; o[1] *= f0.y; o[2] *= f0.z; o[3] *= f0.w;
        o[4] *= f1.x; o[5] *= f1.y; o[6] *= f1.z; o[7] *= f1.w;
#pragma unroll
        for (int k = 0; k < 8; ++k) acs[i][k] += o[k];
        *reinterpret_cast<uint4*>(dx_m + row * D + c) = pack8(o);
      }
      if (dxq) {  // wave-uniform: MX-FP8 image of the same values (D % 32 == 0: the four lanes of a block are live together)
        const MxBlock mb = mx8_encode(o);
        *reinterpret_cast<uint2*>(dxq + row * D + c) = mb.q;
        if ((lane & 3) == 0) dxs[row * (D >> 5) + (c >> 5)] = (uint8_t)mb.scale;
      }
    }
  }
  }  // batch
  float* mine = lds + wave * 3 * D;
#pragma unroll
  for (int i = 0; i < NV8; ++i) {
    const int c = lane * 8 + 512 * i;
    if (c >= D) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<float4*>(mine + c + 4 * h) = make_float4(adg[i][4 * h], adg[i][4 * h + 1], adg[i][4 * h + 2], adg[i][4 * h + 3]);
      *reinterpret_cast<float4*>(mine + D + c + 4 * h) = make_float4(adb[i][4 * h], adb[i][4 * h + 1], adb[i][4 * h + 2], adb[i][4 * h + 3]);
      *reinterpret_cast<float4*>(mine + 2 * D + c + 4 * h) = make_float4(acs[i][4 * h], acs[i][4 * h + 1], acs[i][4 * h + 2], acs[i][4 * h + 3]);
    }
  }
  __syncthreads();
  float4* out = reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 3 * D);
  const float4* l4 = reinterpret_cast<const float4*>(lds);
  const int n4 = (want_colsum ? 3 * D : 2 * D) >> 2, w4 = (3 * D) >> 2;
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 a = l4[i], b = l4[w4 + i], c = l4[2 * w4 + i], d = l4[3 * w4 + i];
    const float4 v = make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z), (a.w + b.w) + (c.w + d.w));
    if (TOK && i >= (2 * D) >> 2) reinterpret_cast<float4*>(dpos + (int64_t)blockIdx.x * D)[i - ((2 * D) >> 2)] = v;
    else out[i] = v;
  }
}

constexpr int64_t LNR_SHORT_ROWS = 4096;  // up to here the register-path backward runs 4 rows per workgroup
static inline int lnr_rows_per_block(int64_t rows) { return rows <= LNR_SHORT_ROWS ? 4 : LNR_ROWS_PER_BLOCK; }
constexpr int64_t LNR8_BIG_ROWS = 8192;  // from here the row8 backward runs two batches per wave (see the kernel)
static inline int lnr8_rows_per_block(int64_t rows) { return rows >= LNR8_BIG_ROWS ? 2 * LNR_ROWS_PER_BLOCK : LNR_ROWS_PER_BLOCK; }

// The one rule for rows per workgroup of the three backward families: the launchers' grids, the partial rows layernorm_bwd
// hands to the fold and the workspace layernorm_bwd_ws sizes all come from here.
enum LnBwdFamily { LN_BWD_GENERAL, LN_BWD_REG, LN_BWD_ROW8 };
static inline int ln_bwd_rows_per_block(LnBwdFamily f, int64_t rows) {
  return f == LN_BWD_ROW8 ? lnr8_rows_per_block(rows) : f == LN_BWD_REG ? lnr_rows_per_block(rows) : LNB_ROWS_PER_BLOCK;
}
static inline int64_t ln_bwd_blocks(LnBwdFamily f, int64_t rows) { return ceil_div(rows, ln_bwd_rows_per_block(f, rows)); }

// The token-major row8 backward (layernorm_bwd_tok) runs one workgroup per token, each walking the token's `batch` rows: up to
// LNR8_TOK_MAX_BATCH clips.  Above it the row-major launch runs with more, shorter workgroups and d pos is summed from its fp32 dx.
// Measured at 324 and 512 tokens x 512 columns, device time of the launches replaced: batch 32: 32.0 us (row-major with the fp32
// dx 17.7 + column sums 14.3) against 11.1; host-timed back to back at batch 64 / 128 / 256: 42 / 77 / 140 us against 21 / 33 /
// 56 - the token-major form was the faster one at every batch tried, so the bound is the largest batch that was measured.
constexpr int LNR8_TOK_MAX_BATCH = 256;
bool layernorm_bwd_tok_ok(int batch, int tokens, int dim) {
  return batch > 0 && tokens > 0 && dim % 8 == 0 && dim <= 1536 && ln_row8_on() && batch <= LNR8_TOK_MAX_BATCH;
}

// tokens: the caller may run the token-major form on these rows (one partial row per token)
size_t layernorm_bwd_ws(int64_t rows, int dim, int tokens) {
  const int64_t nb = std::max({ln_bwd_blocks(LN_BWD_GENERAL, rows), ln_bwd_blocks(LN_BWD_REG, rows), ln_bwd_blocks(LN_BWD_ROW8, rows),
                               (int64_t)tokens});
  return (size_t)nb * 3 * dim * sizeof(float);
}

// ---- launchers: one per kernel template (grid and LDS bytes, launch inside the timing scope, launch check).  The two with
// [4 waves][3][D] floats of LDS pass the default 64 KiB limit at D > 1365: each raises the limit of the instantiation it is about
// to launch, once per device, to what that instantiation can need. ----
template <bool VEC, typename DyT>
static int launch_ln_bwd(const TimingScope* ts, hipStream_t s, const DyT* dy, const float* x, const float* gamma, const float* mean,
                         const float* rstd, const float* dres, float* dx, bf16* dx_lo, float* partial, int64_t rows, int D, int wc) {
  const size_t lds = (size_t)3 * D * sizeof(float);
  launch_in_scope(ts, ln_bwd_kernel<DyT, VEC>, dim3((unsigned)ln_bwd_blocks(LN_BWD_GENERAL, rows)), dim3(256), (uint32_t)lds, s, dy, x,
                  gamma, mean, rstd, dres, dx, dx_lo, partial, rows, D, wc);
  return check_launch("ln_bwd_kernel");
}

template <int NV, typename DyT, typename XT, typename ResT>
static int launch_ln_bwd_reg(const TimingScope* ts, hipStream_t s, const DyT* dy, const XT* x, const float* gamma, const float* mean,
                             const float* rstd, const ResT* dres, float* dx, bf16* dx_lo, float* partial, int64_t rows, int D, int wc,
                             const DropCfg& drop, uint8_t* dxq, uint8_t* dxs) {
  const size_t lds = (size_t)4 * 3 * D * sizeof(float);
  static PerDeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)ln_bwd_reg_kernel<DyT, NV, ResT, XT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       4 * 3 * 256 * NV * (int)sizeof(float));
    AVF_REQUIRE(e == hipSuccess, "layernorm_bwd: cannot raise dynamic LDS limit");
    raised.mark();
  }
  launch_in_scope(ts, ln_bwd_reg_kernel<DyT, NV, ResT, XT>, dim3((unsigned)ln_bwd_blocks(LN_BWD_REG, rows)), dim3(256), (uint32_t)lds, s,
                  dy, x, gamma, mean, rstd, dres, dx, dx_lo, partial, rows, D, wc, drop, dxq, dxs, ln_bwd_rows_per_block(LN_BWD_REG, rows));
  return check_launch("ln_bwd_reg_kernel");
}

template <int NV8, int RU, bool DROP>
static int launch_ln_bwd_row8(const TimingScope* ts, hipStream_t s, const bf16* dy, const bf16* x, const float* gamma,
                              const float* mean, const float* rstd, const bf16* dres, bf16* dx_lo, float* partial, int64_t rows, int D,
                              int wc, uint8_t* dxq, uint8_t* dxs, float* dx, const DropCfg& drop, bf16* dx_m) {
  const size_t lds = (size_t)4 * 3 * D * sizeof(float);
  static PerDeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)ln_bwd_row8_kernel<NV8, RU, DROP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       4 * 3 * 512 * NV8 * (int)sizeof(float));
    AVF_REQUIRE(e == hipSuccess, "layernorm_bwd: cannot raise dynamic LDS limit");
    raised.mark();
  }
  launch_in_scope(ts, ln_bwd_row8_kernel<NV8, RU, DROP>, dim3((unsigned)ln_bwd_blocks(LN_BWD_ROW8, rows)), dim3(256), (uint32_t)lds, s,
                  dy, x, gamma, mean, rstd, dres, dx_lo, partial, rows, D, wc, dxq, dxs, dx, drop, dx_m,
                  ln_bwd_rows_per_block(LN_BWD_ROW8, rows), 0, (float*)nullptr);
  return check_launch("ln_bwd_row8_kernel");
}

template <int NV8, int RU>
static int launch_ln_bwd_row8_tok(const TimingScope* ts, hipStream_t s, const bf16* dy, const bf16* x, const float* gamma,
                                  const float* mean, const float* rstd, const bf16* dres, float* dpos, float* partial, int batch,
                                  int tokens, int D) {
  const size_t lds = (size_t)4 * 3 * D * sizeof(float);
  static PerDeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)ln_bwd_row8_kernel<NV8, RU, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       4 * 3 * 512 * NV8 * (int)sizeof(float));
    AVF_REQUIRE(e == hipSuccess, "layernorm_bwd_tok: cannot raise dynamic LDS limit");
    raised.mark();
  }
  const int nbatch = (int)ceil_div((int64_t)batch, 4 * RU);  // batches of RU clips per wave
  launch_in_scope(ts, ln_bwd_row8_kernel<NV8, RU, false, true>, dim3((unsigned)tokens), dim3(256), (uint32_t)lds, s, dy, x, gamma, mean,
                  rstd, dres, (bf16*)nullptr, partial, (int64_t)batch * tokens, D, 1, (uint8_t*)nullptr, (uint8_t*)nullptr,
                  (float*)nullptr, kNoDrop, (bf16*)nullptr, nbatch * 4 * RU, tokens, dpos);
  return check_launch("ln_bwd_row8_kernel(tok)");
}

// the bottom LayerNorm of a fused stack, all-bf16 streams: dpos[t, :] = sum_b dx[b * tokens + t, :] (fp32 [tokens, dim]) with
// dgamma / dbeta, and no dx at all (ln_bwd_row8_kernel, TOK); ws: layernorm_bwd_ws(rows, dim, tokens)
int layernorm_bwd_tok(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres,
                      float* dpos, float* dgamma, float* dbeta, void* ws, int batch, int tokens, int dim, hipStream_t s,
                      FoldJob* defer_fold) {
  AVF_REQUIRE(dy && x && gamma && mean && rstd && dpos && ws, "layernorm_bwd_tok: null pointer");
  AVF_REQUIRE(layernorm_bwd_tok_ok(batch, tokens, dim), "layernorm_bwd_tok: shape outside the token-major rule (batch=%d dim=%d)", batch, dim);
  AVF_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dres | (uintptr_t)dpos | (uintptr_t)ws) & 15) == 0,
              "layernorm_bwd_tok: pointers must be 16-byte aligned");
  const int64_t rows = (int64_t)batch * tokens;
  TimingScope ts(KC_LAYERNORM, 0.0, (double)rows * dim * (2.0 + 2.0 + (dres ? 2.0 : 0.0)) + (double)tokens * dim * 4.0, s, /*per_kernel=*/true);
  float* partial = (float*)ws;
  AVF_TRY(ln_nv8(dim, [&](auto nv8, auto ru) {
    return launch_ln_bwd_row8_tok<decltype(nv8)::value, decltype(ru)::value>(&ts, s, (const bf16*)dy, (const bf16*)x, gamma, mean, rstd,
                                                                             (const bf16*)dres, dpos, partial, batch, tokens, dim);
  }));
  const FoldJob job{partial, tokens, 3 * dim, dim, dgamma, dbeta, nullptr};
  if (defer_fold) {
    *defer_fold = job;
    return 0;
  }
  return fold_job(job, s);
}

int layernorm_bwd(const void* dy, int dy_dtype, const void* xv, const float* gamma, const float* mean,
                  const float* rstd, const void* dres, float* dx, void* dx_lo, float* dgamma, float* dbeta,
                  float* dcolsum, void* ws, int64_t rows, int dim, hipStream_t s, const DropCfg& drop,
                  FoldJob* defer_fold, int dres_dtype, int x_dtype, void* mx_q, void* mx_s, void* dx_m) {
  // dx_m (with a live `drop`, all-bf16 streams only): dx_lo is then the UNMASKED stream and dx_m the masked image (row8 DROP)
  AVF_REQUIRE(!dx_m || (drop.thresh16 && dx_lo && dy_dtype == AVF_BF16 && x_dtype == AVF_BF16 && (!dres || dres_dtype == AVF_BF16) &&
                        dim % 8 == 0 && dim <= 1536 && !mx_q),
              "layernorm_bwd: a separate masked image needs live dropout on the all-bf16 streams (dim %% 8 == 0, no MX-FP8 image)");
  AVF_REQUIRE(rows > 0 && dim > 0 && ws, "layernorm_bwd: bad arguments");
  AVF_REQUIRE(!mx_q || (mx_s && dy_dtype == AVF_BF16 && dim % 32 == 0 && dim <= 1536 && ((uintptr_t)mx_q & 3) == 0),
              "layernorm_bwd: the MX-FP8 image of dx needs bf16 dy, dim %% 32 == 0 and dim <= 1536 (dim=%d)", dim);
  AVF_REQUIRE(x_dtype == AVF_F32 || (x_dtype == AVF_BF16 && dy_dtype == AVF_BF16 && dim % 4 == 0 && dim <= 1536),
              "layernorm_bwd: a bf16 LayerNorm input needs bf16 dy, dim %% 4 == 0 and dim <= 1536");
  AVF_REQUIRE(dres_dtype == AVF_F32 || (dres_dtype == AVF_BF16 && dy_dtype == AVF_BF16 && dim % 4 == 0 && dim <= 1536 &&
                                         (!drop.thresh16 || dx_m) && dx_lo),
              "layernorm_bwd: a bf16 residual gradient needs bf16 dy, a bf16 output, dim %% 4 == 0, dim <= 1536, and with dropout a "
              "separate masked image");
  AVF_REQUIRE(dx || dx_lo, "layernorm_bwd: no output");
  AVF_REQUIRE(dx || (dim % 4 == 0 && dim <= 1536), "layernorm_bwd: dim %d runs the general kernel, which needs the fp32 dx", dim);
  AVF_REQUIRE(!drop.thresh16 || (dim % 4 == 0 && dim <= 1536), "layernorm_bwd: dropout needs dim %% 4 == 0 and dim <= 1536");
  AVF_REQUIRE((size_t)3 * dim * sizeof(float) <= 64 * 1024, "layernorm_bwd: dim %d too large", dim);
  TimingScope ts(KC_LAYERNORM, 0.0,
                 (double)rows * dim * ((dy_dtype == AVF_BF16 ? 2.0 : 4.0) + (x_dtype == AVF_BF16 ? 2.0 : 4.0) + (dres ? (dres_dtype == AVF_BF16 ? 2.0 : 4.0) : 0.0) +
                                       (dx ? 4.0 : 0.0) + (dx_lo ? 2.0 : 0.0)), s, /*per_kernel=*/true);
  float* partial = (float*)ws;
  const int wc = dcolsum ? 1 : 0;
  const float *x = (const float*)xv, *drf = (const float*)dres;
  const bf16 *dyb = (const bf16*)dy, *xb = (const bf16*)xv, *drb = (const bf16*)dres;
  uint8_t *dxq = (uint8_t*)mx_q, *dxs = (uint8_t*)mx_s;
  const bool fast = (dim % 4 == 0) && dim <= 1536 && (dy_dtype == AVF_F32 || dy_dtype == AVF_BF16);
  const bool row8 = fast && x_dtype == AVF_BF16 && dy_dtype == AVF_BF16 && (!dres || dres_dtype == AVF_BF16) && dx_lo &&
                    (!drop.thresh16 || dx_m) && (!mx_q || dim % 32 == 0) && dim % 8 == 0 && (ln_row8_on() || dx_m);
  const int nb = (int)ln_bwd_blocks(row8 ? LN_BWD_ROW8 : fast ? LN_BWD_REG : LN_BWD_GENERAL, rows);
  if (row8) {
    AVF_TRY(ln_nv8(dim, [&](auto nv8, auto ru) {
      constexpr int NV8 = decltype(nv8)::value, RU = decltype(ru)::value;
      if (dx_m)
        return launch_ln_bwd_row8<NV8, RU, true>(&ts, s, dyb, xb, gamma, mean, rstd, drb, (bf16*)dx_lo, partial, rows, dim, wc, nullptr,
                                                 nullptr, dx, drop, (bf16*)dx_m);
      return launch_ln_bwd_row8<NV8, RU, false>(&ts, s, dyb, xb, gamma, mean, rstd, drb, (bf16*)dx_lo, partial, rows, dim, wc, dxq, dxs,
                                                dx, kNoDrop, nullptr);
    }));
  } else if (fast) {
    // the register kernel: the storage types of dy, x and dres from the pointers, NV at compile time
    auto reg = [&](auto* dyp, auto* xp, auto* drp) {
      return ln_nv(dim, [&](auto nv) {
        return launch_ln_bwd_reg<decltype(nv)::value>(&ts, s, dyp, xp, gamma, mean, rstd, drp, dx, (bf16*)dx_lo, partial, rows, dim, wc,
                                                      drop, dxq, dxs);
      });
    };
    if (x_dtype == AVF_BF16 && dres_dtype == AVF_BF16) AVF_TRY(reg(dyb, xb, drb));
    else if (x_dtype == AVF_BF16) AVF_TRY(reg(dyb, xb, drf));
    else if (dres_dtype == AVF_BF16) AVF_TRY(reg(dyb, x, drb));
    else if (dy_dtype == AVF_F32) AVF_TRY(reg((const float*)dy, x, drf));
    else AVF_TRY(reg(dyb, x, drf));
  } else {
    const bool vec = (dim & 3) == 0;
    auto general = [&](auto* dyp) {
      if (vec) return launch_ln_bwd<true>(&ts, s, dyp, x, gamma, mean, rstd, drf, dx, (bf16*)dx_lo, partial, rows, dim, wc);
      return launch_ln_bwd<false>(&ts, s, dyp, x, gamma, mean, rstd, drf, dx, (bf16*)dx_lo, partial, rows, dim, wc);
    };
    if (dy_dtype == AVF_F32) AVF_TRY(general((const float*)dy));
    else if (dy_dtype == AVF_BF16) AVF_TRY(general(dyb));
    else AVF_REQUIRE(false, "layernorm_bwd: bad dtype %d", dy_dtype);
  }
  const int width = 3 * dim;
  if (defer_fold) {
    AVF_REQUIRE(width % 4 == 0 && (((uintptr_t)partial) & 15) == 0, "layernorm_bwd: deferred fold needs dim %% 4 == 0");
    *defer_fold = FoldJob{partial, nb, width, dim, dgamma, dbeta, dcolsum};
    return 0;
  }
  return fold_job(FoldJob{partial, nb, width, dim, dgamma, dbeta, dcolsum}, s);
}

}  // namespace avf
