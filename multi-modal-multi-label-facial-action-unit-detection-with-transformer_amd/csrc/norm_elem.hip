// norm_elem.hip - HBM-bound element-wise and reduction kernels around the hot path: partial folds and column sums (bias
// gradients), fp32->bf16 casts / dropout helpers / weight images, the AU loss, token fusion and token mean (LayerNorm: layernorm.hip).
//
// Reference math: models/loss.py:63-103 (AULoss), models/avformer.py:95-103 (token fusion).
#include <algorithm>

#include "common.hpp"

namespace avf {

// out[j] = sum_b partial[b][j], j in [0, width): 32 columns x 8 partial-groups per block

__global__ __launch_bounds__(256) void fold_partials_kernel(const float* __restrict__ partial, int nb, int width,
                                                            float* __restrict__ o0, float* __restrict__ o1,
                                                            float* __restrict__ o2, int seg) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cl;
  float a0 = 0.f, a1 = 0.f;
  if (col < width) {
    int b = grp;
    for (; b + 8 < nb; b += 16) {
      a0 += partial[(int64_t)b * width + col];
      a1 += partial[(int64_t)(b + 8) * width + col];
    }
    if (b < nb) a0 += partial[(int64_t)b * width + col];
  }
  red[grp][cl] = a0 + a1;
  __syncthreads();
  if (grp == 0 && col < width) {
    float v = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) + ((red[4][cl] + red[5][cl]) + (red[6][cl] + red[7][cl]));
    const int which = col / seg, c = col - which * seg;
    float* dst = which == 0 ? o0 : (which == 1 ? o1 : o2);
    if (dst) dst[c] = v;
  }
}

// width % 4 == 0: FOLD_COLS columns x FOLD_RG row groups per block, 16-byte loads, 8 loads in flight (common.hpp)
__global__ __launch_bounds__(256) void fold_partials_vec_kernel(FoldJob job) {
  __shared__ float4 red[FOLD_RG][FOLD_COLS / 4];
  fold_columns_vec(job, blockIdx.x, red);
}

static int launch_fold(const float* partial, int nb, int width, float* o0, float* o1, float* o2, int seg, hipStream_t s) {
  if (width % 4 == 0 && (((uintptr_t)partial) & 15) == 0)
    fold_partials_vec_kernel<<<(unsigned)ceil_div(width, FOLD_COLS), 256, 0, s>>>(FoldJob{partial, nb, width, seg, o0, o1, o2});
  else
    fold_partials_kernel<<<(unsigned)ceil_div(width, 32), 256, 0, s>>>(partial, nb, width, o0, o1, o2, seg);
  return check_launch("fold_partials_kernel");
}

int fold_partials(const float* partial, int nb, int width, float* out, hipStream_t s) {
  return launch_fold(partial, nb, width, out, nullptr, nullptr, width, s);
}

int fold_job(const FoldJob& j, hipStream_t s) { return launch_fold(j.partial, j.nb, j.width, j.o0, j.o1, j.o2, j.seg, s); }

// every job of a list in ONE launch (the parity mode's layer backward: its LayerNorm column folds were a launch each - 19 tiny
// launches per C2 step); jobs with a null partial are skipped.  Falls back to one launch per job for unaligned / odd widths.
struct FoldStarts { int first[kFoldMax + 1]; };  // first[j] = first block of job j; first[kFoldMax] = the grid
__global__ __launch_bounds__(256) void fold_list_kernel(FoldList fl, FoldStarts st) {
  __shared__ float4 red[FOLD_RG][FOLD_COLS / 4];
  const int b = blockIdx.x;
  int j = 0;
  for (int i = 1; i < kFoldMax; ++i)  // (uniform; an empty job has first[i] == first[i + 1] and is never the last match)
    if (b >= st.first[i] && st.first[i] < st.first[i + 1]) j = i;
  fold_columns_vec(fl.job[j], b - st.first[j], red);
}
int fold_list(const FoldList& fl, hipStream_t s) {
  AVF_REQUIRE(fl.count >= 0 && fl.count <= kFoldMax, "fold_list: %d jobs (at most %d)", fl.count, kFoldMax);
  FoldStarts st;
  bool vec = true;
  int total = 0;
  for (int j = 0; j < kFoldMax; ++j) {
    st.first[j] = total;
    const FoldJob& job = fl.job[j];
    if (j >= fl.count || !job.partial) continue;
    total += (int)ceil_div(job.width, FOLD_COLS);
    vec = vec && job.width % 4 == 0 && (((uintptr_t)job.partial) & 15) == 0;
  }
  st.first[kFoldMax] = total;
  if (total == 0) return 0;
  if (!vec) {
    for (int j = 0; j < fl.count; ++j)
      if (fl.job[j].partial) AVF_TRY(fold_job(fl.job[j], s));
    return 0;
  }
  fold_list_kernel<<<(unsigned)total, 256, 0, s>>>(fl, st);
  return check_launch("fold_list_kernel");
}

// =============================================================================================
// column sums: out[c] = sum_r in[r, c]  (bias gradients - "db = sum_rows dY")
// =============================================================================================
constexpr int CS_ROW_CHUNKS = 128;

template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ in, int64_t rows, int cols, int64_t ld,
                                                     float* __restrict__ partial) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  const int64_t per = ceil_div(rows, (int64_t)gridDim.y);
  const int64_t r0 = (int64_t)blockIdx.y * per;
  const int64_t r1 = r0 + per < rows ? r0 + per : rows;
  if (col >= cols) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int64_t r = r0;
  for (; r + 3 < r1; r += 4) {
    a0 += to_f32<T>(in[(r + 0) * ld + col]);
    a1 += to_f32<T>(in[(r + 1) * ld + col]);
    a2 += to_f32<T>(in[(r + 2) * ld + col]);
    a3 += to_f32<T>(in[(r + 3) * ld + col]);
  }
  for (; r < r1; ++r) a0 += to_f32<T>(in[r * ld + col]);
  partial[(int64_t)blockIdx.y * cols + col] = (a0 + a1) + (a2 + a3);
}

static int colsum_chunks(int64_t rows) {
  int64_t c = ceil_div(rows, 64);
  if (c > CS_ROW_CHUNKS) c = CS_ROW_CHUNKS;
  if (c < 1) c = 1;
  return (int)c;
}
size_t colsum_ws(int64_t rows, int cols) { return (size_t)colsum_chunks(rows) * cols * sizeof(float); }

int colsum(const void* in, int in_dtype, int64_t rows, int cols, int64_t ld, float* out, void* ws, hipStream_t s) {
  AVF_REQUIRE(rows > 0 && cols > 0 && ws && out, "colsum: bad arguments");
  const int ch = colsum_chunks(rows);
  dim3 grid((unsigned)ceil_div(cols, 256), ch);
  // one row chunk (up to 64 rows - the batch sum behind d pos_embedding: 32 rows x 165 888 columns at C2): the kernel's "partial"
  // row IS the result, written straight to `out`; the fold of one row was a 10 us copy launch
  float* dst = ch == 1 ? out : (float*)ws;
  if (in_dtype == AVF_F32)
    colsum_kernel<float><<<grid, 256, 0, s>>>((const float*)in, rows, cols, ld, dst);
  else if (in_dtype == AVF_BF16)
    colsum_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)in, rows, cols, ld, dst);
  else
    AVF_REQUIRE(false, "colsum: bad dtype %d", in_dtype);
  AVF_TRY(check_launch("colsum_kernel"));
  if (ch == 1) return 0;
  return launch_fold((const float*)ws, ch, cols, out, nullptr, nullptr, cols, s);
}

// =============================================================================================
// casts / weight preparation
// =============================================================================================
__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ in, bf16* __restrict__ out,
                                                        int64_t n, DropCfg drop) {
  const uint64_t dkey = drop.thresh16 ? drop_key(drop) : 0;
  int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (; i + 3 < n; i += stride) {
    float4 v = *reinterpret_cast<const float4*>(in + i);
    if (drop.thresh16) {
      const float4 f = drop_factor4(drop, dkey, (uint64_t)i);
      v.x *= f.x; v.y *= f.y; v.z *= f.z; v.w *= f.w;
    }
    store4<bf16>(out + i, v);
  }
  // tail (n not a multiple of 4): handled by the thread whose i lands on it
  if (i < n && i + 3 >= n)
    for (int64_t j = i; j < n; ++j) out[j] = from_f32<bf16>(in[j]);
}

__global__ __launch_bounds__(256) void dropout_factors_kernel(DropCfg drop, float* __restrict__ out, int64_t n) {
  const uint64_t dkey = drop_key(drop);
  int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (; i + 3 < n; i += stride) *reinterpret_cast<float4*>(out + i) = drop_factor4(drop, dkey, (uint64_t)i);
}
int dropout_factors(const DropCfg& drop, float* out, int64_t n, hipStream_t s) {
  AVF_REQUIRE(n > 0 && n % 4 == 0 && drop.thresh16, "dropout_factors: n %% 4 == 0 and p > 0 required");
  int64_t blocks = ceil_div(n, 1024);
  if (blocks > 2048) blocks = 2048;
  dropout_factors_kernel<<<(unsigned)blocks, 256, 0, s>>>(drop, out, n);
  return check_launch("dropout_factors_kernel");
}

__global__ __launch_bounds__(256) void mask_copy_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n,
                                                            DropCfg drop) {
  const uint64_t dkey = drop_key(drop);
  int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (; i + 3 < n; i += stride) {
    float4 v = *reinterpret_cast<const float4*>(in + i);
    const float4 f = drop_factor4(drop, dkey, (uint64_t)i);
    *reinterpret_cast<float4*>(out + i) = make_float4(v.x * f.x, v.y * f.y, v.z * f.z, v.w * f.w);
  }
}
int mask_copy_f32(const float* in, float* out, int64_t n, hipStream_t s, const DropCfg& drop) {
  AVF_REQUIRE(n > 0 && n % 4 == 0 && drop.thresh16, "mask_copy_f32: n %% 4 == 0 and p > 0 required");
  AVF_REQUIRE((((uintptr_t)in) & 15) == 0 && (((uintptr_t)out) & 15) == 0, "mask_copy_f32: pointers must be 16B aligned");
  int64_t blocks = ceil_div(n, 1024);
  if (blocks > 2048) blocks = 2048;
  mask_copy_f32_kernel<<<(unsigned)blocks, 256, 0, s>>>(in, out, n, drop);
  return check_launch("mask_copy_f32_kernel");
}

int cast_f32_to_bf16(const float* in, void* out, int64_t n, hipStream_t s, const DropCfg& drop) {
  AVF_REQUIRE(n > 0, "cast: n must be positive");
  AVF_REQUIRE(!drop.thresh16 || n % 4 == 0, "cast: dropout needs n %% 4 == 0");
  AVF_REQUIRE((((uintptr_t)in) & 15) == 0 && (((uintptr_t)out) & 7) == 0, "cast: pointers must be 16B/8B aligned");
  int64_t blocks = ceil_div(n, 1024);
  if (blocks > 2048) blocks = 2048;
  cast_bf16_kernel<<<(unsigned)blocks, 256, 0, s>>>(in, (bf16*)out, n, drop);
  return check_launch("cast_bf16_kernel");
}

// w [R,C] fp32 -> w_lo [R,C] bf16 and w_t_lo [C,R] bf16, 32x32 tiles through LDS
__global__ __launch_bounds__(256) void prep_weight_kernel(const float* __restrict__ w, bf16* __restrict__ w_lo,
                                                          bf16* __restrict__ w_t, int R, int C) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = r0 + ty + 8 * i, c = c0 + tx;
    float v = (r < R && c < C) ? w[(int64_t)r * C + c] : 0.f;
    tile[ty + 8 * i][tx] = v;
    if (w_lo && r < R && c < C) w_lo[(int64_t)r * C + c] = from_f32<bf16>(v);
  }
  __syncthreads();
  if (w_t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int c = c0 + ty + 8 * i, r = r0 + tx;  // output row = c, output col = r
      if (c < C && r < R) w_t[(int64_t)c * R + r] = from_f32<bf16>(tile[tx][ty + 8 * i]);
    }
  }
}

// up to 4 weights in one launch (blockIdx.z selects the matrix)
__global__ __launch_bounds__(256) void prep_weights_multi_kernel(PrepBatch b) {
  __shared__ float tile[32][33];
  const PrepDesc d = b.d[blockIdx.z];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  if (c0 >= d.C || r0 >= d.R) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = r0 + ty + 8 * i, c = c0 + tx;
    float v = (r < d.R && c < d.C) ? d.w[(int64_t)r * d.C + c] : 0.f;
    tile[ty + 8 * i][tx] = v;
    if (r < d.R && c < d.C) {
      const bf16 q = from_f32<bf16>(r < d.lo_scaled_rows ? v * d.lo_scale : v);
      d.lo[(int64_t)r * d.C + c] = q;
      // the fragment-major image of the same values (round 5: five pack_ws launches per layer before - 58 us of a 555 us
      // TFormer step that prepares its weights in every forward)
      if (d.lo_p) *reinterpret_cast<bf16*>(reinterpret_cast<char*>(d.lo_p) + pack_ws_off(r, c)) = q;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int c = c0 + ty + 8 * i, r = r0 + tx;
    if (c < d.C && r < d.R) {
      const bf16 q = from_f32<bf16>(tile[tx][ty + 8 * i]);
      d.t[(int64_t)c * d.R + r] = q;
      if (d.t_p) *reinterpret_cast<bf16*>(reinterpret_cast<char*>(d.t_p) + pack_ws_off(c, r)) = q;
    }
  }
}

int prep_weights_multi(const PrepBatch& b, int count, hipStream_t s) {
  AVF_REQUIRE(count >= 1 && count <= 4, "prep_weights_multi: count must be 1..4");
  int mr = 0, mc = 0;
  for (int i = 0; i < count; ++i) {
    AVF_REQUIRE(b.d[i].w && b.d[i].lo && b.d[i].t && b.d[i].R > 0 && b.d[i].C > 0, "prep_weights_multi: bad descriptor");
    mr = b.d[i].R > mr ? b.d[i].R : mr;
    mc = b.d[i].C > mc ? b.d[i].C : mc;
  }
  dim3 grid((unsigned)ceil_div(mc, 32), (unsigned)ceil_div(mr, 32), (unsigned)count);
  prep_weights_multi_kernel<<<grid, 256, 0, s>>>(b);
  return check_launch("prep_weights_multi_kernel");
}

int prep_weight_bf16(const float* w, void* w_lo, void* w_t_lo, int rows, int cols, hipStream_t s) {
  AVF_REQUIRE(rows > 0 && cols > 0, "prep_weight: bad shape");
  dim3 grid((unsigned)ceil_div(cols, 32), (unsigned)ceil_div(rows, 32));
  prep_weight_kernel<<<grid, 256, 0, s>>>(w, (bf16*)w_lo, (bf16*)w_t_lo, rows, cols);
  return check_launch("prep_weight_kernel");
}

// =============================================================================================
// AULoss (models/loss.py:75-103): one block; rows are few (a batch of clips).
//   keep_b = (y[b,0] != ignore);  l = (1-y) z + (1 + (w-1) y) softplus(-z);  loss = mean over kept
//   dl/dz = sigmoid(z) (1 - y + w y) - w y, scaled by 1/(ncls * kept), 0 for dropped rows.
// =============================================================================================
__global__ __launch_bounds__(256) void au_loss_kernel(const float* __restrict__ z, int64_t ldz,
                                                      const float* __restrict__ y, int64_t ldy,
                                                      const float* __restrict__ pw, float ignore, int rows, int ncls,
                                                      float* __restrict__ loss, float* __restrict__ grad, int sum_mode,
                                                      int gwidth) {
  // gwidth >= ncls: rows of `grad` are gwidth wide, columns ncls .. gwidth-1 written as zeros (the gradient of the reference's
  // [B,21] output row whose slots 0..11 are the AU logits: what autograd's slice backward would build with a fill and a copy)
  __shared__ float red[4];
  __shared__ int redc[4];
  float acc = 0.f;
  int kept = 0;
  for (int r = threadIdx.x; r < rows; r += 256) kept += (y[(int64_t)r * ldy] != ignore) ? 1 : 0;
  for (int i = threadIdx.x; i < rows * ncls; i += 256) {
    const int r = i / ncls, c = i - r * ncls;
    if (y[(int64_t)r * ldy] != ignore) {
      const float zz = z[(int64_t)r * ldz + c], yy = y[(int64_t)r * ldy + c], w = pw[c];
      // softplus(-z) = max(-z,0) + log1p(exp(-|z|))
      const float sp = fmaxf(-zz, 0.f) + log1pf(expf(-fabsf(zz)));
      acc += (1.f - yy) * zz + (1.f + (w - 1.f) * yy) * sp;
    }
  }
  acc = wave_sum(acc);
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = acc;
    redc[threadIdx.x >> 6] = kept;
  }
  __syncthreads();
  const float total = (red[0] + red[1]) + (red[2] + red[3]);
  const int nk = redc[0] + redc[1] + redc[2] + redc[3];
  // sum_mode (data-parallel shards): loss[0] = sum over kept rows of the row mean, loss[1] = kept rows; the caller
  // divides by the GLOBAL kept count after reducing both over the ranks (loss.py:85-102 is a ratio)
  const float denom = (sum_mode ? 1.0f : (float)nk) * (float)ncls;
  if (threadIdx.x == 0) {
    loss[0] = total / denom;  // 0/0 -> NaN when every row is ignored (as the reference)
    if (sum_mode) loss[1] = (float)nk;
  }
  const float inv = 1.0f / denom;
  for (int i = threadIdx.x; i < rows * gwidth; i += 256) {
    const int r = i / gwidth, c = i - r * gwidth;
    float g = 0.f;
    if (c < ncls && y[(int64_t)r * ldy] != ignore) {
      const float zz = z[(int64_t)r * ldz + c], yy = y[(int64_t)r * ldy + c], w = pw[c];
      const float sg = 1.0f / (1.0f + expf(-zz));
      g = (sg * (1.f - yy + w * yy) - w * yy) * inv;
    }
    grad[i] = g;
  }
}

// ---------------------------------------------------------------------------------------------
// Token-sequence plumbing of the callers either side of the stack (the fused [B, T_v + T_a, dim] sequence of
// BASELINE.json's configs; reference fusion: models/avformer.py:95-103, mean pooling: models/tformer.py head):
// sequence fusion + positional embedding in one pass, token-mean pooling, and its backward, which writes the top
// layer's incoming gradient in fp32 AND bf16 and its column sums analytically (= sum_b g[b,:]).
// ---------------------------------------------------------------------------------------------
constexpr int TOK_ROWS_PER_BLOCK = 4;

// one workgroup per TOK_ROWS_PER_BLOCK token rows (row = b * T + t): no per-element index division
template <typename OutT>  // float: float4 stores; bf16: the bf16 residual stream, 8-byte stores
__global__ __launch_bounds__(256) void fuse_tokens_kernel(const float4* __restrict__ clip, const float4* __restrict__ audio,
                                                         const float4* __restrict__ pos, OutT* __restrict__ out, int Tv,
                                                         int Ta, int D4, int64_t rows) {
  // the block's TOK_ROWS_PER_BLOCK x D4 quads are dealt to the 256 threads as one flat range (D4 = 128: two rows at a time,
  // every thread busy; one row per pass left half of them idle)
  const int T = Tv + Ta;
  const int64_t row0 = (int64_t)blockIdx.x * TOK_ROWS_PER_BLOCK;
  if constexpr (sizeof(OutT) == 2) {
    if ((D4 & 1) == 0 && ((uintptr_t)out & 15) == 0) {  // bf16 rows of a multiple of 8 columns: two quads in, ONE 16-byte store out (8-byte stores: 1.1 TB/s)
      const int D8 = D4 >> 1;
      for (int i = threadIdx.x; i < TOK_ROWS_PER_BLOCK * D8; i += 256) {
        const int rr = i / D8, c = i - rr * D8;
        const int64_t row = row0 + rr;
        if (row >= rows) return;  // (rr grows with i)
        const int64_t b = row / T;
        const int t = (int)(row - b * T);
        const float4* src = t < Tv ? clip + (b * Tv + t) * D4 : audio + (b * Ta + (t - Tv)) * D4;
        float4 v0 = src[2 * c], v1 = src[2 * c + 1];
        if (pos) {
          const float4 p0 = pos[(int64_t)t * D4 + 2 * c], p1 = pos[(int64_t)t * D4 + 2 * c + 1];
          v0.x += p0.x; v0.y += p0.y; v0.z += p0.z; v0.w += p0.w;
          v1.x += p1.x; v1.y += p1.y; v1.z += p1.z; v1.w += p1.w;
        }
        const float o[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        *reinterpret_cast<uint4*>(out + (row * D4 + 2 * c) * 4) = pack8(o);
      }
      return;
    }
  }
  for (int i = threadIdx.x; i < TOK_ROWS_PER_BLOCK * D4; i += 256) {
    const int rr = i / D4, c = i - rr * D4;
    const int64_t row = row0 + rr;
    if (row >= rows) return;  // (rr grows with i)
    const int64_t b = row / T;
    const int t = (int)(row - b * T);
    const float4* src = t < Tv ? clip + (b * Tv + t) * D4 : audio + (b * Ta + (t - Tv)) * D4;
    float4 v = src[c];
    if (pos) {
      const float4 p = pos[(int64_t)t * D4 + c];
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    store4<OutT>(out + (row * D4 + c) * 4, v);
  }
}

// grid (ceil(D4/16), B); 256 threads = 16 float4 column groups x 16 token lanes
template <typename InT>
__global__ __launch_bounds__(256) void token_mean_fwd_kernel(const InT* __restrict__ y, float4* __restrict__ out, int T,
                                                            int D4) {
  __shared__ float4 red[16][16];
  const int cg = threadIdx.x & 15, tl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cg;
  const int64_t b = blockIdx.y;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < D4) {
    const InT* base = y + (b * T * D4 + c) * 4;
    const int64_t ld = (int64_t)D4 * 4;
    int t = tl;
    for (; t + 48 < T; t += 64) {  // four independent loads in flight
      const float4 v0 = load4<InT>(base + t * ld), v1 = load4<InT>(base + (t + 16) * ld), v2 = load4<InT>(base + (t + 32) * ld),
                   v3 = load4<InT>(base + (t + 48) * ld);
      acc.x += (v0.x + v1.x) + (v2.x + v3.x); acc.y += (v0.y + v1.y) + (v2.y + v3.y);
      acc.z += (v0.z + v1.z) + (v2.z + v3.z); acc.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; t < T; t += 16) {
      const float4 v = load4<InT>(base + t * ld);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  red[tl][cg] = acc;
  __syncthreads();
  if (tl == 0 && c < D4) {
    float4 r = red[0][cg];
#pragma unroll
    for (int j = 1; j < 16; ++j) { r.x += red[j][cg].x; r.y += red[j][cg].y; r.z += red[j][cg].z; r.w += red[j][cg].w; }
    const float inv = 1.0f / (float)T;
    out[b * D4 + c] = make_float4(r.x * inv, r.y * inv, r.z * inv, r.w * inv);
  }
}

// dy[b,t,:] = g[b,:] / T (fp32, and bf16 if dy_lo); the last blocks of the grid write colsum[d] = sum_b g[b,d]
__global__ __launch_bounds__(256) void token_mean_bwd_kernel(const float4* __restrict__ g, float4* __restrict__ dy,
                                                            bf16* __restrict__ dy_lo, float* __restrict__ colsum, int B,
                                                            int T, int D4, int64_t rows, int main_blocks) {
  // the column-sum blocks come FIRST in the grid (they are one dependent chain of B rows each and would otherwise be the tail of
  // the launch), eight loads in flight; same summation order as before
  const int extra = (int)gridDim.x - main_blocks;
  if ((int)blockIdx.x < extra) {
    const int d = (int)blockIdx.x * 256 + threadIdx.x;
    if (d < 4 * D4) {
      const float* gs = reinterpret_cast<const float*>(g);
      float a = 0.f;
      int b = 0;
      for (; b + 8 <= B; b += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = gs[(int64_t)(b + u) * 4 * D4 + d];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
      }
      for (; b < B; ++b) a += gs[(int64_t)b * 4 * D4 + d];
      colsum[d] = a;
    }
    return;
  }
  const float inv = 1.0f / (float)T;
  const int64_t row0 = (int64_t)((int)blockIdx.x - extra) * TOK_ROWS_PER_BLOCK;
  if (!dy && (D4 & 1) == 0 && ((uintptr_t)dy_lo & 15) == 0) {  // the bf16 image alone (the bf16 gradient stream): 16-byte stores
    const int D8 = D4 >> 1;
    for (int i = threadIdx.x; i < TOK_ROWS_PER_BLOCK * D8; i += 256) {
      const int rr = i / D8, c = i - rr * D8;
      const int64_t row = row0 + rr;
      if (row >= rows) return;
      const float4 v0 = g[(row / T) * D4 + 2 * c], v1 = g[(row / T) * D4 + 2 * c + 1];
      const float o[8] = {v0.x * inv, v0.y * inv, v0.z * inv, v0.w * inv, v1.x * inv, v1.y * inv, v1.z * inv, v1.w * inv};
      *reinterpret_cast<uint4*>(dy_lo + 4 * (row * D4 + 2 * c)) = pack8(o);
    }
    return;
  }
  for (int i = threadIdx.x; i < TOK_ROWS_PER_BLOCK * D4; i += 256) {  // (flat range, as fuse_tokens_kernel)
    const int rr = i / D4, c = i - rr * D4;
    const int64_t row = row0 + rr;
    if (row >= rows) return;
    const float4 v = g[(row / T) * D4 + c];
    const float4 r = make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
    if (dy) dy[row * D4 + c] = r;
    if (dy_lo) store4<bf16>(dy_lo + 4 * (row * D4 + c), r);
  }
}

}  // namespace avf

extern "C" int avf_fuse_tokens(const float* clip, const float* audio, const float* pos, float* out, int batch, int t_video,
                               int t_audio, int dim, void* stream) {
  using namespace avf;
  AVF_REQUIRE(out && batch > 0 && t_video >= 0 && t_audio >= 0 && t_video + t_audio > 0 && (clip || t_video == 0) &&
                  (audio || t_audio == 0) && dim > 0 && dim % 4 == 0,
              "fuse_tokens: bad arguments (dim must be a multiple of 4)");
  AVF_REQUIRE((((uintptr_t)clip | (uintptr_t)audio | (uintptr_t)pos | (uintptr_t)out) & 15) == 0,
              "fuse_tokens: pointers must be 16-byte aligned");
  const int64_t rows = (int64_t)batch * (t_video + t_audio);
  AVF_REQUIRE(ceil_div(rows, TOK_ROWS_PER_BLOCK) < (1LL << 31), "fuse_tokens: too many rows");
  fuse_tokens_kernel<float><<<(unsigned)ceil_div(rows, TOK_ROWS_PER_BLOCK), 256, 0, (hipStream_t)stream>>>(
      (const float4*)clip, (const float4*)audio, (const float4*)pos, out, t_video, t_audio, dim / 4, rows);
  return check_launch("fuse_tokens_kernel");
}

extern "C" int avf_fuse_tokens_bf16(const float* clip, const float* audio, const float* pos, void* out_bf16, int batch,
                                    int t_video, int t_audio, int dim, void* stream) {
  using namespace avf;
  AVF_REQUIRE(out_bf16 && batch > 0 && t_video >= 0 && t_audio >= 0 && t_video + t_audio > 0 && (clip || t_video == 0) &&
                  (audio || t_audio == 0) && dim > 0 && dim % 4 == 0,
              "fuse_tokens_bf16: bad arguments (dim must be a multiple of 4)");
  AVF_REQUIRE((((uintptr_t)clip | (uintptr_t)audio | (uintptr_t)pos) & 15) == 0 && ((uintptr_t)out_bf16 & 7) == 0,
              "fuse_tokens_bf16: misaligned pointers");
  const int64_t rows = (int64_t)batch * (t_video + t_audio);
  AVF_REQUIRE(ceil_div(rows, TOK_ROWS_PER_BLOCK) < (1LL << 31), "fuse_tokens_bf16: too many rows");
  fuse_tokens_kernel<bf16><<<(unsigned)ceil_div(rows, TOK_ROWS_PER_BLOCK), 256, 0, (hipStream_t)stream>>>(
      (const float4*)clip, (const float4*)audio, (const float4*)pos, (bf16*)out_bf16, t_video, t_audio, dim / 4, rows);
  return check_launch("fuse_tokens_kernel");
}

extern "C" int avf_token_mean_fwd(const float* y, float* out, int batch, int tokens, int dim, void* stream) {
  using namespace avf;
  AVF_REQUIRE(y && out && batch > 0 && batch <= 65535 && tokens > 0 && dim > 0 && dim % 4 == 0,
              "token_mean_fwd: bad arguments (dim must be a multiple of 4)");
  AVF_REQUIRE((((uintptr_t)y | (uintptr_t)out) & 15) == 0, "token_mean_fwd: pointers must be 16-byte aligned");
  const int D4 = dim / 4;
  token_mean_fwd_kernel<float><<<dim3((D4 + 15) / 16, batch), 256, 0, (hipStream_t)stream>>>(y, (float4*)out, tokens, D4);
  return check_launch("token_mean_fwd_kernel");
}

extern "C" int avf_token_mean_fwd_bf16(const void* y_bf16, float* out, int batch, int tokens, int dim, void* stream) {
  using namespace avf;
  AVF_REQUIRE(y_bf16 && out && batch > 0 && batch <= 65535 && tokens > 0 && dim > 0 && dim % 4 == 0,
              "token_mean_fwd_bf16: bad arguments (dim must be a multiple of 4)");
  AVF_REQUIRE(((uintptr_t)y_bf16 & 7) == 0 && ((uintptr_t)out & 15) == 0, "token_mean_fwd_bf16: misaligned pointers");
  const int D4 = dim / 4;
  token_mean_fwd_kernel<bf16><<<dim3((D4 + 15) / 16, batch), 256, 0, (hipStream_t)stream>>>((const bf16*)y_bf16, (float4*)out,
                                                                                             tokens, D4);
  return check_launch("token_mean_fwd_kernel");
}

extern "C" int avf_token_mean_bwd(const float* g, float* dy, void* dy_bf16, float* colsum, int batch, int tokens, int dim,
                                  void* stream) {
  using namespace avf;
  AVF_REQUIRE(g && (dy || dy_bf16) && batch > 0 && tokens > 0 && dim > 0 && dim % 4 == 0,
              "token_mean_bwd: bad arguments (dim must be a multiple of 4; one of dy / dy_bf16 is required)");
  AVF_REQUIRE((((uintptr_t)g | (uintptr_t)dy) & 15) == 0 && ((uintptr_t)dy_bf16 & 7) == 0,
              "token_mean_bwd: misaligned pointers");
  const int D4 = dim / 4;
  const int64_t rows = (int64_t)batch * tokens;
  AVF_REQUIRE(ceil_div(rows, TOK_ROWS_PER_BLOCK) < (1LL << 30), "token_mean_bwd: too many rows");
  const int main_blocks = (int)ceil_div(rows, TOK_ROWS_PER_BLOCK);
  const int extra = colsum ? (dim + 255) / 256 : 0;
  token_mean_bwd_kernel<<<main_blocks + extra, 256, 0, (hipStream_t)stream>>>((const float4*)g, (float4*)dy, (bf16*)dy_bf16,
                                                                              colsum, batch, tokens, D4, rows, main_blocks);
  return check_launch("token_mean_bwd_kernel");
}

extern "C" int avf_au_loss(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels,
                           const float* pos_weight, float ignore, int rows, int ncls, float* loss, float* grad_unit,
                           void* stream) {
  using namespace avf;
  AVF_REQUIRE(rows > 0 && ncls > 0 && logits && labels && pos_weight && loss && grad_unit, "au_loss: bad arguments");
  au_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, ld_logits, labels, ld_labels, pos_weight, ignore, rows,
                                                     ncls, loss, grad_unit, 0, ncls);
  return check_launch("au_loss_kernel");
}

extern "C" int avf_au_loss_sum(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels,
                               const float* pos_weight, float ignore, int rows, int ncls, float* sum_count,
                               float* grad_unit, void* stream) {
  using namespace avf;
  AVF_REQUIRE(rows > 0 && ncls > 0 && logits && labels && pos_weight && sum_count && grad_unit, "au_loss_sum: bad arguments");
  au_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, ld_logits, labels, ld_labels, pos_weight, ignore, rows,
                                                     ncls, sum_count, grad_unit, 1, ncls);
  return check_launch("au_loss_kernel");
}

extern "C" int avf_au_loss_wide(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels,
                                const float* pos_weight, float ignore, int rows, int ncls, int width, int sum_mode,
                                float* loss, float* grad_wide, void* stream) {
  using namespace avf;
  AVF_REQUIRE(rows > 0 && ncls > 0 && width >= ncls && logits && labels && pos_weight && loss && grad_wide,
              "au_loss_wide: bad arguments");
  au_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, ld_logits, labels, ld_labels, pos_weight, ignore, rows,
                                                     ncls, loss, grad_wide, sum_mode ? 1 : 0, width);
  return check_launch("au_loss_kernel");
}
