// attn_bf16.hip - throughput-mode attention core: LDS-tiled flash attention forward and backward on
// v_mfma_f32_16x16x32_bf16, fp32 online-softmax statistics, bf16 operands.
//
// Reference: models/heads.py:222-237 (scores * dh^-0.5, softmax over keys, P v, head merge).  The
// [B,H,N,N] score tensor the reference materialises never exists here.  q, k, v are read in place from
// the QKV GEMM output [B*N, 3I] (absorbing 'b n (h d) -> b h n d'), o is written as [B*N, I]
// ('b h n d -> b n (h d)').
//
// Orientation trick (the accumulator of one MFMA is the operand of the next, no LDS round trip):
//   forward / dQ : S^T = K Q^T    -> lane owns a query column; P^T (or dS^T) packs straight into the
//                  B operand of  O^T = V^T P^T  /  dQ^T = K^T dS^T ; V^T / K^T fragments come from
//                  ds_read_b64_tr_b16 on the row-major tile.
//   dK / dV      : S = Q K^T      -> lane owns a key column;  dV^T = dO^T P,  dK^T = Q^T dS.
// (k-slot map of a packed accumulator pair / transposed fragment: mfma_frag.hpp)
// Streaming kernels (attn_{fwd,dq,dkv}_bf16_kernel<DH, NW>): a workgroup owns 128 query (key) rows as NW waves of 128/NW.
// dim_head 32 / 64: NW = 4 (32 rows per wave, two 16-row blocks).  dim_head 128: NW = 8 (16 rows per wave) - with two blocks
// per wave the dK/dV kernel's accumulators alone take 128 registers and all three kernels spill at 256; with one they need
// 150 / 162 / 238 VGPRs (forward / dQ / dK-dV), no scratch, one 512-thread workgroup per CU (73.7 KB static LDS each).
// Rounding points (what tests/attn_bf16_util.py emulates; everything else - scores, running maximum, l, lse2, delta - is fp32):
//   forward   the unnormalised P = exp2(s - m) is rounded to bf16 (round to nearest even: pack_pair) before O^T += V^T P^T;
//             o = acc / l is rounded once.  The head-resident kernel takes l from the MFMA of a ones row with the ROUNDED P,
//             the streaming kernel sums the unrounded P on the VALU.
//   backward  P = exp2(s - lse2) in fp32; dS = P * (dP - delta) from that UNROUNDED P, rounded to bf16 before dQ and dK; P
//             rounded to bf16 before dV; delta = fp32 sum of dO * o over the bf16 o it is given; dq, dk, dv rounded once.
#include <type_traits>

#include "attn_dispatch.hpp"
#include "mfma_frag.hpp"

namespace avf {

namespace {

// 1-D grid of nblk * B*H blocks in the per-XCD order (xcd_remap), so the row blocks of one (batch, head) - which
// share that head's K/V (or Q/dO) - run on one XCD and hit in its L2 instead of re-fetching from HBM.
__device__ __forceinline__ void block_coords(int nblk, int& blk, int& bh) {
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  bh = lid / nblk;
  blk = lid - bh * nblk;
}

// stage ROWS rows x DH bf16 from global (row stride ld elements) into an LDS tile with row stride LD bytes;
// rows >= nvalid are zero-filled.  Split in issue (global -> regs) / commit (regs -> LDS).
template <int DH, int ROWS, int NT = 256>
struct TileStager {
  static constexpr int CPR = DH / 8;                     // 16-byte chunks per row
  static constexpr int PER = (ROWS * CPR + NT - 1) / NT;  // chunks per thread (NT = threads of the workgroup)
  uint4 r[PER];
  __device__ __forceinline__ void issue(const bf16* src, int64_t ld, int row0, int nvalid, int tid) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = tid + NT * i;
      const int row = idx / CPR, c = idx - row * CPR;
      r[i] = make_uint4(0, 0, 0, 0);
      if (idx < ROWS * CPR && row < nvalid) r[i] = *reinterpret_cast<const uint4*>(src + (int64_t)(row0 + row) * ld + c * 8);
    }
  }
  template <int LD>
  __device__ __forceinline__ void commit(char* tile, int tid) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = tid + NT * i;
      const int row = idx / CPR, c = idx - row * CPR;
      if (idx < ROWS * CPR) *reinterpret_cast<uint4*>(tile + row * LD + c * 16) = r[i];
    }
  }
};

// =============================================================================================
// forward
// =============================================================================================
// One row's head columns (DB blocks of 16; a lane holds columns 16 d + 4 lg .. + 3 of every block d) as 16-byte stores: the
// lane groups lg, lg + 1 trade the words of blocks d, d + 1 (v_permlane16_swap), after which an even group holds 8 consecutive
// columns of block d and an odd one 8 of block d + 1.  The partner lane (same row, lg +- 1) must be active: call it under a
// predicate on the ROW only.  (8-byte stores to 16 rows per instruction cost the merged backward kernel 6 %.)
template <int DB, typename Get>
__device__ __forceinline__ void store_row_pairs(bf16* row, int lg, Get&& get) {
  static_assert(DB % 2 == 0, "column blocks come in pairs");
#pragma unroll
  for (int d = 0; d < DB; d += 2) {
    const f32x4_t a = get(d), b = get(d + 1);
    const uint32_t a0 = pack_bf16x2(a[0], a[1]), a1 = pack_bf16x2(a[2], a[3]);
    const uint32_t b0 = pack_bf16x2(b[0], b[1]), b1 = pack_bf16x2(b[2], b[3]);
    const auto s0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
    *reinterpret_cast<uint4*>(row + ((lg & 1) ? (d + 1) * 16 + 4 * (lg - 1) : d * 16 + 4 * lg)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
  }
}

template <int DH, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_fwd_bf16_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o,
                                                                     float* __restrict__ lse2, int /*B*/, int N, int H, int qs) {
  constexpr int KS = DH / 32, DB = DH / 16, QB = 8 / NW;  // 128 query rows per workgroup: NW waves x QB blocks of 16
  constexpr int KLD = DH * 2 + 32;  // K tile: row reads (ds_read_b128); +32 B keeps them conflict-free (PMC-checked)
  constexpr int VLD = DH * 2 + 32;  // V tile: transposed reads, 8 consecutive rows -> 8 distinct bank windows
  constexpr int STAGE = 64 * KLD + 64 * VLD;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  int blk, bh;
  block_coords((N + 127) / 128, blk, bh);
  const int b = bh / H, h = bh - b * H;
  const int I = H * DH;
  const int64_t ld = 3 * (int64_t)I;
  const bf16* qbase = qkv + (int64_t)b * N * ld + h * DH;
  const bf16* kbase = qbase + I;
  const bf16* vbase = qbase + 2 * I;
  const int q0 = blk * 128 + wave * 16 * QB;
  const bool active = __builtin_amdgcn_readfirstlane(q0) < N;
  const float c = qs ? 1.0f : LOG2E / sqrtf((float)DH);  // qs: q already carries log2(e)/sqrt(dh)
  AVF_PHASE_INIT();

  bf16x8_t fq[QB][KS];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int q = q0 + qb * 16 + li;
      fq[qb][ks] = ldg_frag(qbase + (int64_t)q * ld + ks * 32 + 8 * lg, q < N);
    }

  f32x4_t ot[DB][QB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) ot[d][qb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m[QB], lsum[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) m[qb] = -INFINITY, lsum[qb] = 0.f;

  TileStager<DH, 64, 64 * NW> sk, sv;
  const int nt = (N + 63) / 64;
  {
    const int nv = N < 64 ? N : 64;
    sk.issue(kbase, ld, 0, nv, tid);
    sv.issue(vbase, ld, 0, nv, tid);
    sk.template commit<KLD>(smem, tid);
    sv.template commit<VLD>(smem + 64 * KLD, tid);
  }
  __syncthreads();
  AVF_PHASE_MARK(0);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) {
      const int r0 = (t + 1) * 64;
      const int nv = (N - r0) < 64 ? (N - r0) : 64;
      sk.issue(kbase, ld, r0, nv, tid);
      sv.issue(vbase, ld, r0, nv, tid);
    }
    AVF_PHASE_MARK(1);
    const char* kt = smem + cur * STAGE;
    const lds_char* vt = (const lds_char*)(smem + cur * STAGE + 64 * KLD);

    // One K/V tile.  TAIL = the tile holds keys past N: only its valid 16-key blocks are computed and the
    // rest is masked; full tiles take the branch-free instantiation.  Waves whose 32 query rows all lie past N
    // only help with staging and barriers.
    auto tile_body = [&](auto tail_tag) {
      constexpr bool TAIL = decltype(tail_tag)::value;
      const int nkb = TAIL ? (N - t * 64 + 15) / 16 : 4;
      // S^T[key][q] = K Q^T
      f32x4_t st[4][QB];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) st[kb][qb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (!TAIL || kb < nkb) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8_t fk = row_frag<KLD>(kt, kb * 16 + li, ks * 32 + 8 * lg);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
              st[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk, fq[qb][ks], st[kb][qb], 0, 0, 0);
          }
        }
      }
      AVF_PHASE_MARK(2);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        float tmax = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (TAIL && (t * 64 + kb * 16 + 4 * lg + r >= N)) st[kb][qb][r] = -INFINITY;
            tmax = fmaxf(tmax, st[kb][qb][r]);  // raw scores: the scale c > 0 commutes with max
          }
        tmax = groups_max_swap(tmax);
        const float mn = fmaxf(m[qb], tmax * c);
        const float alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
        m[qb] = mn;
        float ps = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pv = __builtin_amdgcn_exp2f(fmaf(st[kb][qb][r], c, -mn));  // 2^(c*s - m): one FMA + exp
            st[kb][qb][r] = pv;
            ps += pv;
          }
        lsum[qb] = lsum[qb] * alpha + ps;
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          ot[d][qb][0] *= alpha; ot[d][qb][1] *= alpha; ot[d][qb][2] *= alpha; ot[d][qb][3] *= alpha;
        }
      }
      AVF_PHASE_MARK(3);
      // O^T[d][q] += V^T P^T
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (TAIL && 2 * s >= nkb) continue;
        bf16x8_t p[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) p[qb] = pack_pair(st[2 * s][qb], st[2 * s + 1][qb]);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          const bf16x8_t fv = tr_frag<VLD>(vt, 32 * s, d * 16, li, lg);
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) ot[d][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, p[qb], ot[d][qb], 0, 0, 0);
        }
      }
    };
    if (active) {
      if (t * 64 + 64 > N) tile_body(std::true_type{});
      else tile_body(std::false_type{});
    }
    AVF_PHASE_MARK(4);
    if (t + 1 < nt) {
      sk.template commit<KLD>(smem + (cur ^ 1) * STAGE, tid);
      sv.template commit<VLD>(smem + (cur ^ 1) * STAGE + 64 * KLD, tid);
    }
    AVF_PHASE_MARK(5);
    __syncthreads();
    AVF_PHASE_MARK(6);
  }

#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    float l = lsum[qb];
    l = groups_sum_swap(l);
    const int q = q0 + qb * 16 + li;
    if (q < N) {
      const float inv = 1.0f / l;
      bf16* orow = o + ((int64_t)b * N + q) * I + h * DH;
      store_row_pairs<DB>(orow, lg, [&](int d) { return ot[d][qb] * inv; });
      if (lg == 0) lse2[(int64_t)bh * N + q] = m[qb] + log2f(l);
    }
  }
  AVF_PHASE_MARK(7);
  AVF_PHASE_FLUSH();
}

// =============================================================================================
// head-resident forward (dim_head 64, N <= RES_MAX_N): ONE workgroup per (batch, head) keeps the head's whole K and
// V in LDS - 128 B per row, N rounded up to 32 rows - so nothing is staged twice, there is no ring and
// no per-tile barrier.  The N rows are cut into V = ceil(N/32) groups of 32 query rows; the workgroup has
// W = ceil(V / passes) wavefronts (passes = ceil(V/12): at most 12 waves, three per SIMD at <= 168 VGPRs) and wave w
// takes groups w, w+W, ...  After the load phase the waves free-run over the key tiles, which lets the MFMA
// phase of one wave overlap the softmax VALU phase of another on the same SIMD.  (The backward has no head-resident
// form: the merged kernel of attn_bwd_merged.hip or the streaming pair below.)
//
// LDS image: written by LDS-DMA (global_load_lds_dwordx4, 64 lanes x 16 B = 8 rows per instruction, no staging
// VGPRs), so it is lane-linear per instruction; bank conflicts are avoided by permuting the SOURCE chunk instead:
// row r holds logical 16-B chunk c at slot c ^ res_swz(r), res_swz(r) = ((r>>1)&3)<<1.  That is conflict-free
// (SQ_LDS_BANK_CONFLICT = 0) for the ds_read_b128 row fragments (lane groups of 16: rows x two adjacent chunks) and
// for ds_read_b64_tr_b16 (lane groups of 32: 8 consecutive rows x two adjacent chunks).  Rows past N are loaded
// from row N-1 (finite values; their probabilities are exactly 0).
// Arrival: two barriers only - after the first RES_A tiles have landed, and after everything has (see ResLoader).
// Forward softmax: running maximum with LAZY rescaling - the accumulators are rescaled only when some row's maximum
// grew by more than 2^RES_TAU since the last rescale (a wave-uniform branch, rare after the first tile), so
// probabilities stay <= 2^RES_TAU; the row sums come from the MFMA (a ones fragment as a 65th value row), the
// cross-lane maximum from v_permlane{16,32}_swap instead of LDS permutes.  lse2 = m + log2(l) is exact whatever m is.
// =============================================================================================
constexpr int RES_MAX_N = 576;    // (N rounded to 32) * 256 B of K and V images = 144 KB of the 160 KB
constexpr int RES_A = 1;          // tiles whose DMA is issued before any compute (2 gave the same forward time)
constexpr float RES_TAU = 6.0f;   // log2 of the largest probability kept before a rescale

// The DMA of the head-resident forward is the asm form (glds16_asm; mfma_frag.hpp says why): with the builtin the pieces
// fed from hooks inside the first tile's compute cost a full memory round trip each.
__device__ __forceinline__ void res_dma16(const void* g, char* l) { glds16_asm(g, l); }

__device__ __forceinline__ bf16x8_t ones_frag() {
  u32x4_t r = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
  return __builtin_bit_cast(bf16x8_t, r);
}

// DMA schedule of a head-resident kernel.  Two [rows, 64] bf16 operands a, b (row strides lda, ldb elements) go to
// their LDS images in 8-row pieces, ordered a0 b0 a1 b1 ... (16 pieces per 64-row tile, so arrival is in tile order);
// piece p belongs to wave p mod W and each wave walks its pieces with a cursor.  Phase 1 (the first RES_A tiles) is
// issued up front; the rest is issued one piece at a time from hooks inside the first tile's compute, so no wave sits
// in a full memory queue while the SIMD idles; the second barrier (after the RES_A-th tile) waits for what is left.
struct ResLoader {
  const bf16 *a, *b;
  int64_t lda, ldb;
  char *la, *lb;
  int npieces, N, W, lrow, chunk, cur;
  __device__ __forceinline__ void init(const bf16* a_, int64_t lda_, char* la_, const bf16* b_, int64_t ldb_, char* lb_,
                                       int rows_padded, int N_, int wave, int W_, int lane) {
    a = a_; b = b_; lda = lda_; ldb = ldb_; la = la_; lb = lb_;
    npieces = rows_padded / 4;  // 2 operands x rows/8
    N = N_; W = W_; cur = wave;
    lrow = lane >> 3;
    chunk = (lane & 7) ^ (((lrow >> 1) & 3) << 1);
  }
  __device__ __forceinline__ void issue_one() {  // wave-uniform; no-op once the wave's pieces are out
    if (cur < npieces) {
      const int i = cur >> 1;
      int row = i * 8 + lrow;
      row = row < N ? row : N - 1;
      if (cur & 1) res_dma16(b + (int64_t)row * ldb + chunk * 8, lb + i * 1024);
      else res_dma16(a + (int64_t)row * lda + chunk * 8, la + i * 1024);
      cur += W;
    }
  }
  __device__ __forceinline__ void issue_until(int limit) {
    const int lim = limit < npieces ? limit : npieces;
    while (cur < lim) issue_one();
  }
};

// per-lane byte offsets inside a 64-row tile of an LDS image: row[ks] for the ds_read_b128 row fragment of row
// block kb (add kb*2048), tr[d] for the transposed fragment of 32-row k-step s2 (add s2*4096)
struct ResOffsets {
  int row[2], tr[4];
  __device__ __forceinline__ void init(int li, int lg) {
    const int swz_r = ((li >> 1) & 3) << 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) row[ks] = li * 128 + (((ks * 4 + lg) ^ swz_r) << 4);
    const int swz_t = ((2 * lg + (li >> 3)) & 3) << 1;
#pragma unroll
    for (int d = 0; d < 4; ++d)
      tr[d] = (4 * lg + (li >> 2)) * 128 + (((2 * d + ((li & 3) >> 1)) ^ swz_t) << 4) + (li & 1) * 8;
  }
};

// Tile schedule of the head-resident forward: pass 0 of every wave gates on the two arrival barriers and feeds the
// remaining DMA from its first tile; later passes (more 32-row groups than waves) run without any synchronisation.
template <bool MULTI, typename TileFn, typename SyncFn>
__device__ __forceinline__ void res_sweep(int N, bool first, TileFn&& tile, SyncFn&& sync) {
  const int nt = (N + 63) / 64, nfull = N / 64;
  const bool first_pass = !MULTI || first;  // single-pass kernels: known at compile time
  int t0 = 0;
  if (first_pass) {
    sync();  // the first RES_A tiles are visible
    if (nfull > 0) tile(0, std::false_type{}, std::true_type{});
    else tile(0, std::true_type{}, std::true_type{});
    t0 = nt < RES_A ? nt : RES_A;
    for (int t = 1; t < t0; ++t) {
      if (t < nfull) tile(t, std::false_type{}, std::false_type{});
      else tile(t, std::true_type{}, std::false_type{});
    }
    if (nt > RES_A) sync();  // everything is visible
  }
  for (int t = t0; t < nfull; ++t) tile(t, std::false_type{}, std::false_type{});  // the hot loop: one variant only
  if (nfull < nt && t0 <= nfull) tile(nfull, std::true_type{}, std::false_type{});
}

// MULTI: more 32-row groups than waves (each wave loops over its groups); otherwise exactly one group per wave.
// QS: the q columns already carry log2(e)/sqrt(dh) (layer path) - the scores leave the MFMA in the log2 domain, and the
// subtraction of the running maximum rides in the MFMA's C operand: no per-score FMA.
// MASKED (QS only): the token mask of heads.py:225-232 - keep[b][n] != 0 keeps token n.  A pair (query, key) with either
// token dropped scores -FLT_MAX in the reference: a kept query gives dropped keys zero weight (score -inf here), a dropped
// query's row is one constant, i.e. uniform attention over ALL its keys (score 0 here: lse2 = log2 N exactly, which the
// backward kernel relies on).  The flags of the clip's keys sit in LDS behind the V image.
template <int MAXW, bool MULTI, bool QS, bool MASKED = false>
__global__ __launch_bounds__(MAXW * 64) void attn_fwd_res_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o,
                                                                float* __restrict__ lse2, int N, int H,
                                                                uint8_t* __restrict__ oq = nullptr,
                                                                uint8_t* __restrict__ osc = nullptr,
                                                                const uint8_t* __restrict__ keep = nullptr) {
  static_assert(!MASKED || QS, "the masked form exists for pre-scaled queries only");
  constexpr int DH = 64, KS = 2, DB = 4;
  extern __shared__ __attribute__((aligned(16))) char res_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = blockDim.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int I = H * DH;
  const int64_t ld = 3 * (int64_t)I;
  const bf16* qbase = qkv + (int64_t)b * N * ld + h * DH;
  const bf16* kbase = qbase + I;
  const bf16* vbase = qbase + 2 * I;
  const int NP = (N + 31) & ~31, V = NP >> 5;
  char* ksm = res_smem;
  char* vsm = res_smem + NP * 128;
  const float c = LOG2E / sqrtf((float)DH);
  AVF_PHASE_INIT();
  ResLoader loader;
  loader.init(kbase, ld, ksm, vbase, ld, vsm, NP, N, wave, W, lane);
  ResOffsets off;
  off.init(li, lg);
  const bf16x8_t ones = ones_frag();
  const uint8_t* keepl = reinterpret_cast<const uint8_t*>(res_smem + 2 * NP * 128);  // MASKED: [ceil64(N)] key flags
  if constexpr (MASKED) {
    uint8_t* kw = reinterpret_cast<uint8_t*>(res_smem + 2 * NP * 128);
    for (int i = tid; i < ((N + 63) & ~63); i += blockDim.x) kw[i] = i < N ? keep[(int64_t)b * N + i] : (uint8_t)0;
    wait_lgkmcnt<0>();  // (the first arrival barrier of the sweep publishes them)
  }

  int grp = wave;
  do {
    const bool first_pass = !MULTI || grp == wave;
    const int q0 = grp * 32;
    bool qkeep[2] = {true, true};  // MASKED: is this lane's query row a kept token
    bool cen[2] = {false, false};  // MASKED: has the row's running maximum been centred on a finite score yet
    if constexpr (MASKED) {
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        const int q = q0 + qb * 16 + li;
        qkeep[qb] = q < N ? keep[(int64_t)b * N + q] != 0 : true;
      }
    }
    bf16x8_t fq[2][KS];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int q = q0 + qb * 16 + li;
        fq[qb][ks] = ldg_frag(qbase + (int64_t)q * ld + ks * 32 + 8 * lg, q < N);
      }
    if (first_pass) loader.issue_until(16 * RES_A);

    f32x4_t ot[DB][2], ls[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      ls[qb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int d = 0; d < DB; ++d) ot[d][qb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    float m[2] = {QS ? 0.f : -INFINITY, QS ? 0.f : -INFINITY};
    f32x4_t minit[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // QS: -m, the C operand of the first score MFMA
    bool first_tile = true;                                              // QS: the first tile centres m on its maximum

    auto tile = [&](int t, auto tail_tag, auto feed_tag) {
      constexpr bool TAIL = decltype(tail_tag)::value;
      constexpr bool FEED = decltype(feed_tag)::value;  // this tile also issues the remaining DMA pieces
      const int nkb = TAIL ? (N - t * 64 + 15) / 16 : 4;
      const char* kt = ksm + t * 8192;
      const char* vt = vsm + t * 8192;
      f32x4_t st[4][2];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        st[kb][0] = QS ? minit[0] : f32x4_t{0.f, 0.f, 0.f, 0.f};
        st[kb][1] = QS ? minit[1] : f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (!TAIL || kb < nkb) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8_t fk = row_frag(kt + kb * 2048 + off.row[ks]);
            st[kb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk, fq[0][ks], st[kb][0], 0, 0, 0);
            st[kb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk, fq[1][ks], st[kb][1], 0, 0, 0);
          }
        }
        if (FEED) loader.issue_one();
      }
      AVF_PHASE_MARK(2);
      // 8-wave builds (two waves per SIMD, registers to spare): the V fragments of the first k-step are requested BEFORE
      // the softmax and those of the second one before the first k-step's MFMAs, so the transposed LDS reads land under
      // VALU / MFMA work instead of in front of the PV MFMAs (stamps: the PV section was 1100 cycles per tile for 20 MFMAs)
      constexpr bool VPF = MAXW == 8;
      bf16x8_t fvp[2][DB];
      if constexpr (VPF) {
        if (!TAIL || nkb > 0) {
#pragma unroll
          for (int d = 0; d < DB; ++d) fvp[0][d] = tr_frag<128>((const lds_char*)(vt + off.tr[d]));
        }
      }
      if constexpr (QS) {
        // st = log2-domain score - m.  Re-centre when a row maximum exceeds m by more than RES_TAU (and always on the
        // first tile, which fixes m): only then are the accumulators and this tile's scores shifted.
        float cm[2];
        bool grow = MASKED ? false : first_tile;
        uint32_t kflag[4] = {0u, 0u, 0u, 0u};
        if constexpr (MASKED) {
#pragma unroll
          for (int kb = 0; kb < 4; ++kb) kflag[kb] = *reinterpret_cast<const uint32_t*>(keepl + t * 64 + kb * 16 + 4 * lg);
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          float tmax = -INFINITY;
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if constexpr (MASKED) {
                const bool kk = ((kflag[kb] >> (8 * r)) & 255u) != 0;  // (rows past N carry flag 0)
                const bool real = !TAIL || (t * 64 + kb * 16 + 4 * lg + r < N);
                st[kb][qb][r] = qkeep[qb] ? (kk ? st[kb][qb][r] : -INFINITY) : (real ? -m[qb] : -INFINITY);
              } else {
                if (TAIL && (t * 64 + kb * 16 + 4 * lg + r >= N)) st[kb][qb][r] = -INFINITY;
              }
              tmax = fmaxf(tmax, st[kb][qb][r]);
            }
          cm[qb] = groups_max_swap(tmax);
          if constexpr (MASKED) grow = grow || (cen[qb] ? cm[qb] > RES_TAU : cm[qb] > -1.0e30f);  // (a tile may hold no kept key)
          else grow = grow || (cm[qb] > RES_TAU);
        }
        if (__builtin_amdgcn_ballot_w64(grow) != 0) {  // wave-uniform
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) {
            float shift, alpha;
            if constexpr (MASKED) {
              // a row is centred on its first tile with a finite score (any sign); its accumulators are 0 until then
              const bool fin = cm[qb] > -1.0e30f;
              shift = cen[qb] ? fmaxf(cm[qb], 0.f) : (fin ? cm[qb] : 0.f);
              alpha = cen[qb] ? __builtin_amdgcn_exp2f(-shift) : 1.0f;
              cen[qb] = cen[qb] || fin;
            } else {
              shift = first_tile ? cm[qb] : fmaxf(cm[qb], 0.f);
              alpha = first_tile ? 1.0f : __builtin_amdgcn_exp2f(-shift);  // accumulators are 0 on the first tile
            }
            m[qb] += shift;
            minit[qb] = f32x4_t{-m[qb], -m[qb], -m[qb], -m[qb]};
            ls[qb][0] *= alpha; ls[qb][1] *= alpha; ls[qb][2] *= alpha; ls[qb][3] *= alpha;
#pragma unroll
            for (int d = 0; d < DB; ++d) {
              ot[d][qb][0] *= alpha; ot[d][qb][1] *= alpha; ot[d][qb][2] *= alpha; ot[d][qb][3] *= alpha;
            }
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
              for (int r = 0; r < 4; ++r) st[kb][qb][r] -= shift;
          }
        }
        first_tile = false;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[kb][qb][r] = __builtin_amdgcn_exp2f(st[kb][qb][r]);
      } else {
      float cand[2];
      bool grow = false;
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        float tmax = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (TAIL && (t * 64 + kb * 16 + 4 * lg + r >= N)) st[kb][qb][r] = -INFINITY;
            tmax = fmaxf(tmax, st[kb][qb][r]);
          }
        cand[qb] = groups_max_swap(tmax) * c;
        grow = grow || (cand[qb] > m[qb] + RES_TAU);
      }
      if (__builtin_amdgcn_ballot_w64(grow) != 0) {  // wave-uniform
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          const float mn = fmaxf(m[qb], cand[qb]);
          const float alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
          m[qb] = mn;
          ls[qb][0] *= alpha; ls[qb][1] *= alpha; ls[qb][2] *= alpha; ls[qb][3] *= alpha;
#pragma unroll
          for (int d = 0; d < DB; ++d) {
            ot[d][qb][0] *= alpha; ot[d][qb][1] *= alpha; ot[d][qb][2] *= alpha; ot[d][qb][3] *= alpha;
          }
        }
      }
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) st[kb][qb][r] = __builtin_amdgcn_exp2f(fmaf(st[kb][qb][r], c, -m[qb]));
      }
      AVF_PHASE_MARK(3);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if (TAIL && 2 * s2 >= nkb) continue;
        if constexpr (!VPF) __builtin_amdgcn_sched_barrier(0);  // keep the V fragments of this k-step from being hoisted over the softmax
        const bf16x8_t p0 = pack_pair(st[2 * s2][0], st[2 * s2 + 1][0]);
        const bf16x8_t p1 = pack_pair(st[2 * s2][1], st[2 * s2 + 1][1]);
        if constexpr (VPF) {
          if (s2 == 0 && (!TAIL || nkb > 2)) {
#pragma unroll
            for (int d = 0; d < DB; ++d) fvp[1][d] = tr_frag<128>((const lds_char*)(vt + 4096 + off.tr[d]));
          }
        }
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          bf16x8_t fv;
          if constexpr (VPF) fv = fvp[s2][d];
          else fv = tr_frag<128>((const lds_char*)(vt + s2 * 4096 + off.tr[d]));
          ot[d][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, p0, ot[d][0], 0, 0, 0);
          ot[d][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, p1, ot[d][1], 0, 0, 0);
        }
        ls[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, p0, ls[0], 0, 0, 0);
        ls[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, p1, ls[1], 0, 0, 0);
        if (FEED) loader.issue_one();
      }
      if (FEED) loader.issue_until(1 << 30);
      AVF_PHASE_MARK(4);
    };
    AVF_PHASE_MARK(1);
    res_sweep<MULTI>(N, first_pass, tile, [&] {
      wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      AVF_PHASE_MARK(0);
    });

#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int q = q0 + qb * 16 + li;
      const float l = ls[qb][0];
      const float inv = 1.0f / l;
      {
        // lane groups lg, lg + 1 trade the words of column blocks d, d + 1 (v_permlane16_swap, all lanes active): an even
        // group then holds 8 consecutive columns of block d, an odd one 8 of block d + 1 - 16-byte stores
        bf16* orow = o + ((int64_t)b * N + (q < N ? q : N - 1)) * I + h * DH;
#pragma unroll
        for (int d = 0; d < DB; d += 2) {
          const uint32_t a0 = pack_bf16x2(ot[d][qb][0] * inv, ot[d][qb][1] * inv), a1 = pack_bf16x2(ot[d][qb][2] * inv, ot[d][qb][3] * inv);
          const uint32_t b0 = pack_bf16x2(ot[d + 1][qb][0] * inv, ot[d + 1][qb][1] * inv),
                         b1 = pack_bf16x2(ot[d + 1][qb][2] * inv, ot[d + 1][qb][3] * inv);
          const auto s0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
          if (q < N)
            store_out16(orow + ((lg & 1) ? (d + 1) * 16 + 4 * (lg - 1) : d * 16 + 4 * lg), make_uint4(s0[0], s1[0], s0[1], s1[1]));
        }
        if (q < N && lg == 0) store_out4(lse2 + (int64_t)bh * N + q, m[qb] + log2f(l));
      }
      if (oq) {  // wave-uniform: MX-FP8 image of the output rows (A operand of the out-projection in the fp8 mode); a
                 // 32-block of the head's 64 columns is two 16-column blocks x the 4 lane groups x 4 registers
        // A lane holds columns 16 d + 4 lg .. + 3 of its row for d = 0..3: one dword of the image each, 16 bytes apart.  A
        // 4 x 4 transpose between the register index d and the lane group lg (tr4x4) leaves lane group lg with the 16
        // contiguous bytes of column block d = lg: one 16-byte store (64-byte row segments per instruction; 67.6 -> 65.7 us
        // at B = 64, N = 512 against per-dword stores.  The same transpose on the bf16 output itself measured +2 %: not used)
        const int64_t row = (int64_t)b * N + (q < N ? q : N - 1);
        uint32_t qw[DB], sb[2];
        float vb[DB][4];
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
          for (int r = 0; r < 4; ++r) vb[d][r] = to_f32<bf16>(from_f32<bf16>(ot[d][qb][r] * inv));  // image of the STORED values
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
          float am = 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) am = fmaxf(am, fmaxf(fabsf(vb[2 * blk][r]), fabsf(vb[2 * blk + 1][r])));
          am = groups_max_shfl(am);
          float sinv;
          sb[blk] = mx8_scale_byte(am, &sinv);
          qw[2 * blk] = mx8_pack4(vb[2 * blk], sinv);
          qw[2 * blk + 1] = mx8_pack4(vb[2 * blk + 1], sinv);
        }
        tr4x4(qw);  // lane group lg: bytes 16 lg .. 16 lg + 15 of the head's 64
        if (q < N) {
          *reinterpret_cast<uint4*>(oq + row * I + h * DH + lg * 16) = make_uint4(qw[0], qw[1], qw[2], qw[3]);
          if (lg == 0) *reinterpret_cast<uint16_t*>(osc + row * (I >> 5) + h * 2) = (uint16_t)(sb[0] | (sb[1] << 8));
        }
      }
    }
    AVF_PHASE_MARK(7);
  } while (MULTI && (grp += W) < V);
  AVF_PHASE_FLUSH();
}

// =============================================================================================
// backward: dQ  (query on the lane; sweeps key tiles)
// =============================================================================================
template <int DH, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_dq_bf16_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ d_o,
                                                                    const float* __restrict__ lse2,
                                                                    const float* __restrict__ delta, bf16* __restrict__ dqkv,
                                                                    int /*B*/, int N, int H, int qs) {
  constexpr int KS = DH / 32, DB = DH / 16, QB = 8 / NW;  // 128 query rows per workgroup: NW waves x QB blocks of 16
  constexpr int KLD = DH * 2 + 32;  // K tile: row reads AND transposed reads
  constexpr int VLD = DH * 2 + 32;  // V tile: row reads only (+32 B: conflict-free, PMC-checked)
  constexpr int STAGE = 64 * KLD + 64 * VLD;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  int blk, bh;
  block_coords((N + 127) / 128, blk, bh);
  const int b = bh / H, h = bh - b * H;
  const int I = H * DH;
  const int64_t ld = 3 * (int64_t)I;
  const bf16* qbase = qkv + (int64_t)b * N * ld + h * DH;
  const bf16* kbase = qbase + I;
  const bf16* vbase = qbase + 2 * I;
  const bf16* gbase = d_o + (int64_t)b * N * I + h * DH;
  const int q0 = blk * 128 + wave * 16 * QB;
  const bool active = __builtin_amdgcn_readfirstlane(q0) < N;
  const float scale = 1.0f / sqrtf((float)DH);
  const float c = qs ? 1.0f : LOG2E * scale;

  bf16x8_t fq[QB][KS], fg[QB][KS];
  float L[QB], dl[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int q = q0 + qb * 16 + li;
    const bool ok = q < N;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      fq[qb][ks] = ldg_frag(qbase + (int64_t)q * ld + ks * 32 + 8 * lg, ok);
      fg[qb][ks] = ldg_frag(gbase + (int64_t)q * I + ks * 32 + 8 * lg, ok);
    }
    L[qb] = ok ? lse2[(int64_t)bh * N + q] : 0.f;
    dl[qb] = ok ? delta[(int64_t)bh * N + q] : 0.f;
  }
  f32x4_t dqt[DB][QB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) dqt[d][qb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  TileStager<DH, 64, 64 * NW> sk, sv;
  const int nt = (N + 63) / 64;
  {
    const int nv = N < 64 ? N : 64;
    sk.issue(kbase, ld, 0, nv, tid);
    sv.issue(vbase, ld, 0, nv, tid);
    sk.template commit<KLD>(smem, tid);
    sv.template commit<VLD>(smem + 64 * KLD, tid);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) {
      const int r0 = (t + 1) * 64;
      const int nv = (N - r0) < 64 ? (N - r0) : 64;
      sk.issue(kbase, ld, r0, nv, tid);
      sv.issue(vbase, ld, r0, nv, tid);
    }
    const char* kt = smem + cur * STAGE;
    const char* vt = smem + cur * STAGE + 64 * KLD;
    auto tile_body = [&](auto tail_tag) {
      constexpr bool TAIL = decltype(tail_tag)::value;
      const int nkb = TAIL ? (N - t * 64 + 15) / 16 : 4;
      f32x4_t ds[4][QB];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) ds[kb][qb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (TAIL && kb >= nkb) continue;
        f32x4_t sc[QB], pg[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) sc[qb] = pg[qb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8_t fk = row_frag<KLD>(kt, kb * 16 + li, ks * 32 + 8 * lg);
          const bf16x8_t fv = row_frag<VLD>(vt, kb * 16 + li, ks * 32 + 8 * lg);
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) sc[qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk, fq[qb][ks], sc[qb], 0, 0, 0);
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) pg[qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, fg[qb][ks], pg[qb], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool dead = TAIL && (t * 64 + kb * 16 + 4 * lg + r >= N);
          float e[QB];
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) e[qb] = dead ? 0.f : __builtin_amdgcn_exp2f(sc[qb][r] * c - L[qb]);
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) ds[kb][qb][r] = e[qb] * (pg[qb][r] - dl[qb]);
        }
      }
      // dQ^T[d][q] += K^T dS^T
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (TAIL && 2 * s >= nkb) continue;
        bf16x8_t a[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) a[qb] = pack_pair(ds[2 * s][qb], ds[2 * s + 1][qb]);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          const bf16x8_t fkt = tr_frag<KLD>((const lds_char*)kt, 32 * s, d * 16, li, lg);
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) dqt[d][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fkt, a[qb], dqt[d][qb], 0, 0, 0);
        }
      }
    };
    if (active) {
      if (t * 64 + 64 > N) tile_body(std::true_type{});
      else tile_body(std::false_type{});
    }
    if (t + 1 < nt) {
      sk.template commit<KLD>(smem + (cur ^ 1) * STAGE, tid);
      sv.template commit<VLD>(smem + (cur ^ 1) * STAGE + 64 * KLD, tid);
    }
    __syncthreads();
  }
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int q = q0 + qb * 16 + li;
    if (q < N) {
      bf16* out = dqkv + ((int64_t)b * N + q) * ld + h * DH;
store_row_pairs<DB>(out, lg, [&](int d) { return dqt[d][qb] * scale; });
    }
  }
}

// =============================================================================================
// backward: dK, dV  (key on the lane; sweeps query tiles)
// =============================================================================================
template <int DH, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_dkv_bf16_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ d_o,
                                                                     const float* __restrict__ lse2,
                                                                     const float* __restrict__ delta, bf16* __restrict__ dqkv,
                                                                     int /*B*/, int N, int H, int qs) {
  constexpr int KS = DH / 32, DB = DH / 16, KB = 8 / NW;  // 128 key rows per workgroup: NW waves x KB blocks of 16
  constexpr int TLD = DH * 2 + 32;  // Q and dO tiles: row reads AND transposed reads
  constexpr int STAGE = 2 * 64 * TLD + 2 * 64 * 4;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  int blk, bh;
  block_coords((N + 127) / 128, blk, bh);
  const int b = bh / H, h = bh - b * H;
  const int I = H * DH;
  const int64_t ld = 3 * (int64_t)I;
  const bf16* qbase = qkv + (int64_t)b * N * ld + h * DH;
  const bf16* kbase = qbase + I;
  const bf16* vbase = qbase + 2 * I;
  const bf16* gbase = d_o + (int64_t)b * N * I + h * DH;
  const int k0 = blk * 128 + wave * 16 * KB;
  const bool active = __builtin_amdgcn_readfirstlane(k0) < N;
  const float scale = 1.0f / sqrtf((float)DH);
  const float c = qs ? 1.0f : LOG2E * scale;
  const float kscale = qs ? 1.0f / LOG2E : scale;  // dK = scale dS^T q = dS^T q' / log2(e) when q' = q log2(e) scale

  bf16x8_t fk[KB][KS], fv[KB][KS];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int key = k0 + kb * 16 + li;
      fk[kb][ks] = ldg_frag(kbase + (int64_t)key * ld + ks * 32 + 8 * lg, key < N);
      fv[kb][ks] = ldg_frag(vbase + (int64_t)key * ld + ks * 32 + 8 * lg, key < N);
    }
  f32x4_t dvt[DB][KB], dkt[DB][KB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      dvt[d][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      dkt[d][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }

  TileStager<DH, 64, 64 * NW> sq, sg;
  float rl = 0.f, rd = 0.f;  // staged lse2 / delta (threads 0..63)
  auto issue_stats = [&](int r0) {
    if (tid < 64) {
      const bool ok = r0 + tid < N;
      rl = ok ? lse2[(int64_t)bh * N + r0 + tid] : INFINITY;  // 2^(x - inf) = 0 for padded queries
      rd = ok ? delta[(int64_t)bh * N + r0 + tid] : 0.f;
    }
  };
  auto commit_stats = [&](char* stage) {
    if (tid < 64) {
      reinterpret_cast<float*>(stage + 2 * 64 * TLD)[tid] = rl;
      reinterpret_cast<float*>(stage + 2 * 64 * TLD + 256)[tid] = rd;
    }
  };
  const int nt = (N + 63) / 64;
  {
    const int nv = N < 64 ? N : 64;
    sq.issue(qbase, ld, 0, nv, tid);
    sg.issue(gbase, I, 0, nv, tid);
    issue_stats(0);
    sq.template commit<TLD>(smem, tid);
    sg.template commit<TLD>(smem + 64 * TLD, tid);
    commit_stats(smem);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) {
      const int r0 = (t + 1) * 64;
      const int nv = (N - r0) < 64 ? (N - r0) : 64;
      sq.issue(qbase, ld, r0, nv, tid);
      sg.issue(gbase, I, r0, nv, tid);
      issue_stats(r0);
    }
    const char* qt = smem + cur * STAGE;
    const char* gt = qt + 64 * TLD;
    const float* Ls = reinterpret_cast<const float*>(qt + 2 * 64 * TLD);
    const float* Ds = Ls + 64;

    // One Q/dO tile, processed as two 32-query k-steps so that only one pair of P / dS blocks is live at a time
    // (keeps the kernel under 256 registers -> two waves per SIMD).
    auto tile_body = [&](auto tail_tag) {
      constexpr bool TAIL = decltype(tail_tag)::value;
      const int nqb = TAIL ? (N - t * 64 + 15) / 16 : 4;  // 16-query blocks with valid rows
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (TAIL && 2 * s >= nqb) continue;
        f32x4_t pm[2][KB], dsm[2][KB];  // P and dS, [q-block of the pair][key-block]
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const int qb = 2 * s + h2;
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) pm[h2][kb] = dsm[h2][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          if (TAIL && qb >= nqb) continue;
          f32x4_t sc[KB], pg[KB];
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) sc[kb] = pg[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8_t fqr = row_frag<TLD>(qt, qb * 16 + li, ks * 32 + 8 * lg);
            const bf16x8_t fgr = row_frag<TLD>(gt, qb * 16 + li, ks * 32 + 8 * lg);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) sc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fqr, fk[kb][ks], sc[kb], 0, 0, 0);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) pg[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fgr, fv[kb][ks], pg[kb], 0, 0, 0);
          }
          const float4 l4 = *reinterpret_cast<const float4*>(Ls + qb * 16 + 4 * lg);
          const float4 d4 = *reinterpret_cast<const float4*>(Ds + qb * 16 + 4 * lg);
          const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float e[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) e[kb] = __builtin_amdgcn_exp2f(sc[kb][r] * c - lv[r]);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) pm[h2][kb][r] = e[kb];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) dsm[h2][kb][r] = e[kb] * (pg[kb][r] - dv[r]);
          }
        }
        // dV^T[d][key] += dO^T P ; dK^T[d][key] += Q^T dS
        bf16x8_t pa[KB], da[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) pa[kb] = pack_pair(pm[0][kb], pm[1][kb]);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) da[kb] = pack_pair(dsm[0][kb], dsm[1][kb]);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          const bf16x8_t fgt = tr_frag<TLD>((const lds_char*)gt, 32 * s, d * 16, li, lg);
          const bf16x8_t fqt = tr_frag<TLD>((const lds_char*)qt, 32 * s, d * 16, li, lg);
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) dvt[d][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fgt, pa[kb], dvt[d][kb], 0, 0, 0);
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) dkt[d][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fqt, da[kb], dkt[d][kb], 0, 0, 0);
        }
      }
    };
    if (active) {
      if (t * 64 + 64 > N) tile_body(std::true_type{});
      else tile_body(std::false_type{});
    }
    if (t + 1 < nt) {
      char* nx = smem + (cur ^ 1) * STAGE;
      sq.template commit<TLD>(nx, tid);
      sg.template commit<TLD>(nx + 64 * TLD, tid);
      commit_stats(nx);
    }
    __syncthreads();
  }
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int key = k0 + kb * 16 + li;
    if (key < N) {
      bf16* outk = dqkv + ((int64_t)b * N + key) * ld + I + h * DH;
      bf16* outv = outk + I;
store_row_pairs<DB>(outk, lg, [&](int d) { return dkt[d][kb] * kscale; });
        store_row_pairs<DB>(outv, lg, [&](int d) { return dvt[d][kb]; });
    }
  }
}

}  // namespace

namespace {
// head-resident kernels: dim_head 64, the head's two operands fit in LDS
bool use_resident(int N, int dh) { return dh == 64 && N <= RES_MAX_N; }

// The head-resident variant for N tokens.  V = ceil(N/32) row groups: up to 8 take the 8-wave kernel and 9 .. 12 the 12-wave
// one, a wave per row group in a single pass; more are spread over ceil(V/8) passes of the 8-wave multi-pass kernel.
// -> ATTN_RES8 | ATTN_RES12 | ATTN_RES_MULTI, *W: waves per workgroup
int res_variant(int N, int* W) {
  const int V = (int)ceil_div(N, 32);
  if (V > 12) {
    *W = (int)ceil_div(V, ceil_div(V, 8));
    return ATTN_RES_MULTI;
  }
  *W = V;
  return V <= 8 ? ATTN_RES8 : ATTN_RES12;
}
// f(int_c<MAXW>{}, std::bool_constant<MULTI>{}, waves per workgroup)
template <typename F>
int with_res_variant(int N, F&& f) {
  int W = 0;
  switch (res_variant(N, &W)) {
    case ATTN_RES_MULTI: return f(int_c<8>{}, std::true_type{}, W);
    case ATTN_RES8: return f(int_c<8>{}, std::false_type{}, W);
    default: return f(int_c<12>{}, std::false_type{}, W);
  }
}
// ... as check_launch and the error messages name it behind the kernel's name: "<8,multi,qs,mask>"
template <int MAXW, bool MULTI, bool QS, bool MASKED = false>
constexpr const char* res_tag() {
  if constexpr (MAXW == 12) return MASKED ? "<12,qs,mask>" : QS ? "<12,qs>" : "<12>";
  else if constexpr (MULTI) return MASKED ? "<8,multi,qs,mask>" : QS ? "<8,multi,qs>" : "<8,multi>";
  else return MASKED ? "<8,qs,mask>" : QS ? "<8,qs>" : "<8>";
}

template <auto Kernel, typename... Args>
int res_launch(const TimingScope* ts, const char* family, const char* tag, int blocks, int waves, size_t smem, hipStream_t s,
               Args... args) {
  static const struct Name {  // "attn_fwd_res<8,multi,qs>"
    char str[48];
    Name(const char* f, const char* t) { snprintf(str, sizeof str, "%s%s", f, t); }
  } name(family, tag);
  static PerDeviceOnce once;  // the dynamic-LDS limit, raised once per kernel and device
  if (once.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    AVF_REQUIRE(e == hipSuccess, "%s: cannot raise dynamic LDS limit: %s", name.str, hipGetErrorString(e));
    once.mark();
  }
  AVF_REQUIRE(smem <= 160 * 1024, "%s: %zu bytes of LDS", name.str, smem);
  launch_in_scope(ts, Kernel, dim3(blocks), dim3(waves * 64), (uint32_t)smem, s, args...);
  return check_launch(name.str);
}
}  // namespace

// log2(e)/sqrt(dh): the factor the layer path folds into the query rows of its bf16 Wqkv image
float attn_q_prescale(int dh) { return LOG2E / sqrtf((float)dh); }

// the head-resident forward kernel can also write the MX-FP8 image of its output
bool attn_fwd_emits_mx8(int N, int dh) { return use_resident(N, dh); }

bool attn_masked_bf16_ok(int N, int dh, bool q_prescaled) {
  static const int on = tuning_int("AVF_ATTN_MASK_MFMA", 1);  // A/B aid: 0 = every masked call on the fp32-arithmetic kernels
  return on && q_prescaled && use_resident(N, dh) && N >= 1 && N <= 512;
}

// the kernel attn_fwd_bf16 launches (it switches on this value): a head-resident variant or the streaming kernel
int attn_fwd_bf16_kind(int N, int dh) {
  int W = 0;
  return use_resident(N, dh) ? res_variant(N, &W) : ATTN_STREAM;
}
// ... and attn_bwd_bf16: the merged kernel (under a token mask always: its masked instantiation is a ragged one), or delta +
// the two streaming kernels
int attn_bwd_bf16_kind(int N, int dh, bool q_prescaled, bool masked, int* kb, bool* ragged) {
  *kb = 0;
  *ragged = false;
  if (masked || attn_bwd_merged_ok(N, dh, q_prescaled)) {
    *kb = attn_bwd_merged_kb(N, ragged);
    if (masked) *ragged = true;
    return ATTN_MERGED;
  }
  return ATTN_STREAM;
}

int attn_bf16_plan(int N, int dh, bool q_prescaled, bool masked, int* fwd, int* bwd) {
  AVF_REQUIRE(N >= 1, "attn_plan: tokens %d", N);
  if (masked && !attn_masked_bf16_ok(N, dh, q_prescaled)) {  // attn_fwd_masked_bf16 / attn_bwd_masked_bf16: attn_fwd_vec / attn_bwd_vec
    AVF_REQUIRE(dh == 8 || dh == 16 || dh == 32 || dh == 64 || dh == 128, "attn_plan: unsupported dim_head %d (8,16,32,64,128)", dh);
    *fwd = *bwd = ATTN_F32;
    return 0;
  }
  AVF_REQUIRE(dh == 32 || dh == 64 || dh == 128, "attn_plan: unsupported dim_head %d (32, 64 or 128)", dh);
  int kb = 0;
  bool ragged = false;
  *fwd = attn_fwd_bf16_kind(N, dh);
  *bwd = attn_bwd_bf16_kind(N, dh, q_prescaled, masked, &kb, &ragged);
  if (*bwd == ATTN_MERGED) *bwd += 2 * kb + (ragged ? 1 : 0);
  return 0;
}

int attn_fwd_bf16(const bf16* qkv, bf16* o, float* lse2, int B, int N, int H, int dh, hipStream_t s, bool q_prescaled,
                  void* mx_q, void* mx_s, const void* keep) {
  AVF_REQUIRE(!keep || (attn_masked_bf16_ok(N, dh, q_prescaled) && !mx_q),
              "attn_fwd_bf16: the token mask runs on the MFMA kernels for dim_head 64, N <= 512, pre-scaled q, no fp8 image");
  AVF_REQUIRE(!mx_q || (mx_s && attn_fwd_emits_mx8(N, dh) && ((uintptr_t)mx_q & 3) == 0),
              "attn_fwd_bf16: the MX-FP8 output image exists on the head-resident kernel only (N=%d dh=%d)", N, dh);
  AVF_REQUIRE(B > 0 && N > 0 && H > 0, "attn_fwd_bf16: bad shape");
  AVF_REQUIRE(ceil_div(N, 128) * B * H < (1LL << 31), "attn_fwd_bf16: grid too large");
  AVF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)o & 7) == 0, "attn_fwd_bf16: misaligned pointers");
  TimingScope ts(KC_ATTN_FWD, 4.0 * B * H * (double)N * N * dh, 2.0 * 4.0 * B * N * H * dh, s, /*per_kernel=*/true);
  if (shape_log_on())
    shape_log("attn_fwd,attn_fwd,%d,%d,%d,%d,%d,%.0f,%.0f", B * H, B, N, H * dh, -1, 4.0 * B * H * (double)N * N * dh,
              2.0 * 4.0 * B * N * H * dh);
  if (attn_fwd_bf16_kind(N, dh) != ATTN_STREAM) {
    const size_t smem = (size_t)((N + 31) & ~31) * 128 * 2 + (keep ? (size_t)((N + 63) & ~63) : 0);
    return with_res_variant(N, [&](auto mw, auto mu, int W) {
      auto launch = [&](auto q, auto masked, uint8_t* mq, uint8_t* ms) {
        constexpr int MW = decltype(mw)::value;
        constexpr bool MU = decltype(mu)::value, Q = decltype(q)::value, MK = decltype(masked)::value;
        return res_launch<attn_fwd_res_kernel<MW, MU, Q, MK>>(&ts, "attn_fwd_res", res_tag<MW, MU, Q, MK>(), B * H, W, smem, s, qkv, o,
                                                              lse2, N, H, mq, ms, (const uint8_t*)keep);
      };
      if (keep) return launch(std::true_type{}, std::true_type{}, nullptr, nullptr);  // (pre-scaled q, no fp8 image: checked above)
      return with_bool(q_prescaled, [&](auto q) { return launch(q, std::false_type{}, (uint8_t*)mx_q, (uint8_t*)mx_s); });
    });
  }
  const unsigned grid = (unsigned)(ceil_div(N, 128) * B * H);
  const int qs = q_prescaled ? 1 : 0;
  return with_stream_dim_head(dh, [&](auto d, auto nw) {
    constexpr int DH = decltype(d)::value, NW = decltype(nw)::value;
    launch_in_scope(&ts, attn_fwd_bf16_kernel<DH, NW>, dim3(grid), dim3(64 * NW), 0, s, qkv, o, lse2, B, N, H, qs);
    return check_launch("attn_fwd_bf16_kernel");
  });
}

int attn_fwd_masked_bf16(const void* qkv, void* o, float* lse2, const void* keep, int B, int N, int H, int dh, hipStream_t s,
                         bool q_prescaled) {
  AVF_REQUIRE(keep, "attn_fwd_masked_bf16: no mask");
  if (attn_masked_bf16_ok(N, dh, q_prescaled))
    return attn_fwd_bf16((const bf16*)qkv, (bf16*)o, lse2, B, N, H, dh, s, true, nullptr, nullptr, keep);
  return attn_fwd_vec(AVF_BF16, qkv, o, lse2, B, N, H, dh, s, keep, q_prescaled, /*arith: fp32 storage only*/ 0);
}

bool attn_bwd_emits_mx8(int N, int dh, bool q_prescaled) { return attn_bwd_merged_ok(N, dh, q_prescaled); }

int attn_bwd_bf16(const bf16* qkv, const bf16* o, const bf16* d_o, const float* lse2, bf16* dqkv, float* delta, int B,
                  int N, int H, int dh, hipStream_t s, bool q_prescaled, const void* keep, void* dq_q, void* dq_s) {
  AVF_REQUIRE(!dq_q || (attn_bwd_emits_mx8(N, dh, q_prescaled) && !keep),
              "attn_bwd_bf16: the MX-FP8 image of dqkv exists on the merged kernel only (N=%d dh=%d)", N, dh);
  AVF_REQUIRE(!keep || attn_masked_bf16_ok(N, dh, q_prescaled),
              "attn_bwd_bf16: the token mask runs on the MFMA kernels for dim_head 64, N <= 512, pre-scaled q");
  AVF_REQUIRE(B > 0 && N > 0 && H > 0, "attn_bwd_bf16: bad shape");
  AVF_REQUIRE(ceil_div(N, 128) * B * H < (1LL << 31), "attn_bwd_bf16: grid too large");
  AVF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)d_o & 15) == 0 && ((uintptr_t)dqkv & 7) == 0,
              "attn_bwd_bf16: misaligned pointers");
  TimingScope ts(KC_ATTN_BWD, 10.0 * B * H * (double)N * N * dh, 2.0 * 8.0 * B * N * H * dh, s, /*per_kernel=*/true);
  if (shape_log_on())
    shape_log("attn_bwd,%s,%d,%d,%d,%d,%d,%.0f,%.0f", attn_bwd_merged_ok(N, dh, q_prescaled) ? "attn_bwd_m4_kernel" : "attn_dq+attn_dkv",
              B * H, B, N, H * dh, -1, 10.0 * B * H * (double)N * N * dh, 2.0 * 8.0 * B * N * H * dh);
  int kb = 0;
  bool ragged = false;
  const int kind = attn_bwd_bf16_kind(N, dh, q_prescaled, keep != nullptr, &kb, &ragged);
  // (under a mask the merged kernel at every N <= 512; no fp8 image then: checked above)
  if (kind == ATTN_MERGED) return attn_bwd_merged(&ts, qkv, o, d_o, lse2, dqkv, B, N, H, s, keep, dq_q, dq_s);
  AVF_TRY(attn_delta(AVF_BF16, o, d_o, delta, B, N, H, dh, s));
  const unsigned grid = (unsigned)(ceil_div(N, 128) * B * H);
  const int qs = q_prescaled ? 1 : 0;
  return with_stream_dim_head(dh, [&](auto d, auto nw) {
    constexpr int DH = decltype(d)::value, NW = decltype(nw)::value;
    launch_in_scope(&ts, attn_dq_bf16_kernel<DH, NW>, dim3(grid), dim3(64 * NW), 0, s, qkv, d_o, lse2, (const float*)delta, dqkv, B, N, H, qs);
    launch_in_scope(&ts, attn_dkv_bf16_kernel<DH, NW>, dim3(grid), dim3(64 * NW), 0, s, qkv, d_o, lse2, (const float*)delta, dqkv, B, N, H, qs);
    return check_launch("attn_bwd_bf16 kernels");
  });
}

int attn_bwd_masked_bf16(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, float* delta,
                         const void* keep, int B, int N, int H, int dh, hipStream_t s, bool q_prescaled) {
  AVF_REQUIRE(keep, "attn_bwd_masked_bf16: no mask");
  if (attn_masked_bf16_ok(N, dh, q_prescaled))  // (as the forward chose)
    return attn_bwd_bf16((const bf16*)qkv, (const bf16*)o, (const bf16*)d_o, lse2, (bf16*)dqkv, delta, B, N, H, dh, s, true, keep);
  return attn_bwd_vec(AVF_BF16, qkv, o, d_o, lse2, dqkv, delta, B, N, H, dh, s, keep, q_prescaled, /*arith: fp32 storage only*/ 0);
}

}  // namespace avf
