// layer.hip - host-side orchestration of one transformer layer (forward and backward) on a HIP stream.
//
// Reference: models/heads.py:246-255 - one (Residual(PreNorm(Attention)), Residual(PreNorm(FeedForward)))
// pair; SURVEY.md appendix A gives the op order and the backward formulas.  Everything here is
// enqueue-only (no allocation, no synchronisation) so a caller may capture it into a hipGraph.
//
// forward:   h1 = LN1(x)            -> qkv = h1 Wqkv^T          -> o = attn(qkv)
//            x_mid = o Wo^T + bo + x -> h2 = LN2(x_mid)          -> u = h2 W1^T + b1, g = gelu(u)
//            x_out = g W2^T + b2 + x_mid
// backward:  du = (dx_out W2) o gelu'(u) ; dW2 = dx_out^T g ; db2 = colsum(dx_out)
//            dh2 = du W1 ; dW1 = du^T h2 ; db1 = colsum(du)
//            dx_mid = dx_out + LN2'(dh2) ; dgamma2, dbeta2 ; dbo = colsum(dx_mid)   [fused in LN bwd]
//            do = dx_mid Wo ; dWo = dx_mid^T o ; dqkv = attn'(do) ; dWqkv = dqkv^T h1 ; dh1 = dqkv Wqkv
//            dx_in = dx_mid + LN1'(dh1) ; dgamma1, dbeta1
//
// How the file is organised: a layer's four Linears are four LinearW (shape, fp32 master, every image the mode keeps); an
// activation that feeds one is an Act (tensor + optional MX-FP8 image); linear_fwd / linear_dx pick the GEMM from the two.
// Forward is one sequence of eight steps; backward runs named phases over one LayerBwd (layer_bwd_impl lists them).
#include <algorithm>

#include "common.hpp"

namespace avf {

namespace {

struct Dims {
  int64_t R;  // rows = batch * tokens
  int D, H, dh, I, M, B, N;
  int dt;     // compute dtype
  int arith;  // parity mode (dt == AVF_F32): the arithmetic of every GEMM and of the attention of this call, 1 = bf16x3, 0 = f32-input MFMA
  size_t es;  // element size of compute dtype
  float p;    // dropout probability (0 = off)
  uint64_t seed;
  const uint64_t* seed_dev;
  int layer;
  bool gs16;  // backward keeps the residual gradient stream in bf16 (no fp32 dx between the LayerNorm backward kernels)
  bool gsd;   // ... with LIVE dropout: every hand-off is two bf16 images, the stream (never masked) and, behind it in the same
              // buffer, what the Linear behind the dropout site sees (masked, rescaled) - all-bf16 streams only (resid_bf16)
  bool mx;    // forward nn.Linear GEMMs fed by LayerNorm / GELU (qkv, mlp1, mlp2) take MX-FP8 operands (config 5)
  bool rs16;  // the FORWARD residual stream (x_in, x_mid, x_out) is stored in bf16 (statistics / accumulation stay fp32)
  int xdt;    // storage type of the residual stream
  float p0;   // dropout probability of site 0 (after to_out): 0 when to_out is nn.Identity (no Dropout in it, heads.py:214-217)
  const void* keep;  // optional token mask [B, N] bytes (1 = kept), heads.py:225-232: attention then runs on the fp32-arithmetic kernels
  bool mxb;   // backward dX GEMMs fed by LayerNorm backward / the dGELU epilogue take MX-FP8 operands too (config 5)
  bool gy_mx; // the caller's dx_out_lo buffer already carries the MX-FP8 image behind the bf16 one
};

// bf16 gradient-stream buffers in the mx8_bwd mode: [R, D] bf16 | [R, D] e4m3 | [R, D / 32] E8M0, each part 256-aligned
inline size_t grad_q_off(int64_t R, int D) { return align_up((size_t)R * D * 2, 256); }
inline size_t grad_s_off(int64_t R, int D) { return grad_q_off(R, D) + align_up((size_t)R * D, 256); }
inline size_t grad_stream_bytes(int64_t R, int D, bool mxb, bool gsd = false) {
  if (gsd) return 2 * grad_q_off(R, D);  // [R, D] bf16 stream | [R, D] bf16 masked image (at grad_q_off)
  return mxb ? grad_s_off(R, D) + align_up((size_t)R * D / 32, 256) : (size_t)R * D * 2;
}

int make_dims(const avf_layer_cfg* c, Dims* d) {
  AVF_REQUIRE(c, "layer: null cfg");
  AVF_REQUIRE(c->batch > 0 && c->tokens > 0 && c->dim > 0 && c->heads > 0 && c->dim_head > 0 && c->mlp_dim > 0,
              "layer: non-positive shape in cfg");
  AVF_REQUIRE(c->dtype == AVF_F32 || c->dtype == AVF_BF16, "layer: bad dtype %d", c->dtype);
  AVF_REQUIRE(c->f32_arith == 0 || c->f32_arith == 1, "layer: f32_arith=%d is neither 0 (f32-input MFMA) nor 1 (bf16x3)", c->f32_arith);
  AVF_REQUIRE(c->dropout_p >= 0.0f && c->dropout_p < 1.0f, "layer: dropout_p=%g out of range", (double)c->dropout_p);
  AVF_REQUIRE(c->dropout_p == 0.0f || (c->dim % 4 == 0 && c->dim <= 1536 && c->mlp_dim % 4 == 0),
              "layer: dropout needs dim %% 4 == 0, dim <= 1536");
  // the masks compare 16-bit uniforms with round(p * 65536): a p that rounds to 0 would leave "dropout_p > 0" (which selects the
  // masked gradient images of the bf16 streams) and the kernels' own predicate (thresh16 != 0) in disagreement - refuse it
  AVF_REQUIRE(c->dropout_p == 0.0f || make_drop(c->dropout_p, 0, 0, 0).thresh16 != 0,
              "layer: dropout_p=%g is below the mask resolution (2^-17): pass 0", (double)c->dropout_p);
  // nn.Identity to_out (heads == 1 && dim_head == dim, heads.py:207; never instantiated by the reference): the caller passes the
  // identity matrix as w_out and zeros as b_out (x 1.0 and + 0.0 are exact in fp32 and in bf16 with fp32 accumulation, so the
  // projection GEMM returns the attention output bit for bit) and the library drops the dropout site that nn.Identity lacks
  AVF_REQUIRE(c->project_out == 1 || (c->heads == 1 && c->dim_head == c->dim),
              "layer: project_out = 0 is the nn.Identity to_out case: it needs heads == 1 and dim_head == dim (heads.py:207)");
  d->B = c->batch; d->N = c->tokens; d->D = c->dim; d->H = c->heads; d->dh = c->dim_head;
  d->I = c->heads * c->dim_head; d->M = c->mlp_dim; d->R = (int64_t)c->batch * c->tokens;
  d->dt = c->dtype; d->es = c->dtype == AVF_BF16 ? 2 : 4; d->arith = c->f32_arith;
  d->p = c->dropout_p; d->seed = ((uint64_t)c->seed_hi << 32) | c->seed_lo; d->layer = c->layer_index;
  d->seed_dev = (const uint64_t*)c->seed_dev;
  d->gs16 = c->grad_stream_bf16 != 0;
  d->gsd = d->gs16 && c->dropout_p > 0.0f;
  AVF_REQUIRE(!d->gs16 || (c->dtype == AVF_BF16 && c->dim <= 1536), "layer: grad_stream_bf16 needs the bf16 path and dim <= 1536");
  AVF_REQUIRE(!d->gsd || (c->resid_bf16 != 0 && c->mx8_fwd == 0 && c->dim % 8 == 0),
              "layer: grad_stream_bf16 with dropout_p > 0 needs resid_bf16 (all-bf16 streams), no mx8 and dim %% 8 == 0");
  d->mx = c->mx8_fwd != 0;
  AVF_REQUIRE(!d->mx || (c->dtype == AVF_BF16 && c->dim % 128 == 0 && c->mlp_dim % 128 == 0 && c->dim <= 1536),
              "layer: mx8_fwd needs the bf16 path with dim and mlp_dim multiples of 128 (dim=%d mlp_dim=%d)", c->dim,
              c->mlp_dim);
  d->p0 = c->project_out ? c->dropout_p : 0.0f;
  d->keep = c->key_mask;
  d->mxb = c->mx8_bwd != 0;
  d->gy_mx = c->dx_out_mx8 != 0;
  AVF_REQUIRE(!d->mxb || d->mx, "layer: mx8_bwd needs mx8_fwd");
  d->rs16 = c->resid_bf16 != 0;
  d->xdt = d->rs16 ? AVF_BF16 : AVF_F32;
  AVF_REQUIRE(!d->rs16 || (c->dtype == AVF_BF16 && c->dim % 8 == 0 && c->dim <= 1536),
              "layer: resid_bf16 needs the bf16 path, dim %% 8 == 0 and dim <= 1536 (dim=%d)", c->dim);
  if (c->dtype == AVF_BF16) {
    AVF_REQUIRE(d->D % 8 == 0 && d->I % 8 == 0 && d->M % 8 == 0, "layer(bf16): dim, inner and mlp_dim must be multiples of 8");
    AVF_REQUIRE(d->dh == 32 || d->dh == 64 || d->dh == 128, "layer(bf16): dim_head must be 32, 64 or 128 (got %d)", d->dh);
  } else {
    AVF_REQUIRE(d->D % 4 == 0 && d->I % 4 == 0 && d->M % 4 == 0, "layer(f32): dim, inner and mlp_dim must be multiples of 4");
  }
  return 0;
}

struct Carver {
  char* base;
  size_t off;
  explicit Carver(void* b) : base((char*)b), off(0) {}
  void* take(size_t bytes) {
    void* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  }
};

struct Saved {
  void *h1, *qkv, *o, *h2, *u, *g, *x_mid;  // x_mid: fp32, or bf16 on the bf16 residual stream
  float *mean1, *rstd1, *lse2, *mean2, *rstd2;
};
size_t carve_saved(const Dims& d, void* base, Saved* s) {
  Carver c(base);
  Saved t{};
  t.h1 = c.take(d.R * d.D * d.es);
  t.mean1 = (float*)c.take(d.R * 4);
  t.rstd1 = (float*)c.take(d.R * 4);
  t.qkv = c.take(d.R * 3 * d.I * d.es);
  t.o = c.take(d.R * d.I * d.es);
  t.lse2 = (float*)c.take((size_t)d.B * d.H * d.N * 4);
  t.x_mid = c.take(d.R * d.D * (d.rs16 ? 2 : 4));
  t.h2 = c.take(d.R * d.D * d.es);
  t.mean2 = (float*)c.take(d.R * 4);
  t.rstd2 = (float*)c.take(d.R * 4);
  t.u = c.take(d.R * d.M * d.es);
  t.g = c.take(d.R * d.M * d.es);
  if (s) *s = t;
  return c.off;
}

// One nn.Linear of the layer, y[R, out] = x[R, in] W[out, in]^T, with every image of W that the mode keeps (null where it keeps
// none; all null in the fp32 mode, which multiplies with the master itself)
struct LinearW {
  int out, in;
  const float* w;   // fp32 master (null where the caller brought the image buffer alone)
  void *lo, *lo_t;  // bf16 W [out, in] and W^T [in, out] (the dX GEMM's operand, an NT GEMM again)
  void *q, *s;      // mx8_fwd: MX-FP8 image of lo (e4m3 bytes + one E8M0 scale byte per 32 along in)
  void *tq, *ts;    // mx8_bwd: MX-FP8 image of lo_t (blocks along out, the reduction of dX)
  void *p, *tp;     // fragment-major images of lo / lo_t for the weight-stationary GEMM (gemm_ws.hip), null if unfit
};
// the order is the one of the grouped weight-gradient launch: attention half, then MLP half - the XCD-aware block order of the
// 256 x 128 kernel cuts the tile list in the middle, and the two halves then share no operand panel (3 I D + D I tiles |
// 2 M D tiles: equal when I = D, M = 2 D)
enum { kQkv, kOut, kMlp1, kMlp2, kLinears };
struct LayerW { LinearW lin[kLinears]; };
// MX-FP8 images in the lowp buffer, and their quantiser jobs: the row-major images in the first order, then the transposed ones
// in the second (the orders in which the images were added to the buffer; every offset in it is fixed)
constexpr int kMxOrder[kLinears] = {kQkv, kMlp1, kMlp2, kOut}, kMxOrderT[kLinears] = {kMlp2, kMlp1, kOut, kQkv};
struct Shape { int out, in; };
Shape linear_shape(const Dims& d, int i) {  // W[out, in] of the four
  const Shape s[kLinears] = {{3 * d.I, d.D}, {d.D, d.I}, {d.M, d.D}, {d.D, d.M}};
  return s[i];
}

// Shapes, masters (p may be null) and images of the four Linears.  Layout of the lowp buffer: the eight bf16 images lead
// (avf_*_adam_step finds them by their offsets from the front), the MX-FP8 images follow, the fragment-major images come LAST.
size_t carve_lowp(const Dims& d, void* base, LayerW* out, const avf_layer_params* p = nullptr) {
  LayerW t{};
  const float* const master[kLinears] = {p ? p->w_qkv : nullptr, p ? p->w_out : nullptr, p ? p->w1 : nullptr, p ? p->w2 : nullptr};
  for (int i = 0; i < kLinears; ++i) { t.lin[i].out = linear_shape(d, i).out; t.lin[i].in = linear_shape(d, i).in; t.lin[i].w = master[i]; }
  Carver c(base);
  if (d.dt == AVF_BF16) {
    for (LinearW& L : t.lin) { L.lo = c.take((size_t)L.out * L.in * 2); L.lo_t = c.take((size_t)L.out * L.in * 2); }
    if (d.mx) {  // (the transposed images have their place in every mx8_fwd buffer; avf_stack_quant_weights_mx8 fills them for mx8_bwd)
      for (int i = 0; i < kLinears; ++i) {
        LinearW& L = t.lin[kMxOrder[i]];
        L.q = c.take((size_t)L.out * L.in); L.s = c.take((size_t)L.out * L.in / 32);
      }
      for (int i = 0; i < kLinears; ++i) {
        LinearW& L = t.lin[kMxOrderT[i]];
        L.tq = c.take((size_t)L.out * L.in); L.ts = c.take((size_t)L.out * L.in / 32);
      }
    }
    // Wqkv [3I, D], Wo [D, I], W1 [M, D] (forward) and W2^T [M, D], Wo^T [I, D] (the dX GEMMs with a 512-deep reduction)
    const struct { int lin; bool transposed; } ws[] = {{kQkv, false}, {kOut, false}, {kMlp1, false}, {kMlp2, true}, {kOut, true}};
    for (const auto& e : ws) {
      LinearW& L = t.lin[e.lin];
      const int rows = e.transposed ? L.in : L.out, cols = e.transposed ? L.out : L.in;
      if (pack_ws_ok(rows, cols)) (e.transposed ? L.tp : L.p) = c.take(pack_ws_bytes(rows, cols));
    }
  }
  if (out) *out = t;
  return c.off;
}

// the four weight-gradient GEMMs of a layer as one grouped launch, dW[out, in] = dY[R, out]^T X[R, in] (all reduce over the R
// token rows): the shapes here, the operands by dw_problem
TnGroupArgs dw_group(const Dims& d) {
  TnGroupArgs a{};
  a.count = kLinears; a.K = d.R; a.f32_arith = d.arith;
  for (int i = 0; i < kLinears; ++i) { a.M[i] = a.lda[i] = linear_shape(d, i).out; a.N[i] = a.ldb[i] = linear_shape(d, i).in; }
  return a;
}
void dw_problem(TnGroupArgs& a, int i, const void* dY, const void* X, float* dW) { a.A[i] = dY; a.B[i] = X; a.C[i] = dW; }

size_t work_colsum_bytes(const Dims& d) {
  size_t csb = colsum_ws(d.R, std::max(d.M, d.D));
  if (d.dt == AVF_BF16) csb = std::max(csb, gemm_nt_colsum_ws(d.R, d.M));
  return csb;
}
// split-K scratch of the weight gradients: the largest of the four single launches and of the grouped one
size_t work_dw_bytes(const Dims& d) {
  const bool lo = d.dt == AVF_BF16;
  const TnGroupArgs ga = dw_group(d);
  // (parity mode: narrow layers split their long token reduction, gemm_f32_ws; neither size depends on d.arith: the buffer serves
  // either arithmetic)
  size_t g = lo ? gemm_bf16_tn_group_ws(ga) : gemm_f32x3_tn_group_ws(ga);
  for (int i = 0; i < ga.count; ++i) g = std::max(g, lo ? gemm_bf16_tn_ws(ga.M[i], ga.N[i], d.R) : gemm_f32_ws(ga.M[i], ga.N[i], d.R));
  return g;
}

struct Work {
  void *du, *dh, *d_o, *dqkv, *dx_mid_lo, *dx_out_lo, *ln_ws, *ln_ws1, *cs_ws, *gemm_ws;
  float *dx_mid, *delta;
  void *hq, *hs, *gq, *gs;  // mx8_fwd only: MX-FP8 images of the LayerNorm output and of gelu(u), forward scratch
  void *oq, *os;            // mx8_fwd: image of the attention output (forward scratch)
  void *duq, *dus, *mq, *ms, *gyq, *gys;  // mx8_bwd: images of du, of dx_mid, and of dx_out when the caller brought none
  void *dqq, *dqs;                        // mx8_bwd: image of dqkv (written by the merged attention backward)
  void *dx_out_s, *dx_mid_m;  // gsd: the unmasked bf16 stream image of dx_out (top of the stack), the masked image of dx_mid
  float *gy_m, *gm_m;       // fp32 mode with live dropout: masked copies of dx_out / dx_mid (what the Linears behind sites 2 / 0 see)
  float* small_part;        // short-sequence backward: per-clip partial rows (pb1 [B][M] | pln2 [B][3D] | pln1 [B][3D])
};
size_t carve_work(const Dims& d, void* base, Work* w) {
  Carver c(base);
  Work t{};
  t.du = c.take(d.R * d.M * d.es);
  t.dh = c.take(d.R * d.D * d.es);
  t.d_o = c.take(d.R * d.I * d.es);
  t.dqkv = c.take(d.R * 3 * d.I * d.es);
  t.dx_mid = (float*)c.take(d.R * d.D * 4);
  t.dx_mid_lo = c.take(d.dt == AVF_BF16 ? d.R * d.D * 2 : 0);
  t.dx_out_lo = c.take(d.dt == AVF_BF16 ? d.R * d.D * 2 : 0);
  t.delta = (float*)c.take((size_t)d.B * d.H * d.N * 4);
  t.ln_ws = c.take(layernorm_bwd_ws(d.R, d.D));
  t.ln_ws1 = c.take(layernorm_bwd_ws(d.R, d.D, d.N));  // LN1 partials (its fold may be deferred past LN2's; token-major: one row per token)
  t.cs_ws = c.take(work_colsum_bytes(d));
  t.gemm_ws = c.take(work_dw_bytes(d));
  t.small_part = (float*)c.take(small_layer_ok(d.dt, d.N, d.D, d.H, d.dh, d.M) ? small_bwd_partial_floats(d.B, d.D, d.M) * 4 : 0);
  if (d.mx) {
    t.hq = c.take(d.R * d.D); t.hs = c.take(d.R * d.D / 32);
    t.gq = c.take(d.R * d.M); t.gs = c.take(d.R * d.M / 32);
    t.oq = c.take(d.R * d.I); t.os = c.take(d.R * d.I / 32);
  }
  if (d.mxb) {
    t.duq = c.take(d.R * d.M); t.dus = c.take(d.R * d.M / 32);
    t.mq = c.take(d.R * d.D);  t.ms = c.take(d.R * d.D / 32);
    t.gyq = c.take(d.R * d.D); t.gys = c.take(d.R * d.D / 32);
    t.dqq = c.take(d.R * 3 * d.I); t.dqs = c.take(d.R * 3 * d.I / 32);
  }
  t.dx_out_s = c.take(d.gsd ? d.R * d.D * 2 : 0);
  t.dx_mid_m = c.take(d.gsd ? d.R * d.D * 2 : 0);
  const bool f32_drop = d.dt == AVF_F32 && d.p > 0.f;
  t.gy_m = (float*)c.take(f32_drop ? d.R * d.D * 4 : 0);
  t.gm_m = (float*)c.take(f32_drop ? d.R * d.D * 4 : 0);
  if (w) *w = t;
  return c.off;
}

// A layer whose weight gradients are DEFERRED (avf_layer_bwd_dx, avf_layers_dw) keeps what the grouped launch will read in a
// block of its own instead of the shared scratch, which the layers below overwrite: the A operands du, dqkv and dx_mid_lo (the
// B operands already live in the layer's saved activations), the bf16 image of dx_out where the layer made it itself, and the
// partial rows of its three column folds.  bf16 path only.
size_t carve_dw_block(const Dims& d, void* base, Work* w) {
  Carver c(base);
  Work sizes_only{};
  Work& t = w ? *w : sizes_only;  // (the other fields of *w stay what carve_work made them)
  t.du = c.take(d.R * d.M * 2);
  t.dqkv = c.take(d.R * 3 * d.I * 2);
  t.dx_mid_lo = c.take(d.R * d.D * 2);
  t.dx_out_lo = c.take(d.R * d.D * 2);
  t.ln_ws = c.take(layernorm_bwd_ws(d.R, d.D));
  t.ln_ws1 = c.take(layernorm_bwd_ws(d.R, d.D, d.N));
  t.cs_ws = c.take(work_colsum_bytes(d));
  return c.off;
}
// what avf_layer_bwd_dx leaves behind for avf_layers_dw (host memory, caller-provided, avf_layer_dw_desc_bytes() long)
constexpr uint32_t kDwDescMagic = 0x64574431u;
struct DwDeferred {
  uint32_t magic;
  TnGroupArgs grp;   // the four problems of the layer, attention half first (dw_group)
  FoldJob folds[3];  // db1 | dgamma2, dbeta2, dbo | dgamma1, dbeta1, the db2 of the layer below
};
// the modes whose weight gradients can wait: the bf16 path on its grouped launch, nothing that adds images or masks
bool dw_defer_mode_ok(const Dims& d) {
  return d.dt == AVF_BF16 && !d.gsd && d.p == 0.f && !d.mx && !d.mxb && !d.keep && !small_layer_ok(d.dt, d.N, d.D, d.H, d.dh, d.M);
}

// the dropout sites of a layer (make_drop: 0 after to_out, 1 after GELU, 2 after net.3) and, for the gradient handed to the layer
// below, that layer's site 2.  p0: no site 0 behind an nn.Identity to_out
struct Drops { DropCfg site0, site1, site2, prev2; };
Drops make_drops(const Dims& d) {
  const auto site = [&d](float p, int layer, int k) { return make_drop(p, d.seed, layer, k, d.seed_dev); };
  return Drops{site(d.p0, d.layer, 0), site(d.p, d.layer, 1), site(d.p, d.layer, 2), d.layer > 0 ? site(d.p, d.layer - 1, 2) : kNoDrop};
}

// An activation or gradient as the A operand of a Linear's GEMM: the tensor in the compute dtype and, where its producer wrote
// one, its MX-FP8 image (q: e4m3 bytes, s: E8M0 scales along the reduction)
struct Act { const void *x, *q, *s; };
// C[R, out] = x[R, in] * W[out, in]^T  (nn.Linear forward): on MX-FP8 operands when the mode says so and both images exist,
// else on the bf16 image (with its fragment-major image, where there is one, for the weight-stationary kernel) / the fp32 master.
// e: what the GEMM does beside the product - epilogue, bias, residual, aux, drop, colsum + workspace + defer_fold, mx_q / mx_s
// (the MX-FP8 image of the result) - in a GemmArgs of which nothing else is set
int linear_fwd(const Dims& d, const LinearW& L, const Act& x, void* C, int c_dtype, const GemmArgs& e, hipStream_t s) {
  GemmArgs a = gemm_dense(d.dt, 0, 1, d.R, L.out, L.in, e);
  a.C = C; a.c_dtype = c_dtype; a.f32_arith = d.arith;
  if (d.mx && x.q && L.q) {
    a.A = x.q; a.B = L.q; a.mx_q = a.mx_s = nullptr;
    return gemm_mx8_nt(a, x.s, L.s, s, e.mx_q, e.mx_s);
  }
  a.A = x.x; a.B = d.dt == AVF_BF16 ? L.lo : (const void*)L.w; a.Bp = L.p;
  return gemm(a, s);
}

// dX[R, in] = dY[R, out] * W[out, in].  bf16 mode consumes the transposed image lo_t [in, out] as an NT GEMM; mx8_bwd the
// MX-FP8 images of dY and of lo_t when both exist.  ws_first: where the weight-stationary bf16 kernel takes the shape it is
// preferred to the MX-FP8 GEMM (it writes e.mx_q / e.mx_s itself)
int linear_dx(const Dims& d, const LinearW& L, const Act& dy, void* dX, const GemmArgs& e, hipStream_t s, bool ws_first = false) {
  const bool lo = d.dt == AVF_BF16;
  GemmArgs a = gemm_dense(d.dt, 0, lo ? 1 : 0, d.R, L.in, L.out, e);
  a.A = dy.x; a.B = lo ? L.lo_t : (const void*)L.w; a.Bp = L.tp;
  a.C = dX; a.c_dtype = d.dt; a.f32_arith = d.arith;
  if (!(d.mxb && dy.q && L.tq) || (ws_first && gemm_bf16_nt_ws_ok(a))) return gemm(a, s);
  a.A = dy.q; a.B = L.tq; a.Bp = nullptr; a.mx_q = a.mx_s = nullptr;
  return gemm_mx8_nt(a, dy.s, L.ts, s, e.mx_q, e.mx_s);
}

// dW[out, in] = dY[R, out]^T * X[R, in]   (fp32 result)
int linear_dw(const Dims& d, const LinearW& L, const void* dY, const void* X, float* dW, void* ws, hipStream_t s) {
  GemmArgs a = gemm_dense(d.dt, 1, 0, L.out, L.in, d.R);
  a.A = dY; a.B = X; a.C = dW; a.c_dtype = AVF_F32; a.workspace = ws; a.f32_arith = d.arith;
  return gemm(a, s);
}

}  // namespace

size_t gemm_ws(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K) {
  if (dtype == AVF_BF16 && transA == 1 && transB == 0) return gemm_bf16_tn_ws(M, N, K);
  if (dtype == AVF_F32) return gemm_f32_ws(M, N, K);
  return 0;
}

int lowp_ws_images(const avf_layer_cfg* cfg, void* lowp, LowpWs* out) {
  Dims d;
  AVF_TRY(make_dims(cfg, &d));
  LayerW W;
  carve_lowp(d, lowp, &W);
  *out = LowpWs{W.lin[kQkv].p, W.lin[kOut].p, W.lin[kMlp1].p, W.lin[kMlp2].tp, W.lin[kOut].tp};
  return 0;
}

int gemm(const GemmArgs& a, hipStream_t s) {
  if (a.dtype == AVF_F32) return gemm_f32(a, s);
  if (a.dtype == AVF_BF16) {
    if (a.transA == 0 && a.transB == 1) return gemm_bf16_nt(a, s);
    if (a.transA == 1 && a.transB == 0) return gemm_bf16_tn(a, s);
    AVF_REQUIRE(false, "gemm(bf16): only NT (transA=0,transB=1) and TN (transA=1,transB=0) forms exist");
  }
  AVF_REQUIRE(false, "gemm: bad dtype %d", a.dtype);
}

}  // namespace avf

using namespace avf;

extern "C" size_t avf_layer_saved_bytes(const avf_layer_cfg* cfg) {
  Dims d;
  if (make_dims(cfg, &d)) return 0;
  return carve_saved(d, nullptr, nullptr);
}
extern "C" size_t avf_layer_lowp_bytes(const avf_layer_cfg* cfg) {
  Dims d;
  if (make_dims(cfg, &d)) return 0;
  return carve_lowp(d, nullptr, nullptr);
}
extern "C" size_t avf_layer_grad_stream_bytes(const avf_layer_cfg* cfg) {
  Dims d;
  if (make_dims(cfg, &d)) return 0;
  return grad_stream_bytes(d.R, d.D, d.mxb, d.gsd);
}
extern "C" size_t avf_layer_workspace_bytes(const avf_layer_cfg* cfg) {
  Dims d;
  if (make_dims(cfg, &d)) return 0;
  return align_up(carve_work(d, nullptr, nullptr), 256);
}

extern "C" int avf_layer_prepare_weights(const avf_layer_cfg* cfg, const avf_layer_params* p, void* lowp,
                                         void* stream) {
  Dims d;
  AVF_TRY(make_dims(cfg, &d));
  if (d.dt != AVF_BF16) return 0;
  AVF_REQUIRE(p && lowp, "prepare_weights: null pointer");
  LayerW W;
  carve_lowp(d, lowp, &W, p);
  // one launch writes, per Linear, the bf16 image, its transpose and the fragment-major images for the weight-stationary GEMM that
  // the shape has (the optimizer step rewrites all of them itself: optim.hip)
  PrepBatch b;
  for (int i = 0; i < kLinears; ++i) {
    const LinearW& L = W.lin[i];
    b.d[i] = PrepDesc{L.w, (bf16*)L.lo, (bf16*)L.lo_t, L.out, L.in, 1.0f, 0, L.p, L.tp};
  }
  // the query rows of the forward image of Wqkv carry the softmax scale (the transposed image, which backward
  // multiplies dqkv with, does not): q' = h1 (c Wq)^T, so the attention kernels get log2-domain scores from the MFMA
  b.d[kQkv].lo_scale = attn_q_prescale(d.dh);
  b.d[kQkv].lo_scaled_rows = d.I;
  return prep_weights_multi(b, kLinears, (hipStream_t)stream);
}

extern "C" int avf_stack_quant_weights_mx8(const avf_layer_cfg* cfg, int layers, void* const* lowp, void* stream) {
  Dims d;
  AVF_TRY(make_dims(cfg, &d));
  AVF_REQUIRE(d.mx, "stack_quant_weights_mx8: cfg.mx8_fwd is not set");
  AVF_REQUIRE(layers > 0 && layers <= 64 && lowp, "stack_quant_weights_mx8: bad arguments");
  MxQuantJob jobs[64 * 8];
  int n = 0;
  for (int i = 0; i < layers; ++i) {
    AVF_REQUIRE(lowp[i], "stack_quant_weights_mx8: null image buffer (layer %d)", i);
    LayerW W;
    carve_lowp(d, lowp[i], &W);
    // an image exists where the 32-blocks tile its reduction axis in whole 128-deep K-steps (in of Wo is I, out of Wqkv 3 I: any
    // multiple of 8; dim and mlp_dim are multiples of 128 in this mode)
    for (int k = 0; k < kLinears; ++k) {
      const LinearW& L = W.lin[kMxOrder[k]];
      if (L.in % 128 == 0) jobs[n++] = MxQuantJob{L.lo, L.q, L.s, L.out, L.in};
    }
    for (int k = 0; k < kLinears && d.mxb; ++k) {  // transposed images: Wt[in, out], blocks along out
      const LinearW& L = W.lin[kMxOrderT[k]];
      if (L.out % 128 == 0) jobs[n++] = MxQuantJob{L.lo_t, L.tq, L.ts, L.in, L.out};
    }
  }
  return quant_mx8_multi(jobs, n, (hipStream_t)stream);
}

// The two ends of a fused stack (avf_layer_fwd_embed, avf_layer_bwd_pos / avf_layer_bwd_dx_pos): the all-bf16 streams of the
// general bf16 layer - no dropout, no MX-FP8 images, no key mask - on the row8 LayerNorm kernels.  A caller asks the _ok function
// and takes the plain entry points where it says no (the stack's own switch for A/B runs is AVF_STACK_ENDS, transformer.py).
static bool stack_ends_mode_ok(const Dims& d) {
  return d.dt == AVF_BF16 && d.rs16 && d.gs16 && !d.gsd && d.p == 0.f && !d.mx && !d.mxb &&
         !d.keep && d.D % 8 == 0 && d.D <= 1536;
}
extern "C" int avf_layer_fwd_embed_ok(const avf_layer_cfg* cfg) {
  Dims d;
  return !make_dims(cfg, &d) && stack_ends_mode_ok(d) && layernorm_fwd_embed_ok(d.D);
}
extern "C" int avf_layer_bwd_pos_ok(const avf_layer_cfg* cfg) {
  Dims d;
  return !make_dims(cfg, &d) && stack_ends_mode_ok(d) && layernorm_bwd_tok_ok(d.B, d.N, d.D);
}

// The three decisions of the short-sequence layer (layer_small.hip), each taken at ONE place - layer_fwd_impl, LayerBwd::begin,
// LayerBwd::small - and answered to a caller by avf_layer_small_path from the same three functions.
static bool small_fwd_taken(const Dims& d) {  // the whole forward in one launch
  return !d.mx && !d.rs16 && !d.keep && small_layer_ok(d.dt, d.N, d.D, d.H, d.dh, d.M);
}
static bool small_bwd_taken(const Dims& d) {  // the two fused kernels around the attention backward
  static const int small_bwd_on = tuning_int("AVF_LAYER_SMALL_BWD", 1);  // tuning / A-B aid
  return d.dt == AVF_BF16 && !d.rs16 && !d.mx && !d.keep && small_bwd_on && small_layer_ok(d.dt, d.N, d.D, d.H, d.dh, d.M);
}
static bool small_att_fused(const Dims& d) {  // ... the second of which runs the attention backward itself
  static const int small_att_on = tuning_int("AVF_LAYER_SMALL_ATT", 1);  // tuning / A-B aid: 0 = per-operator attention backward
  return small_att_on && d.H <= 16;
}
extern "C" int avf_layer_small_path(const avf_layer_cfg* cfg) {
  Dims d;
  if (make_dims(cfg, &d)) return 0;
  const bool bwd = small_bwd_taken(d);
  return (small_fwd_taken(d) ? 1 : 0) | (bwd ? 2 : 0) | (bwd && small_att_fused(d) ? 4 : 0);
}

// emb (avf_layer_fwd_embed): the layer's input is cat([clip, audio], 1) + pos; LayerNorm-1 builds it and stores it as emb->x0
struct EmbedSrc { const float *clip, *audio, *pos; int t_video; void* x0; };
struct LayerFwdIO { const void* x_in; void *x_out, *saved; const EmbedSrc* emb; };  // x_in: null with emb

// o = attn(qkv).  oq / os (config 5, optional): the head-resident kernel also writes the MX-FP8 image of o
static int fwd_attention(const Dims& d, const Saved& sv, void* oq, void* os, hipStream_t s) {
  const bool lo = d.dt == AVF_BF16;
  // token mask (heads.py:225-232): on the MFMA kernels where they carry it (bf16, dim_head 64, up to 512 tokens), else on
  // the fp32-arithmetic ones (attn_fwd_masked_bf16 chooses); the fp8 mode and the fp32 mode go to the fp32-arithmetic ones directly
  if (d.keep && lo && !d.mx) return attn_fwd_masked_bf16(sv.qkv, sv.o, sv.lse2, d.keep, d.B, d.N, d.H, d.dh, s, /*q_prescaled=*/true);
  if (d.keep) return attn_fwd_vec(d.dt, sv.qkv, sv.o, sv.lse2, d.B, d.N, d.H, d.dh, s, d.keep, /*q_prescaled=*/d.mx, d.arith);
  if (lo) return attn_fwd_bf16((const bf16*)sv.qkv, (bf16*)sv.o, sv.lse2, d.B, d.N, d.H, d.dh, s, /*q_prescaled=*/true, oq, os);
  return attn_fwd_f32((const float*)sv.qkv, (float*)sv.o, sv.lse2, d.B, d.N, d.H, d.dh, s, d.arith);
}

static int layer_fwd_impl(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const LayerFwdIO& io,
                          void* workspace, void* stream) {
  Dims d;
  AVF_TRY(make_dims(cfg, &d));
  const EmbedSrc* emb = io.emb;
  const void* x_in = io.x_in;
  if (emb) {
    AVF_REQUIRE(stack_ends_mode_ok(d) && layernorm_fwd_embed_ok(d.D) && emb->x0 && emb->t_video > 0 && emb->t_video < d.N,
                "layer_fwd_embed: needs the all-bf16 streams without dropout, fp8 or mask, and both token groups (ask "
                "avf_layer_fwd_embed_ok first)");
    x_in = emb->x0;
  }
  AVF_REQUIRE(p && x_in && io.x_out && io.saved, "layer_fwd: null pointer");
  AVF_REQUIRE(d.dt == AVF_F32 || lowp, "layer_fwd(bf16): lowp weights missing");
  hipStream_t s = (hipStream_t)stream;
  Saved sv;
  carve_saved(d, io.saved, &sv);
  LayerW W;
  carve_lowp(d, (void*)lowp, &W, p);
  const LinearW &qkv = W.lin[kQkv], &out = W.lin[kOut], &mlp1 = W.lin[kMlp1], &mlp2 = W.lin[kMlp2];
  const Drops dr = make_drops(d);
  // config 5 (mx8_fwd): the three GEMMs whose A operand leaves a row-wise producer (LayerNorm, GELU epilogue) run on the MX-FP8
  // matrix path; the producers emit the e4m3 image (hq / hs, gq / gs) beside the bf16 tensor backward needs, the weights' images
  // come from avf_stack_quant_weights_mx8.  (mx8_bwd: the dX GEMMs fed by LayerNorm backward / dGELU likewise, avf_layer_bwd.)
  // In every other mode the images are null and each Linear runs on its bf16 / fp32 operands.
  Work w{};
  bool o_mx = false;
  if (d.mx) {
    AVF_REQUIRE(workspace, "layer_fwd(mx8): workspace missing");
    carve_work(d, workspace, &w);
    // out-proj: its A operand is produced per head; the head-resident attention kernel writes the image from its epilogue
    static const int o_mx_on = tuning_int("AVF_MX8_OUTPROJ", 1);  // tuning / A-B aid: 0 = out-projection on bf16 operands
    o_mx = o_mx_on && !d.keep && attn_fwd_emits_mx8(d.N, d.dh) && d.I % 128 == 0;
  } else if (small_fwd_taken(d)) {  // short sequences: the whole layer in one launch
    const bool lo = d.dt == AVF_BF16;
    return layer_fwd_small(d.B, d.N, d.D, d.H, d.M, cfg->ln_eps, /*score_scale=*/1.0f, p, lo ? qkv.lo : (const void*)qkv.w, lo ? out.lo : (const void*)out.w,
                           lo ? mlp1.lo : (const void*)mlp1.w, lo ? mlp2.lo : (const void*)mlp2.w, (const float*)x_in, (float*)io.x_out,
                           sv.h1, sv.mean1, sv.rstd1, sv.qkv, sv.o, sv.lse2, (float*)sv.x_mid, sv.h2, sv.mean2, sv.rstd2, sv.u, sv.g,
                           dr.site0, dr.site1, dr.site2, s);
  }
  void *oq = o_mx ? w.oq : nullptr, *os = o_mx ? w.os : nullptr;
  if (emb)
    AVF_TRY(layernorm_fwd_embed(emb->clip, emb->audio, emb->pos, d.B, emb->t_video, d.N - emb->t_video, emb->x0, p->ln1_w, p->ln1_b,
                                sv.h1, sv.mean1, sv.rstd1, d.D, cfg->ln_eps, s));
  else
    AVF_TRY(layernorm_fwd(x_in, p->ln1_w, p->ln1_b, sv.h1, d.dt, sv.mean1, sv.rstd1, d.R, d.D, cfg->ln_eps, s, w.hq, w.hs, d.xdt));
  AVF_TRY(linear_fwd(d, qkv, Act{sv.h1, w.hq, w.hs}, sv.qkv, d.dt, GemmArgs{}, s));
  AVF_TRY(fwd_attention(d, sv, oq, os, s));
  GemmArgs e_out, e_up, e_down;
  e_out.epilogue = AVF_EPI_BIAS_RES; e_out.bias = p->b_out; e_out.residual = x_in; e_out.drop = dr.site0;
  AVF_TRY(linear_fwd(d, out, Act{sv.o, oq, os}, sv.x_mid, d.xdt, e_out, s));
  AVF_TRY(layernorm_fwd(sv.x_mid, p->ln2_w, p->ln2_b, sv.h2, d.dt, sv.mean2, sv.rstd2, d.R, d.D, cfg->ln_eps, s, w.hq, w.hs, d.xdt));
  e_up.epilogue = AVF_EPI_BIAS_GELU; e_up.bias = p->b1; e_up.aux = sv.u; e_up.drop = dr.site1; e_up.mx_q = w.gq; e_up.mx_s = w.gs;
  AVF_TRY(linear_fwd(d, mlp1, Act{sv.h2, w.hq, w.hs}, sv.g, d.dt, e_up, s));
  e_down.epilogue = AVF_EPI_BIAS_RES; e_down.bias = p->b2; e_down.residual = sv.x_mid; e_down.drop = dr.site2;
  AVF_TRY(linear_fwd(d, mlp2, Act{sv.g, w.gq, w.gs}, io.x_out, d.xdt, e_down, s));
  return 0;
}

extern "C" int avf_layer_fwd(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                             void* x_out, void* saved, void* workspace, void* stream) {
  return layer_fwd_impl(cfg, p, lowp, LayerFwdIO{x_in, x_out, saved, nullptr}, workspace, stream);
}
extern "C" int avf_layer_fwd_embed(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const float* clip,
                                   const float* audio, const float* pos, int t_video, void* x0, void* x_out, void* saved,
                                   void* workspace, void* stream) {
  const EmbedSrc emb{clip, audio, pos, t_video, x0};
  return layer_fwd_impl(cfg, p, lowp, LayerFwdIO{nullptr, x_out, saved, &emb}, workspace, stream);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// The caller's pointers (not ABI: the extern "C" entries fill it by field name).
struct LayerBwdIO {
  const void *x_in = nullptr, *saved = nullptr;
  // gradient of the layer output: fp32, and / or its bf16 image (bf16 gradient stream: the image alone will do); its column sums
  // (db2) where the layer above has made them
  const float *dx_out = nullptr, *dx_out_colsum = nullptr;
  const void* dx_out_lo = nullptr;
  float *dx_in = nullptr, *dx_in_colsum = nullptr;  // dx_in may alias dx_out; dx_in_colsum: the db2 of the layer below
  void* dx_in_lo = nullptr;
  // avf_layer_bwd_pos / avf_layer_bwd_dx_pos, the bottom layer of a fused stack: LayerNorm-1 backward runs token-major and writes
  // d pos_embedding [N, D] instead of dx_in / dx_in_lo, which are then not asked for
  float* d_pos = nullptr;
  // dw_block / dw_desc (both or neither): the weight gradients and the column folds of the layer are NOT launched - their
  // operands stay in dw_block and dw_desc describes them for avf_layers_dw
  void* dw_block = nullptr;
  DwDeferred* dw_desc = nullptr;
};

// One backward call: what it knows (settled once by begin, resolve_gy and plan_dw) and its phases, in the order of layer_bwd_impl.
struct LayerBwd {
  Dims d;
  hipStream_t s;
  const avf_layer_params* p;
  const avf_layer_grads* g;
  LayerBwdIO io;
  Saved sv;
  LayerW W;
  Work w;
  Drops dr;  // the Linears behind a dropout site see the masked, rescaled gradient (the residual stream does not)
  bool lo;         // bf16 compute
  bool small_bwd;  // the short-sequence layer: two fused kernels around the attention backward (layer_small.hip)
  // incoming gradient as the Linears see it: gy (GEMM operand in the compute dtype, masked by site 2 under dropout; its MX-FP8
  // image in mx8_bwd); gsd: gy_stream is the unmasked bf16 stream, LayerNorm-2 backward's residual gradient
  Act gy;
  const void* gy_stream;
  bool own_copy;   // gy was made here from dx_out (so it carries this layer's site-2 mask, and db2 may sum it)
  bool gm_masked;  // gsd behind a real to_out: a separate masked image of dx_mid exists (site 0)
  bool f32_drop;   // fp32 mode with live dropout: net.3 / to_out see masked fp32 copies of dx_out / dx_mid
  bool f32_drop0;  // ... the second one only behind a real to_out (no site 0 behind nn.Identity)
  const void* gm;  // dx_mid as to_out sees it
  void *inq, *ins;  // mx8_bwd: where LayerNorm-1 backward writes the image of dx_in (behind the bf16 one in the caller's buffer)
  // the four dW GEMMs as ONE grouped launch at the end of the layer (bf16: `grouped`, which also defers the layer's column
  // folds to that launch's fold) or right after the attention backward (parity mode, bf16x3 arithmetic: `grouped32`)
  TnGroupArgs grp;
  bool grouped, grouped32;
  FoldList folds;  // db1 | dgamma2, dbeta2, dbo | dgamma1, dbeta1, the db2 of the layer below
  bool dw_grouped() const { return grouped || grouped32; }
  FoldJob* ln_fold(int j) { return dw_grouped() ? &folds.job[j] : nullptr; }

  int begin(const avf_layer_cfg* cfg, const avf_layer_params* params, const void* lowp, const avf_layer_grads* grads,
            const LayerBwdIO& caller, void* workspace, void* stream);
  int resolve_gy(), plan_dw(), db2(), small(), mlp_half(), attn_half(), ln1(), finish();
};

// validate the call, carve the buffers, settle what depends on the configuration alone
int LayerBwd::begin(const avf_layer_cfg* cfg, const avf_layer_params* params, const void* lowp, const avf_layer_grads* grads,
                    const LayerBwdIO& caller, void* workspace, void* stream) {
  AVF_TRY(make_dims(cfg, &d));
  p = params; g = grads; io = caller;
  s = (hipStream_t)stream;
  AVF_REQUIRE(!io.d_pos || (stack_ends_mode_ok(d) && layernorm_bwd_tok_ok(d.B, d.N, d.D) && !io.dx_in && !io.dx_in_lo && !io.dx_in_colsum),
              "layer_bwd_pos: needs the all-bf16 streams without dropout, fp8 or mask, a batch within the token-major rule (ask "
              "avf_layer_bwd_pos_ok first) and no dx_in outputs");
  AVF_REQUIRE(!io.dw_desc || (io.dw_block && dw_defer_mode_ok(d) && ((uintptr_t)io.dw_block & 255) == 0),
              "layer_bwd_dx: this mode keeps its weight gradients in the layer (ask avf_layer_dw_defer_ok first), or the "
              "operand block is missing / not 256-byte aligned");
  AVF_REQUIRE(p && io.x_in && io.saved && g && workspace, "layer_bwd: null pointer");
  // bf16 gradient stream: the incoming gradient may come as its bf16 image alone, and the fp32 dx_in is optional (a caller
  // asks for it only where it consumes it, e.g. below the bottom layer)
  AVF_REQUIRE(d.gs16 ? (io.dx_out || io.dx_out_lo) && (io.dx_in || io.dx_in_lo || io.d_pos) : (io.dx_out && io.dx_in),
              "layer_bwd: null gradient pointer");
  AVF_REQUIRE(!d.gs16 || io.dx_in_lo || io.d_pos, "layer_bwd(grad_stream_bf16): dx_in_lo missing");
  AVF_REQUIRE(d.dt == AVF_F32 || lowp, "layer_bwd(bf16): lowp weights missing");
  carve_saved(d, (void*)io.saved, &sv);
  carve_lowp(d, (void*)lowp, &W, p);
  carve_work(d, workspace, &w);
  if (io.dw_desc) carve_dw_block(d, io.dw_block, &w);
  lo = d.dt == AVF_BF16;
  dr = make_drops(d);
  // short sequences (the reference's 12-token stacks): the six dependent launches around the attention backward run as two
  // fused kernels (layer_small.hip), which also make the bf16 image of the incoming gradient when the caller gave none
  small_bwd = small_bwd_taken(d);
  if (d.mxb && io.dx_in_lo) {
    inq = (char*)io.dx_in_lo + grad_q_off(d.R, d.D);
    ins = (char*)io.dx_in_lo + grad_s_off(d.R, d.D);
  }
  return 0;
}

// the gradient of the layer output in the compute dtype (GEMM operand), from whichever form the caller brought
int LayerBwd::resolve_gy() {
  const void* x = io.dx_out;  // the operand
  if (lo) {
    if (io.dx_out_lo && d.gsd) {  // [stream | masked by this layer's site-2 mask] - written by the layer above's LayerNorm-1 backward
      gy_stream = io.dx_out_lo;
      x = (const char*)io.dx_out_lo + grad_q_off(d.R, d.D);
    } else if (io.dx_out_lo) x = io.dx_out_lo;  // the caller's previous call already applied this layer's site-2 mask
    else if (small_bwd) x = w.dx_out_lo;  // written by the fused kernel (small)
    else {
      AVF_TRY(cast_f32_to_bf16(io.dx_out, w.dx_out_lo, d.R * d.D, s, dr.site2));
      x = w.dx_out_lo;
      own_copy = true;
      if (d.gsd) {  // top of the stack: the stream image beside the masked one
        AVF_TRY(cast_f32_to_bf16(io.dx_out, w.dx_out_s, d.R * d.D, s, kNoDrop));
        gy_stream = w.dx_out_s;
      }
    }
  }
  AVF_REQUIRE(!d.gsd || !small_bwd, "layer_bwd: grad_stream_bf16 with dropout on a short-sequence layer (internal error)");
  gm_masked = d.gsd && d.p0 > 0.f;
  f32_drop = !lo && d.p > 0.f;
  if (f32_drop) {  // net.3 sees the gradient through its site-2 mask
    AVF_TRY(mask_copy_f32(io.dx_out, w.gy_m, d.R * d.D, s, dr.site2));
    x = w.gy_m;
    own_copy = true;
  }
  f32_drop0 = f32_drop && d.p0 > 0.f;
  gm = lo ? (gm_masked ? (const void*)w.dx_mid_m : (const void*)w.dx_mid_lo)
          : (f32_drop0 ? (const void*)w.gm_m : (const void*)w.dx_mid);
  gy = Act{x, nullptr, nullptr};
  if (d.mxb && d.gy_mx && io.dx_out_lo) {  // the image rides behind the bf16 one; else mlp_half quantises gy
    gy.q = (const char*)io.dx_out_lo + grad_q_off(d.R, d.D);
    gy.s = (const char*)io.dx_out_lo + grad_s_off(d.R, d.D);
  }
  return 0;
}

// the weight-gradient group (all operands stay alive in the workspace until the end of the layer) and whether it can launch as one
int LayerBwd::plan_dw() {
  grp = dw_group(d);
  dw_problem(grp, kQkv, w.dqkv, sv.h1, g->w_qkv);
  dw_problem(grp, kOut, gm, sv.o, g->w_out);
  dw_problem(grp, kMlp1, w.du, sv.h2, g->w1);
  dw_problem(grp, kMlp2, gy.x, sv.g, g->w2);
  grp.workspace = w.gemm_ws;
  // parity mode, bf16x3 arithmetic (round 6): the four fp32 weight gradients as one launch + one fold, issued right after
  // the attention backward - the last point where every operand exists and dx_out (which dx_in may alias) is still intact
  grouped32 = !lo && !small_bwd && gemm_f32x3_tn_group_ok(grp);
  // bf16 mode: when the shapes allow the LDS-DMA kernel
  grouped = lo && gemm_bf16_tn_group_ok(grp);
  folds.count = 3;
  AVF_REQUIRE(!io.dw_desc || (grouped && !small_bwd), "layer_bwd_dx: the layer's weight gradients do not form a grouped launch "
              "(rows %% 64, widths %% 8, 16-byte aligned operands)");
  return 0;
}

// db2 = column sums of dx_out: handed over by the caller (the next layer's LN1 backward produced them) or summed here
// (the caller normally points the previous call's dx_in_colsum straight at this layer's b2 slot: nothing to do)
int LayerBwd::db2() {
  float* out = g->b2;
  if (io.dx_out_colsum && io.dx_out_colsum != out)
    AVF_REQUIRE(hipMemcpyAsync(out, io.dx_out_colsum, (size_t)d.D * 4, hipMemcpyDeviceToDevice, s) == hipSuccess,
                "layer_bwd: memcpy failed");
  else if (!io.dx_out_colsum) {
    if (d.p > 0.f) {  // db2 sums the MASKED gradient (short sequences: the image the fused kernel has just written / read)
      AVF_REQUIRE(own_copy || small_bwd, "layer_bwd: with dropout pass dx_out_colsum together with dx_out_lo");
      AVF_TRY(colsum(gy.x, d.dt, d.R, d.D, d.D, out, w.cs_ws, s));
    } else if (io.dx_out) {
      AVF_TRY(colsum(io.dx_out, AVF_F32, d.R, d.D, d.D, out, w.cs_ws, s));
    } else {
      AVF_TRY(colsum(gy.x, AVF_BF16, d.R, d.D, d.D, out, w.cs_ws, s));
    }
  }
  return 0;
}

// the short-sequence layer: kernel A (feed-forward half up to d_o), db2, the attention backward (inside kernel B for up to 16
// heads), kernel B (dh1, LayerNorm-1 backward); its per-clip partial rows become the layer's three folds
int LayerBwd::small() {
  float* pb1 = w.small_part;
  float* pln2 = pb1 + (size_t)d.B * d.M;
  float* pln1 = pln2 + (size_t)d.B * 3 * d.D;
  SmallBwdAHost ha;
  ha.dx_out = io.dx_out; ha.dx_out_lo = io.dx_out_lo; ha.gy_store = io.dx_out_lo ? nullptr : w.dx_out_lo; ha.x_mid = (const float*)sv.x_mid;
  ha.u = sv.u; ha.ln2_w = p->ln2_w; ha.mean2 = sv.mean2; ha.rstd2 = sv.rstd2;
  ha.w2_t = W.lin[kMlp2].lo_t; ha.w1_t = W.lin[kMlp1].lo_t; ha.wo_t = W.lin[kOut].lo_t; ha.dx_mid = d.gs16 ? nullptr : w.dx_mid;
  ha.du = w.du; ha.dx_mid_lo = w.dx_mid_lo; ha.d_o = w.d_o; ha.pb1 = pb1; ha.pln2 = pln2; ha.gs16 = d.gs16 ? 1 : 0;
  ha.dr0 = dr.site0; ha.dr1 = dr.site1; ha.dr2 = dr.site2;
  AVF_TRY(layer_bwd_small_a(d.B, d.N, d.D, d.I, d.M, ha, s));
  AVF_TRY(db2());
  const bool fuse_att = small_att_fused(d);
  if (!fuse_att)
    AVF_TRY(attn_bwd_bf16((const bf16*)sv.qkv, (const bf16*)sv.o, (const bf16*)w.d_o, sv.lse2, (bf16*)w.dqkv, w.delta,
                          d.B, d.N, d.H, d.dh, s, /*q_prescaled=*/true));
  SmallBwdBHost hb;
  hb.attention = fuse_att ? 1 : 0;
  hb.qkv = sv.qkv; hb.o = sv.o; hb.d_o = w.d_o; hb.lse2 = sv.lse2; hb.H = d.H;
  {  // P = exp2(s c - lse2); dq = scale dS k; dk = scale dS^T q = dS^T q' / log2(e) when q' = q log2(e) scale (attn_bf16.hip)
    const float scale = 1.0f / sqrtf((float)d.dh), log2e = 1.4426950408889634f;
    hb.score_scale = 1.0f;
    hb.dq_scale = scale;
    hb.dk_scale = 1.0f / log2e;
  }
  hb.dqkv = w.dqkv; hb.wqkv_t = W.lin[kQkv].lo_t; hb.x_in = (const float*)io.x_in; hb.ln1_w = p->ln1_w; hb.mean1 = sv.mean1;
  hb.rstd1 = sv.rstd1; hb.dx_mid = d.gs16 ? nullptr : w.dx_mid; hb.dx_mid_lo = w.dx_mid_lo; hb.dx_in = io.dx_in; hb.dx_in_lo = io.dx_in_lo;
  hb.pln1 = pln1; hb.gs16 = d.gs16 ? 1 : 0; hb.dr_prev2 = dr.prev2;
  AVF_TRY(layer_bwd_small_b(d.B, d.N, d.D, d.I, hb, s));
  folds.job[0] = FoldJob{pb1, d.B, d.M, d.M, g->b1, nullptr, nullptr};
  folds.job[1] = FoldJob{pln2, d.B, 3 * d.D, d.D, g->ln2_w, g->ln2_b, g->b_out};
  folds.job[2] = FoldJob{pln1, d.B, 3 * d.D, d.D, g->ln1_w, g->ln1_b, io.dx_in_colsum};
  return 0;
}

// ---- feed-forward half: db2, dW2, du (+ db1), dh2, LayerNorm-2 backward (dx_mid, dgamma2, dbeta2, dbo), dW1 ---------------------
int LayerBwd::mlp_half() {
  const LinearW &mlp1 = W.lin[kMlp1], &mlp2 = W.lin[kMlp2];
  AVF_TRY(db2());
  if (!dw_grouped()) AVF_TRY(linear_dw(d, mlp2, gy.x, sv.g, g->w2, w.gemm_ws, s));
  // config 5, backward half: the three dX GEMMs whose A operand leaves a row-wise producer (LayerNorm backward of this /
  // the next layer, the dGELU epilogue) read MX-FP8 images written by that producer; dqkv -> dh1 (A produced per head by the
  // attention backward) and the four weight-gradient GEMMs (reduction over tokens, not features) stay bf16
  if (d.mxb && !gy.q) {  // top of the stack (or a caller without the image): one quantiser pass over the bf16 gradient
    AVF_TRY(quant_mx8(gy.x, AVF_BF16, d.D, d.R, d.D, w.gyq, d.D, w.gys, s));
    gy.q = w.gyq; gy.s = w.gys;
  }
  // Where the weight-stationary bf16 kernel takes the shape it is the faster form of the dGELU launch even in the fp8 mode (C5:
  // 49 us against 70 on MX-FP8 operands - the launch is bound by the 168 MB it reads and writes beside the operands, which fp8
  // does not touch); it emits the same image of du
  const bool dgelu_ws_first = d.mxb;
  // du = (gy W2) * gelu'(u), with the image of du for the fp8 GEMM behind it (mx8_bwd); bf16: db1 = colsum(du) fused into the epilogue
  GemmArgs e_dgelu;
  e_dgelu.epilogue = AVF_EPI_DGELU; e_dgelu.aux = sv.u; e_dgelu.drop = dr.site1; e_dgelu.mx_q = w.duq; e_dgelu.mx_s = w.dus;
  if (lo) { e_dgelu.colsum = g->b1; e_dgelu.workspace = w.cs_ws; e_dgelu.defer_fold = grouped ? &folds.job[0] : nullptr; }
  AVF_TRY(linear_dx(d, mlp2, gy, w.du, e_dgelu, s, dgelu_ws_first));
  if (!lo) AVF_TRY(colsum(w.du, d.dt, d.R, d.M, d.M, g->b1, w.cs_ws, s));
  AVF_TRY(linear_dx(d, mlp1, Act{w.du, w.duq, w.dus}, w.dh, GemmArgs{}, s));
  if (d.gs16)  // residual gradient in: the bf16 image the GEMMs read (gsd: the unmasked stream); out: the bf16 dx_mid only
    AVF_TRY(layernorm_bwd(w.dh, d.dt, sv.x_mid, p->ln2_w, sv.mean2, sv.rstd2, d.gsd ? gy_stream : gy.x, nullptr, w.dx_mid_lo,
                          g->ln2_w, g->ln2_b, g->b_out, w.ln_ws, d.R, d.D, s, dr.site0, ln_fold(1), AVF_BF16,
                          d.xdt, w.mq, w.ms, gm_masked ? w.dx_mid_m : nullptr));
  else
    AVF_TRY(layernorm_bwd(w.dh, d.dt, sv.x_mid, p->ln2_w, sv.mean2, sv.rstd2, io.dx_out, w.dx_mid,
                          lo ? w.dx_mid_lo : nullptr, g->ln2_w, g->ln2_b, g->b_out, w.ln_ws, d.R, d.D, s, dr.site0,
                          ln_fold(1), AVF_F32, d.xdt, w.mq, w.ms));
  if (!dw_grouped()) AVF_TRY(linear_dw(d, mlp1, w.du, sv.h2, g->w1, w.gemm_ws, s));
  return 0;
}

// ---- attention half: dWo, d_o, the attention backward (dqkv), the parity mode's grouped dW, dh1 -------------------------------
int LayerBwd::attn_half() {
  if (f32_drop0) AVF_TRY(mask_copy_f32(w.dx_mid, w.gm_m, d.R * d.D, s, dr.site0));  // to_out sees dx_mid through its site-0 mask
  if (!dw_grouped()) AVF_TRY(linear_dw(d, W.lin[kOut], gm, sv.o, g->w_out, w.gemm_ws, s));
  AVF_TRY(linear_dx(d, W.lin[kOut], Act{gm, w.mq, w.ms}, w.d_o, GemmArgs{}, s));
  // dqkv -> dh1 on MX-FP8 operands, the image of dqkv written by the merged attention backward (DESIGN_HISTORY.md section 17, item 5):
  // built and bit-exact, but the image costs the attention kernel 18 us at B = 64, N = 512 (50 us before its stores were
  // made 16 bytes wide and dQ's 32-blocks wave-local) while the K = 1536 GEMM, already at 0.87 PFLOP/s on bf16 operands,
  // gains ~9 us: C5 5.06 ms per step with it against 4.93 without - OFF unless AVF_MX8_DQKV=1.
  const int dq_mx_on = tuning_int("AVF_MX8_DQKV", 0);  // (read per call: a test flips it inside one process)
  const bool dq_mx = d.mxb && dq_mx_on && !d.keep && (3 * d.I) % 128 == 0 && d.D % 128 == 0 &&
                     attn_bwd_emits_mx8(d.N, d.dh, /*q_prescaled=*/true);
  if (d.keep && lo && !d.mx)  // (attn_bwd_masked_bf16 chooses as the forward's attn_fwd_masked_bf16 did)
    AVF_TRY(attn_bwd_masked_bf16(sv.qkv, sv.o, w.d_o, sv.lse2, w.dqkv, w.delta, d.keep, d.B, d.N, d.H, d.dh, s,
                                 /*q_prescaled=*/true));
  else if (d.keep)
    AVF_TRY(attn_bwd_vec(d.dt, sv.qkv, sv.o, w.d_o, sv.lse2, w.dqkv, w.delta, d.B, d.N, d.H, d.dh, s, d.keep,
                         /*q_prescaled=*/lo, d.arith));
  else if (lo)
    AVF_TRY(attn_bwd_bf16((const bf16*)sv.qkv, (const bf16*)sv.o, (const bf16*)w.d_o, sv.lse2, (bf16*)w.dqkv, w.delta,
                          d.B, d.N, d.H, d.dh, s, /*q_prescaled=*/true, nullptr, dq_mx ? w.dqq : nullptr, dq_mx ? w.dqs : nullptr));
  else
    AVF_TRY(attn_bwd_f32((const float*)sv.qkv, (const float*)sv.o, (const float*)w.d_o, sv.lse2, (float*)w.dqkv,
                         w.delta, d.B, d.N, d.H, d.dh, s, d.arith));
  if (grouped32) AVF_TRY(gemm_f32x3_tn_group(grp, s));
  // dh1 = dqkv Wqkv (dq_mx: on MX-FP8 operands, the image of dqkv left the attention backward's epilogue)
  return linear_dx(d, W.lin[kQkv], Act{w.dqkv, dq_mx ? w.dqq : nullptr, dq_mx ? w.dqs : nullptr}, w.dh, GemmArgs{}, s);
}

// ---- LayerNorm-1 backward (dx_in or d pos_embedding, dgamma1, dbeta1, the db2 of the layer below), then dWqkv -------------------
// dx_in may alias dx_out, which the grouped dW2 GEMM does not read (it uses the copy gy)
int LayerBwd::ln1() {
  if (io.d_pos)
    AVF_TRY(layernorm_bwd_tok(w.dh, io.x_in, p->ln1_w, sv.mean1, sv.rstd1, w.dx_mid_lo, io.d_pos, g->ln1_w, g->ln1_b, w.ln_ws1, d.B,
                              d.N, d.D, s, ln_fold(2)));
  else if (d.gs16)  // (gsd: the masked image for the layer below goes behind the stream in dx_in_lo; layer 0 has no site below it)
    AVF_TRY(layernorm_bwd(w.dh, d.dt, io.x_in, p->ln1_w, sv.mean1, sv.rstd1, w.dx_mid_lo, io.dx_in, io.dx_in_lo, g->ln1_w, g->ln1_b,
                          io.dx_in_colsum, w.ln_ws1, d.R, d.D, s, dr.prev2, ln_fold(2), AVF_BF16, d.xdt, inq, ins,
                          (d.gsd && dr.prev2.thresh16) ? (char*)io.dx_in_lo + grad_q_off(d.R, d.D) : nullptr));
  else
    AVF_TRY(layernorm_bwd(w.dh, d.dt, io.x_in, p->ln1_w, sv.mean1, sv.rstd1, w.dx_mid, io.dx_in, lo ? io.dx_in_lo : nullptr,
                          g->ln1_w, g->ln1_b, io.dx_in_colsum, w.ln_ws1, d.R, d.D, s, dr.prev2, ln_fold(2), AVF_F32, d.xdt,
                          inq, ins));
  if (!dw_grouped()) AVF_TRY(linear_dw(d, W.lin[kQkv], w.dqkv, sv.h1, g->w_qkv, w.gemm_ws, s));
  return 0;
}

// the weight gradients that were not launched on the way, and the layer's column folds
int LayerBwd::finish() {
  if (io.dw_desc) {  // deferred: describe the group and the folds for avf_layers_dw
    DwDeferred* dd = io.dw_desc;
    dd->magic = kDwDescMagic;
    dd->grp = grp; dd->grp.workspace = nullptr;
    for (int j = 0; j < 3; ++j) dd->folds[j] = folds.job[j];
    return 0;
  }
  // one launch folds the split-K slabs of the four weight gradients and the three deferred column folds
  // (db1; dgamma2/dbeta2/dbo; dgamma1/dbeta1/previous layer's db2)
  if (grouped) return gemm_bf16_tn_group(grp, s, &folds);
  if (grouped32) return fold_list(folds, s);  // the two LayerNorm column folds of the layer in one launch (job 0 stays empty)
  if (small_bwd) {  // (the general path has launched its single dW GEMMs and folds where their operands appeared)
    AVF_TRY(linear_dw(d, W.lin[kMlp2], gy.x, sv.g, g->w2, w.gemm_ws, s));
    AVF_TRY(linear_dw(d, W.lin[kMlp1], w.du, sv.h2, g->w1, w.gemm_ws, s));
    AVF_TRY(linear_dw(d, W.lin[kOut], gm, sv.o, g->w_out, w.gemm_ws, s));
    AVF_TRY(linear_dw(d, W.lin[kQkv], w.dqkv, sv.h1, g->w_qkv, w.gemm_ws, s));
    for (int j = 0; j < 3; ++j) AVF_TRY(fold_job(folds.job[j], s));
  }
  return 0;
}

static int layer_bwd_impl(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const avf_layer_grads* g,
                          const LayerBwdIO& io, void* workspace, void* stream) {
  LayerBwd b{};
  AVF_TRY(b.begin(cfg, p, lowp, g, io, workspace, stream));
  AVF_TRY(b.resolve_gy());
  AVF_TRY(b.plan_dw());
  if (b.small_bwd) {
    AVF_TRY(b.small());
  } else {
    AVF_TRY(b.mlp_half());
    AVF_TRY(b.attn_half());
    AVF_TRY(b.ln1());
  }
  return b.finish();
}

extern "C" int avf_layer_bwd(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                             const void* saved, const float* dx_out, const void* dx_out_lo,
                             const float* dx_out_colsum, float* dx_in, void* dx_in_lo, float* dx_in_colsum,
                             const avf_layer_grads* g, void* workspace, void* stream) {
  LayerBwdIO io;
  io.x_in = x_in; io.saved = saved; io.dx_out = dx_out; io.dx_out_lo = dx_out_lo; io.dx_out_colsum = dx_out_colsum;
  io.dx_in = dx_in; io.dx_in_lo = dx_in_lo; io.dx_in_colsum = dx_in_colsum;
  return layer_bwd_impl(cfg, p, lowp, g, io, workspace, stream);
}

// ---- deferred weight gradients: the dX chain of a layer now, the dW groups of several layers in one launch later ----------------
extern "C" int avf_layer_dw_defer_ok(const avf_layer_cfg* cfg, int* tiles_per_layer, int* slots) {
  Dims d;
  if (make_dims(cfg, &d) || !dw_defer_mode_ok(d) || d.R % 64 != 0) return 0;
  const TnGroupArgs ga = dw_group(d);
  if (!gemm_bf16_tn_group_ok(ga)) return 0;
  int t = 0, sl = 0;
  gemm_bf16_tn_group_plan(ga, &t, &sl);
  if (tiles_per_layer) *tiles_per_layer = t;
  if (slots) *slots = sl;
  return 1;
}
extern "C" int avf_layers_dw_max(void) { return kTnGroupMax / 4; }
extern "C" size_t avf_layer_dw_block_bytes(const avf_layer_cfg* cfg) {
  Dims d;
  if (make_dims(cfg, &d) || !dw_defer_mode_ok(d)) return 0;
  return align_up(carve_dw_block(d, nullptr, nullptr), 256);
}
extern "C" size_t avf_layer_dw_desc_bytes(void) { return sizeof(DwDeferred); }

// the bottom layer of a fused stack when only d pos_embedding is wanted below it (LayerBwdIO::d_pos)
extern "C" int avf_layer_bwd_pos(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                                 const void* saved, const float* dx_out, const void* dx_out_lo, const float* dx_out_colsum,
                                 float* d_pos, const avf_layer_grads* g, void* workspace, void* stream) {
  AVF_REQUIRE(d_pos, "layer_bwd_pos: null d_pos");
  LayerBwdIO io;
  io.x_in = x_in; io.saved = saved; io.dx_out = dx_out; io.dx_out_lo = dx_out_lo; io.dx_out_colsum = dx_out_colsum;
  io.d_pos = d_pos;
  return layer_bwd_impl(cfg, p, lowp, g, io, workspace, stream);
}
extern "C" int avf_layer_bwd_dx_pos(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                                    const void* saved, const float* dx_out, const void* dx_out_lo, const float* dx_out_colsum,
                                    float* d_pos, const avf_layer_grads* g, void* workspace, void* dw_block, void* dw_desc,
                                    void* stream) {
  AVF_REQUIRE(d_pos && dw_block && dw_desc, "layer_bwd_dx_pos: null d_pos / operand block / descriptor");
  LayerBwdIO io;
  io.x_in = x_in; io.saved = saved; io.dx_out = dx_out; io.dx_out_lo = dx_out_lo; io.dx_out_colsum = dx_out_colsum;
  io.d_pos = d_pos; io.dw_block = dw_block; io.dw_desc = (DwDeferred*)dw_desc;
  return layer_bwd_impl(cfg, p, lowp, g, io, workspace, stream);
}

extern "C" int avf_layer_bwd_dx(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                                const void* saved, const float* dx_out, const void* dx_out_lo,
                                const float* dx_out_colsum, float* dx_in, void* dx_in_lo, float* dx_in_colsum,
                                const avf_layer_grads* g, void* workspace, void* dw_block, void* dw_desc, void* stream) {
  AVF_REQUIRE(dw_block && dw_desc, "layer_bwd_dx: null operand block / descriptor");
  LayerBwdIO io;
  io.x_in = x_in; io.saved = saved; io.dx_out = dx_out; io.dx_out_lo = dx_out_lo; io.dx_out_colsum = dx_out_colsum;
  io.dx_in = dx_in; io.dx_in_lo = dx_in_lo; io.dx_in_colsum = dx_in_colsum;
  io.dw_block = dw_block; io.dw_desc = (DwDeferred*)dw_desc;
  return layer_bwd_impl(cfg, p, lowp, g, io, workspace, stream);
}

// the group over the layers of `descs` (the order given: top layer first), each layer attention half | MLP half
static int layers_dw_group(const avf_layer_cfg* cfgs, int n_layers, const void* const* descs, TnGroupArgs* grp, FoldList* fl) {
  AVF_REQUIRE(cfgs && n_layers >= 1 && n_layers <= kTnGroupMax / 4, "layers_dw: 1..%d layers per group", kTnGroupMax / 4);
  memset(grp, 0, sizeof(*grp));
  if (fl) memset(fl, 0, sizeof(*fl));
  for (int l = 0; l < n_layers; ++l) {
    Dims d;
    AVF_TRY(make_dims(&cfgs[l], &d));
    AVF_REQUIRE(dw_defer_mode_ok(d), "layers_dw: layer %d is in a mode that keeps its weight gradients in the layer", l);
    TnGroupArgs one;
    if (descs) {
      const DwDeferred* dd = (const DwDeferred*)descs[l];
      AVF_REQUIRE(dd && dd->magic == kDwDescMagic, "layers_dw: descriptor %d was not written by avf_layer_bwd_dx", l);
      one = dd->grp;
      AVF_REQUIRE(one.K == d.R, "layers_dw: descriptor %d belongs to another configuration", l);
      for (int j = 0; j < 3; ++j) fl->job[3 * l + j] = dd->folds[j];
    } else {
      one = dw_group(d);
    }
    AVF_REQUIRE(l == 0 || one.K == grp->K, "layers_dw: the layers of a group share their token rows");
    grp->K = one.K;
    for (int i = 0; i < 4; ++i) {
      const int q = 4 * l + i;
      grp->A[q] = one.A[i]; grp->B[q] = one.B[i]; grp->C[q] = one.C[i];
      grp->M[q] = one.M[i]; grp->N[q] = one.N[i]; grp->lda[q] = one.lda[i]; grp->ldb[q] = one.ldb[i];
    }
  }
  grp->count = 4 * n_layers;
  if (fl) fl->count = 3 * n_layers;
  return 0;
}
extern "C" size_t avf_layers_dw_workspace_bytes(const avf_layer_cfg* cfgs, int n_layers) {
  TnGroupArgs grp;
  if (layers_dw_group(cfgs, n_layers, nullptr, &grp, nullptr)) return 0;
  return gemm_bf16_tn_group_ws(grp);
}
extern "C" int avf_layers_dw(const avf_layer_cfg* cfgs, int n_layers, const void* const* descs, void* workspace,
                             size_t workspace_bytes, void* stream) {
  AVF_REQUIRE(descs, "layers_dw: null descriptors");
  TnGroupArgs grp;
  FoldList fl;
  AVF_TRY(layers_dw_group(cfgs, n_layers, descs, &grp, &fl));
  AVF_REQUIRE(gemm_bf16_tn_group_ok(grp), "layers_dw: the group does not fit the grouped launch");
  const size_t need = gemm_bf16_tn_group_ws(grp);
  AVF_REQUIRE(need == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need),
              "layers_dw: split-K workspace missing or too small (%zu bytes given, %zu needed)", workspace_bytes, need);
  grp.workspace = workspace;
  return gemm_bf16_tn_group(grp, (hipStream_t)stream, &fl);  // + the slab fold with the column folds, or the column folds alone
}
