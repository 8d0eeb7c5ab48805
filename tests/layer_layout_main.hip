// Stand-alone host program (no GPU): prints the byte offset of every piece that layer.hip carves out of a layer's lowp, saved and
// workspace buffers, one "<configuration> <buffer>.<piece> <offset>" line each (-1: the mode keeps no such piece).
// tests/test_layer_sizes_cpu.py compiles it against the built library and compares the lines with recorded ones: the Adam kernels
// and the Python side find images by offset, and a reordering of equal-sized pieces does not show in the size queries.
#include <cstdio>

#include "layer.hip"

static char* const kBase = (char*)(uintptr_t)(1 << 20);
static void show(const char* cfg, const char* piece, const void* p) {
  printf("%s %s %lld\n", cfg, piece, p ? (long long)((const char*)p - kBase) : -1LL);
}
#define SHOW(s, f) show(name, #s "." #f, s.f)

static void layout(const char* name, avf_layer_cfg c) {
  Dims d;
  if (make_dims(&c, &d)) {
    printf("%s invalid\n", name);
    return;
  }
  LayerW W;
  carve_lowp(d, kBase, &W);
  const char* lin[kLinears] = {"qkv", "out", "mlp1", "mlp2"};
  for (int i = 0; i < kLinears; ++i) {
    const LinearW& L = W.lin[i];
    const void* img[8] = {L.lo, L.lo_t, L.q, L.s, L.tq, L.ts, L.p, L.tp};
    const char* what[8] = {"lo", "lo_t", "q", "s", "tq", "ts", "p", "tp"};
    char piece[32];
    for (int k = 0; k < 8; ++k) {
      snprintf(piece, sizeof(piece), "lowp.%s.%s", lin[i], what[k]);
      show(name, piece, img[k]);
    }
  }
  Saved sv;
  carve_saved(d, kBase, &sv);
  SHOW(sv, h1); SHOW(sv, mean1); SHOW(sv, rstd1); SHOW(sv, qkv); SHOW(sv, o); SHOW(sv, lse2); SHOW(sv, x_mid); SHOW(sv, h2);
  SHOW(sv, mean2); SHOW(sv, rstd2); SHOW(sv, u); SHOW(sv, g);
  Work w;
  carve_work(d, kBase, &w);
  SHOW(w, du); SHOW(w, dh); SHOW(w, d_o); SHOW(w, dqkv); SHOW(w, dx_mid); SHOW(w, dx_mid_lo); SHOW(w, dx_out_lo); SHOW(w, delta);
  SHOW(w, ln_ws); SHOW(w, ln_ws1); SHOW(w, cs_ws); SHOW(w, gemm_ws); SHOW(w, small_part); SHOW(w, hq); SHOW(w, hs); SHOW(w, gq);
  SHOW(w, gs); SHOW(w, oq); SHOW(w, os); SHOW(w, duq); SHOW(w, dus); SHOW(w, mq); SHOW(w, ms); SHOW(w, gyq); SHOW(w, gys);
  SHOW(w, dqq); SHOW(w, dqs); SHOW(w, dx_out_s); SHOW(w, dx_mid_m); SHOW(w, gy_m); SHOW(w, gm_m);
  Work b = w;
  carve_dw_block(d, kBase, &b);
  show(name, "dw_block.du", b.du); show(name, "dw_block.dqkv", b.dqkv); show(name, "dw_block.dx_mid_lo", b.dx_mid_lo);
  show(name, "dw_block.dx_out_lo", b.dx_out_lo); show(name, "dw_block.ln_ws", b.ln_ws); show(name, "dw_block.ln_ws1", b.ln_ws1);
  show(name, "dw_block.cs_ws", b.cs_ws);
}

static avf_layer_cfg cfg(int B, int N, int D, int H, int dh, int M, int dtype, float p) {
  avf_layer_cfg c{};
  c.batch = B; c.tokens = N; c.dim = D; c.heads = H; c.dim_head = dh; c.mlp_dim = M; c.dtype = dtype;
  c.project_out = 1; c.ln_eps = 1e-5f; c.dropout_p = p;
  return c;
}

int main() {
  avf_layer_cfg c = cfg(2, 64, 512, 8, 64, 1024, AVF_BF16, 0.f);  // the weight-stationary images exist (K = 512)
  c.grad_stream_bf16 = 1; c.resid_bf16 = 1;
  layout("bf16_k512", c);
  c.resid_bf16 = 0; c.mx8_fwd = 1; c.mx8_bwd = 1; c.dx_out_mx8 = 1;  // every MX-FP8 image; sizes of Wo, W1 / W2 and Wqkv all differ
  layout("mx8_k512", c);
  c = cfg(2, 64, 128, 4, 64, 384, AVF_BF16, 0.f);  // inner 256 != dim: Wo is not square
  c.grad_stream_bf16 = 1; c.mx8_fwd = 1;
  layout("mx8_fwd_inner256", c);
  c = cfg(2, 100, 128, 2, 64, 256, AVF_BF16, 0.1f);  // all-bf16 streams with live dropout: the two-image hand-off buffers
  c.grad_stream_bf16 = 1; c.resid_bf16 = 1;
  layout("bf16_resid16_drop", c);
  layout("f32_drop", cfg(2, 100, 128, 2, 64, 256, AVF_F32, 0.1f));  // masked fp32 copies
  c = cfg(2, 12, 128, 4, 32, 256, AVF_BF16, 0.f);  // short-sequence layer: its partial rows
  c.grad_stream_bf16 = 1;
  layout("small_n12", c);
  return 0;
}
