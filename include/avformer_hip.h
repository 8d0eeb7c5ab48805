/* avformer_hip.h - C ABI of libavformer_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary for the transformer hot path of
 * ColinWine/Multi-modal-Multi-label-Facial-Action-Unit-Detection-with-Transformer.
 * The reference has no native layer of its own (pure PyTorch eager), so there is no FFI to mirror;
 * each entry point below cites the reference Python it replaces (paths relative to the reference
 * repository root).  Conventions:
 *
 *   - every function returns 0 on success, non-zero on error; avf_last_error() returns a
 *     thread-local message for the last failure.  Nothing throws across the boundary.
 *   - all data pointers are CALLER-OWNED DEVICE pointers (PyTorch allocates inputs, outputs,
 *     saved activations and workspaces); the library allocates nothing persistent.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *     All work is enqueued on it; no entry point synchronises the device (graph-capture safe).
 *   - activations are row-major [rows = batch*tokens, features]; the residual stream is fp32;
 *     `dtype` selects the compute/storage type of the non-residual activations:
 *     AVF_F32 (parity mode: fp32 MFMA / fp32 VALU) or AVF_BF16 (throughput mode: bf16 MFMA,
 *     fp32 accumulate, fp32 LayerNorm/softmax statistics).
 */
#ifndef AVFORMER_HIP_H
#define AVFORMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVF_F32 0
#define AVF_BF16 1

/* GEMM epilogues (avf_gemm) */
#define AVF_EPI_NONE 0      /* C = acc (+bias if given)                                           */
#define AVF_EPI_BIAS_RES 1  /* C(f32) = acc + bias + residual(f32)        heads.py:175,238,196    */
#define AVF_EPI_BIAS_GELU 2 /* aux = acc + bias ; C = tanh-GELU(aux)      heads.py:166,191-192    */
#define AVF_EPI_DGELU 3     /* C = acc * dGELU/du(aux)                    backward of heads.py:166 */

typedef struct avf_layer_cfg {
  int32_t batch;       /* clips B                                                              */
  int32_t tokens;      /* tokens per clip N                                                    */
  int32_t dim;         /* D      - Transformer(dim, ...)                  heads.py:243          */
  int32_t heads;       /* H                                               heads.py:204          */
  int32_t dim_head;    /* dh ; inner I = H*dh                             heads.py:206          *
                        * bf16 / mx8 / resid_bf16: 32, 64 or 128 (else avf_layer_* fail naming dim_head); f32: 8, 16, 32, 64, 128.
                        * Attention kernels per width: bf16 unmasked - head-resident and merged forms at 64 (<= 576 / 512 tokens),
                        * the streaming MFMA forms at 32, 64 and 128; masked calls and bf16 storage under a mask - the fp32-arithmetic
                        * kernels at 8..128 (bf16: the MFMA forms at 64, <= 512 tokens); f32 parity, unmasked - the three-product
                        * bf16x3 kernels at 64 only, the f32-input MFMA kernels at 32, 64 and 128 (dim_head 128 takes them under
                        * either arithmetic), the fp32 VALU kernels at 8 and 16. */
  int32_t mlp_dim;     /* M                                               heads.py:189          */
  int32_t dtype;       /* AVF_F32 | AVF_BF16                                                    */
  int32_t project_out; /* 0 iff heads==1 && dim_head==dim (nn.Identity)   heads.py:207: pass the identity matrix as w_out and
                          zeros as b_out (the GEMM then returns the attention output exactly); no dropout site 0 */
  float ln_eps;        /* nn.LayerNorm default 1e-5                       heads.py:181          */
  float dropout_p;     /* nn.Dropout p of the three sites (after to_out, after GELU, after net.3)
                          heads.py:194-196,216; 0 = eval()/no dropout.  p > 0 needs dim % 4 == 0, dim <= 1536.  Masks are a pure
                          function of (seed, layer_index, site, element), regenerated in backward.               */
  uint32_t seed_lo, seed_hi; /* dropout seed: use a fresh value per forward, the same one in its backward        */
  int32_t layer_index; /* position of this layer in its stack (keys the dropout masks)                          */
  const void* seed_dev; /* optional device pointer to a uint64 seed; when non-null it replaces seed_lo/hi and is read
                          by the kernels at run time, so a captured hipGraph draws fresh masks on every replay
                          (the caller advances the value between forwards, e.g. with a captured add)            */
  int32_t grad_stream_bf16; /* 1 (AVF_BF16, dropout_p == 0, dim <= 1536): avf_layer_bwd keeps the residual gradient stream in
                          bf16 - it reads the incoming gradient from dx_out_lo (dx_out may be null; if only dx_out is given it
                          is cast first), the two LayerNorm backward kernels exchange bf16 only, and the fp32 dx_in is written
                          only when the pointer is non-null (a caller passes it where it consumes fp32, e.g. for the bottom
                          layer).  Per-layer parameter gradients stay fp32.                                            */
  int32_t mx8_fwd;     /* 1 (AVF_BF16 only; dim, mlp_dim % 128 == 0): the forward GEMMs of to_qkv, net.0 and net.3 take MX-FP8
                          operands (BASELINE config 5).  The bf16 weight-image buffer then also holds their e4m3 images:
                          refresh them with avf_stack_quant_weights_mx8 whenever the bf16 images changed.          */
  int32_t resid_bf16;  /* 1 (AVF_BF16 only; dim % 8 == 0, dim <= 1536): the FORWARD residual stream is stored in bf16 - x_in, x_out of
                          avf_layer_fwd / avf_layer_bwd and the saved mid-layer stream are bf16 tensors (LayerNorm statistics,
                          GEMM accumulation and the residual add itself stay fp32; one bf16 rounding per residual add).
                          Cuts the HBM bytes of the two LayerNorms and the two residual GEMM epilogues of a layer by a third. */
  int32_t mx8_bwd;     /* 1 (needs mx8_fwd): the backward GEMMs dX = dY W of net.3, net.0 and to_out take MX-FP8 operands too: the
                          LayerNorm backward kernels and the dGELU epilogue write the e4m3 image of their output beside the bf16
                          one, avf_stack_quant_weights_mx8 also makes the images of the transposed weights.  The bf16
                          gradient-stream buffers dx_out_lo / dx_in_lo of avf_layer_bwd are then avf_layer_grad_stream_bytes()
                          long: [R, D] bf16 | [R, D] e4m3 | [R, D/32] E8M0 (each part 256-byte aligned).               */
  int32_t dx_out_mx8;  /* mx8_bwd: 1 = dx_out_lo already carries that image (it was written as the dx_in_lo of the layer
                          above by avf_layer_bwd with mx8_bwd set); 0 = the layer quantises dx_out_lo itself (top layer) */
  const void* key_mask; /* optional token mask of Transformer.forward(x, mask) (heads.py:225-232; no reference caller passes one):
                          device bytes [batch, tokens], 1 = token kept - the reference's mask padded with a leading True.  A pair
                          (i, j) with either token dropped scores -FLT_MAX: a dropped query attends uniformly to all keys, a kept
                          query gives dropped keys zero weight; no gradient flows through a filled score.  bf16 layers with
                          dim_head 64 and <= 512 tokens apply it inside the MFMA attention kernels (head-resident forward, merged
                          backward); every other case runs the attention core on the fp32-arithmetic kernels (correct, not tuned). */
  int32_t f32_arith;   /* AVF_F32: the arithmetic of every GEMM and of the attention core of THIS call, 1 = bf16x3, 0 = the f32-input
                          MFMA (the two modes of avf_set_f32_arith, below).  A layer call does not look at the process-wide default:
                          a caller hands a backward the value its forward ran under, and lse2, o and the grouped weight-gradient
                          decision then belong to the kernels that read them.  Must be 0 or 1 (AVF_BF16 ignores which). */
} avf_layer_cfg;

/* fp32 master parameters of one layer, in state_dict order:
 * layers.{i}.0.fn.norm.{weight,bias}, .0.fn.fn.to_qkv.weight [3I,D], .0.fn.fn.to_out.0.{weight [D,I],bias},
 * layers.{i}.1.fn.norm.{weight,bias}, .1.fn.fn.net.0.{weight [M,D],bias}, .1.fn.fn.net.3.{weight [D,M],bias} */
typedef struct avf_layer_params {
  const float *ln1_w, *ln1_b, *w_qkv, *w_out, *b_out, *ln2_w, *ln2_b, *w1, *b1, *w2, *b2;
} avf_layer_params;

/* gradients, same shapes; every non-null pointer is OVERWRITTEN (not accumulated) */
typedef struct avf_layer_grads {
  float *ln1_w, *ln1_b, *w_qkv, *w_out, *b_out, *ln2_w, *ln2_b, *w1, *b1, *w2, *b2;
} avf_layer_grads;

int avf_version(void);
/* sizeof(avf_layer_cfg) / sizeof(avf_layer_params) as this library was compiled: a binding checks its own struct
 * declarations against them before the first call (a shorter caller-side struct would be read past its end) */
size_t avf_sizeof_layer_cfg(void);
size_t avf_sizeof_layer_params(void);
const char* avf_last_error(void);
/* 1 if a gfx950 device is usable by this process */
int avf_device_ok(void);

/* ---- per-operator entry points --------------------------------------------------------- */

/* nn.LayerNorm(dim) forward - heads.py:178-185.  x fp32 [rows,dim] -> y (y_dtype) ; mean/rstd fp32 [rows].
 * (fp32 x only, here and in avf_layernorm_bwd; a bf16 x goes through avf_layernorm_fwd_ex / avf_layernorm_bwd_ex below) */
int avf_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype,
                      float* mean, float* rstd, int64_t rows, int dim, float eps, void* stream);

/* LayerNorm backward.  dx = dres (nullable) + LN'(dy); optional low-precision copy dx_lo (bf16, nullable);
 * dgamma/dbeta [dim]; dcolsum (nullable) = column sums of dx (bias gradient of the Linear that produced x).
 * workspace >= avf_layernorm_bwd_workspace_bytes(rows, dim). */
size_t avf_layernorm_bwd_workspace_bytes(int64_t rows, int dim);
int avf_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                      const float* rstd, const float* dres, float* dx, void* dx_lo, float* dgamma,
                      float* dbeta, float* dcolsum, void* workspace, int64_t rows, int dim, void* stream);

/* The general LayerNorm door: every storage type and option that the layer calls use (the two entry points above pin x to
 * fp32 and have no dropout).  Same math, same workspace size query.
 *   forward:  x_dtype AVF_F32 | AVF_BF16.  A bf16 x needs a bf16 y, dim % 4 == 0 and dim <= 1536 (error otherwise).
 *   backward: x_dtype / dres_dtype AVF_F32 | AVF_BF16 (dres nullable; its dtype is then ignored).  A bf16 x needs bf16 dy,
 *             dim % 4 == 0, dim <= 1536; a bf16 dres needs bf16 dy, dx_lo, dim % 4 == 0, dim <= 1536.  Outputs: dx (fp32,
 *             nullable when dim % 4 == 0 and dim <= 1536), dx_lo (bf16, nullable), dx_m (bf16, nullable), at least one of
 *             dx / dx_lo; dgamma / dbeta [dim]; dcolsum (nullable).
 *   dropout:  (seed_lo, seed_hi, layer_index, site, p) name a dropout site exactly as avf_dropout_factors does; p == 0 is
 *             no dropout.  With f = those factors and g = dres + LN'(dy) the outputs are
 *               without dx_m (one-row-per-wave kernels):   dx = g, dx_lo = bf16(f * g),                dcolsum = sum_r f * g
 *               with dx_m (all-bf16 streams, dim % 8 == 0): dx = g, dx_lo = bf16(g), dx_m = bf16(f * g), dcolsum = sum_r f * g
 *             i.e. dx is never masked, the column sums always are, and dx_lo is the masked image only when there is no dx_m.
 *             dx_m needs p > 0, bf16 dy / x / dres and dx_lo (error otherwise).
 * dgamma / dbeta / dcolsum are sums of the fp32 values (before any bf16 store), combined in a fixed order: the same inputs
 * give the same bits.  No MX-FP8 image here (see avf_layernorm_fwd_mx8 / avf_layernorm_bwd_mx8). */
int avf_layernorm_fwd_ex(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                         float* rstd, int64_t rows, int dim, float eps, void* stream);
int avf_layernorm_bwd_ex(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* gamma, const float* mean,
                         const float* rstd, const void* dres, int dres_dtype, float* dx, void* dx_lo, void* dx_m, float* dgamma,
                         float* dbeta, float* dcolsum, void* workspace, int64_t rows, int dim, uint32_t seed_lo,
                         uint32_t seed_hi, int layer_index, int site, float p, void* stream);

/* column sums (bias gradients): out[c] = sum_r in[r,c].  workspace >= avf_colsum_workspace_bytes. */
size_t avf_colsum_workspace_bytes(int64_t rows, int cols);
int avf_colsum(const void* in, int in_dtype, int64_t rows, int cols, int64_t ld, float* out, void* workspace,
               void* stream);

/* fp32 -> bf16 cast (n elements) */
int avf_cast_f32_to_bf16(const float* in, void* out, int64_t n, void* stream);
/* fp32 weight [rows,cols] -> bf16 copy [rows,cols] and bf16 transpose [cols,rows] (either may be null) */
int avf_prep_weight_bf16(const float* w, void* w_lo, void* w_t_lo, int rows, int cols, void* stream);

/* GEMM  C[M,N] = op(A)[M,K] * op(B)[K,N]  with fused epilogue.
 *   transA = 0: A stored [M,K] (lda)      transA = 1: A stored [K,M] (lda)
 *   transB = 0: B stored [K,N] (ldb)      transB = 1: B stored [N,K] (ldb)   (nn.Linear weight layout)
 * dtype AVF_F32: every form, any sizes.  dtype AVF_BF16: (transA=0,transB=1) "NT" with K%8==0, and
 * (transA=1,transB=0) "TN" (weight gradients, fp32 output, M%8==0, N%8==0).
 * c_dtype: storage type of C (and aux).  workspace (avf_gemm_workspace_bytes): the split-K slabs of a bf16 TN GEMM (required), of an
 * fp32 weight-gradient-shaped or skinny GEMM (optional: without it the unsplit general kernel runs). */
size_t avf_gemm_workspace_bytes(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K);
int avf_gemm(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
             const void* B, int64_t ldb, void* C, int64_t ldc, int c_dtype, int epilogue, const float* bias,
             const float* residual, int64_t ldres, void* aux, int64_t ldaux, void* workspace, void* stream);

/* Weight-stationary persistent NT GEMM (csrc/gemm_ws.hip): C[M,N] = epilogue(A[M,512] W[N,512]^T), the nn.Linear forward /
 * dX GEMMs of /root/reference/models/heads.py:191,195,212,215 at dim == 512.  W travels as its FRAGMENT-MAJOR image
 * (avf_pack_weight_ws of the row-major bf16 image, avf_pack_weight_ws_bytes(rows, cols) bytes; rows % 256 == 0, cols == 512):
 * each of the 8 wavefronts of a persistent workgroup keeps 32 weight rows in registers for the whole launch, only A streams.
 * Same epilogues, argument meaning and bit-for-bit the results of avf_gemm(AVF_BF16, 0, 1, ...); colsum (optional, with
 * workspace >= avf_gemm_nt_ws_workspace_bytes(M, N) - one partial row per persistent workgroup group, NOT the
 * avf_colsum_workspace_bytes of the standalone column sum): column sums of the stored C.  mx_q / mx_s (optional; DGELU with colsum and a
 * bf16 C, N % 32 == 0): also the MX-FP8 image of the fp32 values behind C (e4m3 [M][N], E8M0 [M][N/32]) - the fp8 mode's dGELU
 * GEMM keeps bf16 operands here and still feeds the fp8 GEMM behind it.  Errors if the shape does not qualify (M < 2048,
 * K != 512, N % 256 != 0). */
int avf_pack_weight_ws_ok(int64_t rows, int64_t cols);
size_t avf_pack_weight_ws_bytes(int64_t rows, int64_t cols);
size_t avf_gemm_nt_ws_workspace_bytes(int64_t M, int64_t N);
/* 1 when avf_gemm(AVF_BF16, 0, 1, ...) and the layer calls send this shape / epilogue to the persistent kernel (given 16-byte
 * aligned operands and no dropout); avf_gemm_nt_ws itself takes every shape the kernel can run */
int avf_gemm_nt_ws_dispatch(int64_t M, int64_t N, int64_t K, int epilogue, int c_dtype);
int avf_pack_weight_ws(const void* w_bf16, int64_t ldw, int64_t rows, int64_t cols, void* out, void* stream);

/* Test plumbing for the tiled bf16 NT GEMM: C[M,N] = epilogue(A[M,K] B[N,K]^T) as avf_gemm(AVF_BF16, 0, 1, ...) runs it, plus
 * the two things only a layer call could ask of that kernel family so far:
 *   colsum   (nullable) fp32 [N]: column sums over the rows of the values behind the stored C (fp32, before their rounding to
 *            c_dtype); needs workspace >= avf_gemm_nt_ws_workspace_bytes(M, N).
 *   dropout  (seed_lo, seed_hi, layer_index, site, p) name a dropout site exactly as avf_dropout_factors does, element index
 *            m * N + n; p == 0 is no dropout.  With f = those factors: BIAS_RES C = (acc + bias) * f + residual, BIAS_GELU
 *            aux = acc + bias (unmasked), C = gelu(aux) * f, DGELU C = acc * f * gelu'(aux).  Not on AVF_EPI_NONE.
 * residual and aux are stored in C's type.  Never the weight-stationary kernel, never an MX-FP8 image.
 * avf_gemm_nt_plan: which kernel that call runs, decided by the function the launcher itself acts on.  Pointers are replaced
 * by their presence (every operand 16-byte aligned).  *kind: 0 = the register-staged kernel (K % 64 != 0; *tile = -1), 1 = the
 * tiled LDS-DMA kernel; *tile: the tile configuration's id; *lean: the LEAN code of the instantiation (0 = general epilogue,
 * 1 = lean, 2 = lean with column sums, + 4 = with the dropout site); *wpf: 1 when the launch does the weight warm-up. */
int avf_gemm_nt_ex(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                   int c_dtype, int epilogue, const float* bias, const void* residual, int64_t ldres, void* aux, int64_t ldaux,
                   void* workspace, float* colsum, uint32_t seed_lo, uint32_t seed_hi, int layer_index, int site, float p,
                   void* stream);
int avf_gemm_nt_plan(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int c_dtype, int epilogue,
                     int has_bias, int64_t ldres, int64_t ldaux, int want_colsum, float p, int* kind, int* tile, int* lean,
                     int* wpf);
int avf_gemm_nt_ws(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B_packed, void* C, int64_t ldc,
                   int c_dtype, int epilogue, const float* bias, const void* residual, int64_t ldres, void* aux, int64_t ldaux,
                   void* workspace, float* colsum, void* mx_q, void* mx_s, void* stream);

/* The weight gradients of one layer (or of up to four layers) as ONE grouped launch (autograd of nn.Linear,
 * heads.py:191,195,212,215): up to sixteen
 * C_i[M_i,N_i] (fp32, dense) = A_i[K,M_i]^T * B_i[K,N_i] (bf16, token-major, dense: lda = M_i, ldb = N_i) that share the
 * reduction length K (the B*N token rows); K % 64 == 0, M_i % 8 == 0, N_i % 8 == 0.  Split-K partial slabs live in
 * `workspace` (avf_gemm_tn_group_workspace_bytes) and are folded by a second launch; a group whose tiles fill the chip
 * unsplit needs no workspace (0 bytes) and stores straight to C_i.
 * avf_gemm_tn_group_plan: what that launch decides, by the function the launcher itself acts on (host code only; the
 * tuning switches AVF_TN_BIG / AVF_TN_XCD / AVF_TN_SPLITS count exactly as in the launch).  out[0] = 1 for the
 * 256 x 128 tile, 0 for the 128 x 128 one; out[1] = wavefronts per workgroup (8 on the 256 x 128 tile, else 4); out[2] = output tiles of the group;
 * out[3] = S, the split count; out[4] = reduction rows per split (a multiple of 64; a split that starts past K writes a slab
 * of zeros); out[5] = the block order of the 256 x 128 kernel (> 0: XCD groups, -1: eighths of the split-major work list,
 * 0: tile-major; 0 on the 128 x 128 kernel); out[6] = workgroups launched; out[7] = the fold kernel's instantiation (2 .. 8 =
 * unrolled for that many slabs, 0 = its run-time loop, -1 = no fold: S == 1).  The workspace the launch needs is
 * S * sum(M_i N_i) * 4 bytes, never more than avf_gemm_tn_group_workspace_bytes.
 * avf_gemm_tn_plan: the same for avf_gemm(AVF_BF16, transA = 1, transB = 0): out[0] = S (up to 32), out[1] = rows per split. */
size_t avf_gemm_tn_group_workspace_bytes(int count, int64_t K, const int64_t* M, const int64_t* N);
int avf_gemm_tn_group(int count, int64_t K, const void* const* A, const void* const* B, float* const* C, const int64_t* M,
                      const int64_t* N, void* workspace, void* stream);
int avf_gemm_tn_group_plan(int count, int64_t K, const int64_t* M, const int64_t* N, int32_t* out);
int avf_gemm_tn_plan(int64_t M, int64_t N, int64_t K, int32_t* out);

/* Test plumbing for the fp32 (parity-mode) GEMM family of csrc/gemm_f32.hip: C[M,N] = epilogue(op(A) op(B)) as
 * avf_gemm(AVF_F32, transA, transB, ...) runs it - fp32 operands, C, residual and aux; workspace optional (without it the call
 * runs unsplit) - plus the dropout site only a layer call could ask of it so far: (seed_lo, seed_hi, layer_index, site, p) as
 * avf_gemm_nt_ex takes them, element index m * N + n, p == 0 is no dropout, not on AVF_EPI_NONE.
 * avf_gemm_f32_plan: what that call decides under the default arithmetic it would read (avf_set_f32_arith), by the function the launcher
 * itself acts on (host code only).  Pointers are replaced by their presence and alignment: bit i of `misaligned` set = that
 * operand is 4 bytes past a 16-byte boundary (bit 0 A, 1 B, 2 C, 3 bias, 4 residual, 5 aux, 6 workspace).
 * out[0] = the kernel: 0 = gemm_f32x3_kernel (bf16x3), 1 = gemm_f32_kernel on 32 x 32 tiles (T = 1), 2 = on 64 x 64 tiles
 * (T = 2); out[1] / out[2] = 1 when the reduction is the unit-stride axis of A / of B (AKF / BKF of the bf16x3 kernel);
 * out[3] = S, the split count (1: unsplit); out[4] = reduction rows per split (0 when unsplit); out[5] = 1 when the bf16x3
 * kernel's epilogue (or its slab store) uses 16-byte accesses. */
int avf_gemm_f32_ex(int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                    int64_t ldb, void* C, int64_t ldc, int epilogue, const float* bias, const float* residual, int64_t ldres,
                    void* aux, int64_t ldaux, void* workspace, uint32_t seed_lo, uint32_t seed_hi, int layer_index, int site,
                    float p, void* stream);
int avf_gemm_f32_plan(int transA, int transB, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                      int epilogue, int has_bias, int64_t ldres, int64_t ldaux, int has_workspace, int misaligned, int32_t* out);
/* The weight gradients of one parity-mode layer as ONE launch in the bf16x3 arithmetic: 2 .. 4 C_i[M_i,N_i] (fp32, dense) =
 * A_i[K,M_i]^T B_i[K,N_i] (fp32, token-major, rows lda[i] / ldb[i] apart; null: dense) sharing K >= 512, M_i >= 96, N_i >= 96,
 * N_i % 4 == 0, every pointer 16-byte aligned, split over K into slabs in `workspace` (..._workspace_bytes) and folded by a
 * second launch.  avf_gemm_f32_tn_group_plan: out[0] = 1 when the launch takes the group under the default arithmetic it would
 * read, which must be 1 (else the rest is 0 and avf_gemm_f32_tn_group refuses), out[1] = 128 x 128 tiles of the group, out[2] = S, out[3] =
 * reduction rows per split (a multiple of 32). */
size_t avf_gemm_f32_tn_group_workspace_bytes(int count, int64_t K, const int64_t* M, const int64_t* N);
int avf_gemm_f32_tn_group_plan(int count, int64_t K, const int64_t* M, const int64_t* N, int32_t* out);
int avf_gemm_f32_tn_group(int count, int64_t K, const void* const* A, const int64_t* lda, const void* const* B,
                          const int64_t* ldb, float* const* C, const int64_t* M, const int64_t* N, void* workspace, void* stream);

/* MX-FP8 operands (OCP microscaling: e4m3 elements, one E8M0 scale byte per 32 consecutive elements of a row) for the
 * forward nn.Linear GEMMs (heads.py:191,195,212) on v_mfma_scale_f32_16x16x128_f8f6f4 - BASELINE config 5.
 *   avf_quant_mx8:   x [rows,cols] (AVF_F32 | AVF_BF16, cols % 32 == 0) -> q [rows,cols] bytes, scales [rows,cols/32] bytes;
 *                    scale = floor(log2(block amax)) - 8 (+127), q = rne_e4m3(clamp(x * 2^-(scale-127), +-448)).
 *   avf_gemm_mx8_nt: C[M,N] = A[M,K] * B[N,K]^T from two such images (K % 128 == 0), fp32 accumulate, epilogues
 *                    AVF_EPI_NONE / BIAS_RES / BIAS_GELU / DGELU as avf_gemm; c_q / c_scales (optional, BIAS_GELU / DGELU, N % 32 == 0):
 *                    also the MX-FP8 image of the stored C, ready to be the next GEMM's A operand. */
/* e4m3 images of Wqkv, W1, W2, Wo (and, cfg.mx8_bwd, of the transposed W2, W1, Wo) of every layer of a stack from their
 * bf16 images, one launch (cfg.mx8_fwd = 1);
 * lowp[i] = the avf_layer_lowp_bytes buffer of layer i, after avf_layer_prepare_weights / the library Adam wrote it */
int avf_stack_quant_weights_mx8(const avf_layer_cfg* cfg, int layers, void* const* lowp, void* stream);
int avf_quant_mx8(int dtype, const void* x, int64_t rows, int64_t cols, void* q, void* scales, void* stream);
int avf_gemm_mx8_nt(int64_t M, int64_t N, int64_t K, const void* a_q, const void* a_scales, const void* b_q,
                    const void* b_scales, void* C, int64_t ldc, int c_dtype, int epilogue, const float* bias,
                    const float* residual, int64_t ldres, void* aux, int64_t ldaux, void* c_q, void* c_scales,
                    void* stream);
/* Test plumbing for the MX-FP8 NT GEMM: the same kernel family as avf_gemm_mx8_nt with what only a layer call could ask of it
 * so far.  lda / ldb: row strides of the e4m3 images in BYTES (multiples of 16; the scale images stay dense, [rows][K/32]);
 * residual and aux in C's type with their own leading dimensions; colsum (nullable) fp32 [N]: column sums over the rows of the
 * values behind the stored C (fp32, before their rounding to c_dtype), needs workspace >= avf_gemm_nt_ws_workspace_bytes(M, N);
 * (seed_lo, seed_hi, layer_index, site, p): a dropout site as avf_gemm_nt_ex takes it (element index m * N + n, p == 0 is no
 * dropout, not on AVF_EPI_NONE); c_q / c_scales as avf_gemm_mx8_nt.
 * avf_gemm_mx8_nt_plan: which instantiation that call runs, decided by the function the launcher itself acts on.  Pointers are
 * replaced by their presence (every operand 16-byte aligned).  *tile: the tile configuration's id; *lean: the LEAN code
 * (0 = general epilogue, 1 = lean, + 2 = with column sums, + 4 = with the MX-FP8 image of C). */
int avf_gemm_mx8_nt_ex(int64_t M, int64_t N, int64_t K, const void* a_q, int64_t lda, const void* a_scales, const void* b_q,
                       int64_t ldb, const void* b_scales, void* C, int64_t ldc, int c_dtype, int epilogue, const float* bias,
                       const void* residual, int64_t ldres, void* aux, int64_t ldaux, void* workspace, float* colsum,
                       uint32_t seed_lo, uint32_t seed_hi, int layer_index, int site, float p, void* c_q, void* c_scales,
                       void* stream);
int avf_gemm_mx8_nt_plan(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int c_dtype, int epilogue,
                         int has_bias, int64_t ldres, int64_t ldaux, int want_colsum, float p, int want_image, int* tile,
                         int* lean);
/* nn.LayerNorm forward (heads.py:178-185) writing the bf16 output AND its MX-FP8 image (dim % 32 == 0, dim <= 1536) */
int avf_layernorm_fwd_mx8(const float* x, const float* gamma, const float* beta, void* y_bf16, float* mean, float* rstd,
                          void* y_q, void* y_scales, int64_t rows, int dim, float eps, void* stream);

/* nn.LayerNorm backward (avf_layernorm_bwd with bf16 dy) writing the bf16 image dx_lo of dx = dres + dLN AND its MX-FP8
 * image (dim % 32 == 0, dim <= 1536): the A operand of the dX GEMM below the LayerNorm in the fp8 mode; dx (fp32) optional */
int avf_layernorm_bwd_mx8(const void* dy_bf16, const float* x, const float* gamma, const float* mean, const float* rstd,
                          const float* dres, float* dx, void* dx_lo, void* dx_q, void* dx_scales, float* dgamma, float* dbeta,
                          void* workspace, int64_t rows, int dim, void* stream);
/* avf_attn_fwd / avf_attn_bwd with the token mask of heads.py:225-232 (keep: device bytes [batch, tokens], 1 = kept; see
 * avf_layer_cfg.key_mask); fp32 arithmetic on fp32 or bf16 storage; workspace as avf_attn_bwd */
int avf_attn_fwd_masked(int dtype, const void* qkv, void* o, float* lse2, const void* keep, int batch, int tokens, int heads,
                        int dim_head, void* stream);
int avf_attn_bwd_masked(int dtype, const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv,
                        void* workspace, const void* keep, int batch, int tokens, int heads, int dim_head, void* stream);
/* bf16 attention forward (avf_attn_fwd) also writing the MX-FP8 image of o [B*N, I] - the A operand of to_out (heads.py:215)
 * in the fp8 mode.  Head-resident kernel only: dim_head 64, tokens <= 576 (error otherwise). */
int avf_attn_fwd_mx8(const void* qkv, void* o, float* lse2, void* o_q, void* o_scales, int batch, int tokens, int heads,
                     int dim_head, void* stream);
/* bf16 attention backward for PRE-SCALED queries (the q columns of qkv carry log2(e) / sqrt(dim_head), as the layer's Wqkv
 * image produces them) also writing the MX-FP8 image of dqkv [B*N, 3I] - the A operand of the dqkv -> dh1 GEMM (autograd of
 * heads.py:212) in the fp8 mode.  Merged kernel only: avf_attn_bwd_emits_mx8(tokens, dim_head) says (error otherwise). */
int avf_attn_bwd_emits_mx8(int tokens, int dim_head);
int avf_attn_bwd_mx8(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, void* dqkv_q,
                     void* dqkv_scales, int batch, int tokens, int heads, int dim_head, void* stream);

/* Multi-head self-attention core - heads.py:222-237.  qkv [B*N, 3I] (q|k|v, head-major columns),
 * o [B*N, I], lse2 fp32 [B,H,N] = log2-domain log-sum-exp of the scaled scores (saved for backward). */
int avf_attn_fwd(int dtype, const void* qkv, void* o, float* lse2, int batch, int tokens, int heads,
                 int dim_head, void* stream);
/* backward: dqkv [B*N,3I] from do [B*N,I].  workspace >= avf_attn_bwd_workspace_bytes (holds delta [B,H,N]). */
size_t avf_attn_bwd_workspace_bytes(int batch, int tokens, int heads, int dim_head);
int avf_attn_bwd(int dtype, const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv,
                 void* workspace, int batch, int tokens, int heads, int dim_head, void* stream);

/* The same attention core (bf16 only) on a projection whose q columns are ALREADY multiplied by log2(e)/sqrt(dim_head):
 * the scores leave the MFMA in the log2 domain and the subtraction of the running maximum / of lse2 rides in the MFMA's
 * C operand (no per-score multiply-add).  This is what avf_layer_fwd / avf_layer_bwd run - they fold the factor into the
 * query rows of the bf16 copy of to_qkv.weight (heads.py:212) - and dq, dk, dv are still the gradients with respect to
 * the UNSCALED q, k, v.  workspace >= avf_attn_bwd_workspace_bytes(...). */
int avf_attn_fwd_qs(const void* qkv, void* o, float* lse2, int batch, int tokens, int heads, int dim_head, void* stream);
int avf_attn_bwd_qs(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, void* workspace,
                    int batch, int tokens, int heads, int dim_head, void* stream);
/* Which kernels the bf16 attention core launches for a shape - host code only, decided by the functions the launchers
 * themselves switch on.  masked = 0: avf_attn_fwd / avf_attn_bwd on AVF_BF16 (q_prescaled = 0) and avf_attn_fwd_qs /
 * avf_attn_bwd_qs (q_prescaled = 1); masked = 1: avf_attn_fwd_masked_qs / avf_attn_bwd_masked_qs and the layer.
 *   *fwd: AVF_ATTN_RES8 | RES12 | RES_MULTI - the head-resident kernel with up to 8 / 12 waves in one pass, or 8 waves in
 *         several; AVF_ATTN_STREAM - the streaming kernel; AVF_ATTN_F32 - the fp32-arithmetic kernel (masked = 1 only).
 *   *bwd: AVF_ATTN_STREAM - delta + the two streaming kernels; AVF_ATTN_F32 - the fp32-arithmetic ones (masked = 1 only);
 *         or AVF_ATTN_MERGED + 2 * KB + ragged - the merged kernel with KB = 1 .. 4 key blocks per wave, ragged = 1 when
 *         the last key block holds rows past `tokens` (always under a mask).
 * The tuning switches of the library (AVF_TUNING=1) move the answers exactly as they move the launches. */
#define AVF_ATTN_RES8 0
#define AVF_ATTN_RES12 1
#define AVF_ATTN_RES_MULTI 2
#define AVF_ATTN_STREAM 3
#define AVF_ATTN_F32 4
#define AVF_ATTN_MERGED 8
int avf_attn_plan(int tokens, int dim_head, int q_prescaled, int masked, int* fwd, int* bwd);
/* Which kernel family the fp32-arithmetic attention (avf_attn_fwd / avf_attn_bwd on AVF_F32, and the masked / bf16-storage
 * calls that share its dispatch) takes under the default arithmetic those calls read (avf_get_f32_arith) - host code only, read-only,
 * answered by the predicates the dispatch itself switches on:
 *   AVF_ATTN_PARITY_VEC     the one-lane-per-query kernels (a mask, bf16 storage, pre-scaled q, another dim_head, or a tensor
 *                           that does not start on a 16-byte boundary)
 *   AVF_ATTN_PARITY_F32MFMA the f32-input MFMA kernels (dim_head 32 / 64 / 128)
 *   AVF_ATTN_PARITY_BF16X3  three bf16 products per fp32 product (dim_head 64, arithmetic 1)
 * aligned16 = 1: every tensor of the call (qkv, o, d_o, dqkv) starts on a 16-byte boundary.  aligned16 = 0: qkv itself does
 * not - both families refuse such a call, forward and backward.  A call whose qkv is aligned and another tensor is not lies
 * outside this query: the forward then looks at o, the backward at d_o and dqkv, and its bf16x3 kernels also at o (a
 * misaligned o alone sends that backward to the f32-input MFMA kernels). */
#define AVF_ATTN_PARITY_VEC 0
#define AVF_ATTN_PARITY_F32MFMA 1
#define AVF_ATTN_PARITY_BF16X3 2
int avf_attn_parity_plan(int dtype, int dim_head, int masked, int q_prescaled, int aligned16, int heads);
/* ... with the token mask of heads.py:225-232 (keep: device bytes [batch, tokens], 1 = kept - ANY pattern, token 0 and
 * whole clips included): the masked attention core exactly as avf_layer_fwd / avf_layer_bwd run it in a bf16, non-fp8
 * stack - one internal helper picks the kernels for the layer and for these calls.  avf_attn_masked_on_mfma(tokens,
 * dim_head) = 1: the masked head-resident MFMA forward and the masked merged backward (dim_head 64, tokens <= 512);
 * 0: the fp32-arithmetic kernels on bf16 storage with pre-scaled q.  lse2 of a dropped query: log2(tokens) on the MFMA
 * kernels, unspecified (finite) otherwise.  workspace >= avf_attn_bwd_workspace_bytes(...). */
int avf_attn_masked_on_mfma(int tokens, int dim_head);
int avf_attn_fwd_masked_qs(const void* qkv, void* o, float* lse2, const void* keep, int batch, int tokens, int heads,
                           int dim_head, void* stream);
int avf_attn_bwd_masked_qs(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, void* workspace,
                           const void* keep, int batch, int tokens, int heads, int dim_head, void* stream);

/* Token-sequence plumbing of the callers either side of the stack (fp32, dim % 4 == 0, 16-byte aligned pointers).
 *  avf_fuse_tokens:   out[b, t, :] = (t < t_video ? clip[b, t, :] : audio[b, t - t_video, :]) + pos[t, :]  (pos nullable)
 *                     - the sequence-axis fusion torch.cat([clip, audio], 1) + pos_embedding of BASELINE.json's configs
 *                     (feature-axis fusion of the reference: models/avformer.py:95-103).
 *  avf_token_mean_fwd: out[b, :] = mean_t y[b, t, :]                      (x.mean(dim=1), models/tformer.py head)
 *  avf_token_mean_bwd: dy[b, t, :] = g[b, :] / tokens (nullable when dy_bf16 is given), the same in bf16 (dy_bf16, nullable), and colsum[d] =
 *                     sum_b g[b, d] (nullable) = the column sums of dy that the top layer's bias gradient needs. */
int avf_fuse_tokens(const float* clip, const float* audio, const float* pos, float* out, int batch, int t_video,
                    int t_audio, int dim, void* stream);
int avf_token_mean_fwd(const float* y, float* out, int batch, int tokens, int dim, void* stream);
/* the two ends of a bf16 residual stream (cfg.resid_bf16; dim % 8 == 0): the fused token build writing bf16, the token mean
 * reading bf16 (fp32 accumulation, fp32 result) */
int avf_fuse_tokens_bf16(const float* clip, const float* audio, const float* pos, void* out_bf16, int batch, int t_video,
                         int t_audio, int dim, void* stream);
int avf_token_mean_fwd_bf16(const void* y_bf16, float* out, int batch, int tokens, int dim, void* stream);
int avf_token_mean_bwd(const float* g, float* dy, void* dy_bf16, float* colsum, int batch, int tokens, int dim,
                       void* stream);

/* ---- token producers / consumers either side of the stack; fp32, one launch each ------------------
 * avf_bn1d_fwd / _bwd: nn.BatchNorm1d of AU_former (heads.py:263,293) on x [batch, features].  training != 0: batch
 *   statistics (and, when non-null, running_mean / running_var <- (1-momentum) r + momentum stat, unbiased variance, and
 *   *num_batches_tracked += 1); training == 0: the running statistics.  y = (x - mean) * invstd * gamma + beta; mean /
 *   invstd [features] are kept for backward.  Backward: dx (nullable), dgamma, dbeta (nullable) from dy.
 * avf_token_dots_fwd / _bwd: the per-token bias-free Linear(emb, 1) heads (heads.py:325-337, tformer.py:389-401):
 *   out[b, t] = tokens[b, t, :] . w[t, :] (w rows ldw apart); out rows are ldo apart and columns tokens_per_clip .. pad_to-1
 *   are zeroed (the [B,21] layout of train.py:136-138).  Backward: dtokens (nullable), dw [tokens_per_clip, emb] rows lddw apart
 *   (nullable).
 * avf_assemble_tokens: out[b, t, :] = (t < n_lead ? lead[t, :] : x[b, t - n_lead, :]) + pos[t, :] (pos nullable) - TFormer's
 *   cls token + positional table (vformer.py:279-287; n_lead = 1), or a bare positional add (n_lead = 0).
 * avf_cat_features: out[b, t, :] = concat(a[b, t, :emb_a], v[b, t, :emb_v]) + pos[t, :] - avformer.py:100 + tformer.py:383-386.
 * avf_transpose_add: in [batch, rows, cols] -> out [batch, cols, rows] (+ pos [cols, rows], nullable): the feature-map <-> token
 *   permutes of ResFormer.forward (sformer.py:316-318, 326-327).
 * avf_zero_cols: out[r, c0..c1) = 0. */
int avf_bn1d_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                 int64_t* num_batches_tracked, float* y, float* mean, float* invstd, int batch, int features, float eps,
                 float momentum, int training, void* stream);
int avf_bn1d_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* invstd, float* dx,
                 float* dgamma, float* dbeta, int batch, int features, int training, void* stream);
int avf_token_dots_fwd(const float* tokens, const float* w, int64_t ldw, float* out, int64_t ldo, int pad_to, int batch,
                       int tokens_per_clip, int emb, void* stream);
int avf_token_dots_bwd(const float* dout, int64_t ldo, const float* tokens, const float* w, int64_t ldw, float* dtokens,
                       float* dw, int64_t lddw, int batch, int tokens_per_clip, int emb, void* stream);
int avf_assemble_tokens(const float* x, const float* lead, const float* pos, float* out, int batch, int patches, int n_lead,
                        int dim, void* stream);
int avf_cat_features(const float* a, const float* v, const float* pos, float* out, int batch, int tokens_per_clip, int emb_a,
                     int emb_v, void* stream);
int avf_transpose_add(const float* in, const float* pos, float* out, int batch, int rows, int cols, void* stream);
int avf_zero_cols(float* out, int64_t ld, int rows, int c0, int c1, void* stream);
/* counter[0] += 1; snapshot[0] = counter[0] (device int64 scalars, one launch, graph-capturable): the dropout seed of one forward
 * of a stack (nn.Dropout at heads.py:194,196,216 draws fresh masks per call; the kernels of a forward and of its backward read
 * the snapshot through cfg.seed_dev). */
int avf_seed_advance(int64_t* counter, int64_t* snapshot, void* stream);
/* a small nn.Linear on a few rows written into a zero-padded row - the AU logits of a pooled feature in the reference's [B,21]
 * layout (avformer.py:101-105): out[r, o] = x[r,:] . w[o,:] + bias[o] (o < out_features), 0 up to `width`; one launch.
 * Backward: dx = dout[:, :O] w, dw = dout[:, :O]^T x, db = column sums (any of them may be null); dout rows are ldd apart. */
int avf_linear_pad_fwd(const float* x, const float* w, const float* bias, float* out, int rows, int in_features, int out_features,
                       int width, void* stream);
int avf_linear_pad_bwd(const float* dout, int64_t ldd, const float* x, const float* w, float* dx, float* dw, float* db, int rows,
                       int in_features, int out_features, void* stream);

/* AULoss - loss.py:63-103.  logits/labels fp32 [rows, 12] (ld given); rows whose FIRST label == ignore
 * are dropped; loss[0] = mean over kept rows x 12 of BCE-with-logits(pos_weight); grad_unit [rows,12]
 * (contiguous) = d loss / d logits.  All rows dropped => NaN (as the reference). */
int avf_au_loss(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels, const float* pos_weight,
                float ignore, int rows, int ncls, float* loss, float* grad_unit, void* stream);
/* The same as a (sum, count) pair for batch-sharded data parallelism - loss.py:85-102 is a RATIO, so ranks with different
 * numbers of ignored rows must reduce numerator and denominator separately: sum_count[0] = sum over kept rows of the row's
 * mean BCE, sum_count[1] = kept rows, grad_unit = d sum_count[0] / d logits.  All rows dropped => (0, 0), zero gradient. */
int avf_au_loss_sum(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels,
                    const float* pos_weight, float ignore, int rows, int ncls, float* sum_count, float* grad_unit,
                    void* stream);
/* Either of the two (sum_mode 0 / 1) with the gradient laid out as the model's OUTPUT row: grad_wide [rows, width] contiguous,
 * columns 0..ncls-1 as grad_unit above, ncls..width-1 zero - the gradient of the reference's [B,21] row whose first 12 slots are
 * the AU logits (train.py:136-138, loss on out[:, :12]: avformer.py get_au_loss), in the same launch instead of the fill + copy
 * autograd's slice backward adds.  `loss`: one float (sum_mode 0) or the (sum, count) pair (sum_mode 1). */
int avf_au_loss_wide(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels, const float* pos_weight,
                     float ignore, int rows, int ncls, int width, int sum_mode, float* loss, float* grad_wide, void* stream);

/* ---- the task losses of the multi-task step (train.py:146,229; models/loss.py) ----------------
 * One single-workgroup launch computes the expression (EX), action-unit (AU) and valence / arousal (VA) losses on the model's
 * output rows out [rows, width] (row stride ld_out) and their gradient in that layout; nothing synchronises with the host.
 *   y_ex  int64 [rows]            class 0..6, or ex_ignore; null: no EX loss
 *   y_au  fp32 [rows, 12] (ld_au) rows whose FIRST label == au_ignore are dropped; null: no AU loss
 *   y_va  fp32 [rows, va_ncols] (ld_va) labels == va_ignore are dropped per column; null: no VA loss
 *   losses[3] = (ex, au, va); counts[3] = valid EX rows, AU labels != au_ignore, VA labels != va_ignore (as fp32);
 *   grad_wide [rows, width] contiguous: columns ex_col..+6 hold d losses[0] / d out, au_col..+11 d losses[1] / d out,
 *   va_col..+va_ncols-1 d losses[2] / d out; zero everywhere else and in the block of a task whose labels are null.
 * EX: cross-entropy with class weights ex_weight (nn.CrossEntropyLoss) or the focal loss of loss.py:398-466 (ex_weight = alpha;
 * 'mean' = sum / (rows x valid rows), ignored rows gather class 0 and are masked).  AU: AULoss (loss.py:63-103) or DiceAULoss
 * (loss.py:149-176: unweighted per-unit Dice + 5 x the pos-weighted BCE mean).  VA: va_weight[0] CCC(column 0) + va_weight[1]
 * CCC(column 1) with CCCLoss of loss.py:271-313 (unbiased variances, divided by `rows` as counted before the drop, 0 without a
 * gradient when at most one row is left), on tanh(out) when va_tanh is set.  Every row ignored: NaN for EX and AU as the
 * reference.  normalize: each loss (and its gradient) is divided by its count, and is 0 where the count is 0. */
#define AVF_TASK_LOSS_EX_CLASSES 7
#define AVF_TASK_LOSS_AU_UNITS 12
enum { AVF_EX_CROSS_ENTROPY = 0, AVF_EX_FOCAL = 1 };
enum { AVF_AU_BCE = 0, AVF_AU_DICE_BCE = 1 };
typedef struct avf_task_loss_cfg {
  int32_t ex_mode, au_mode;
  int32_t ex_col, au_col, va_col; /* first column of each block in the row: 12, 0, 19 in the reference's layout */
  int32_t va_ncols;               /* 2 (valence, arousal) or 1 */
  int32_t va_tanh;                /* 1: the CCC is taken on tanh(out), derivative included */
  int32_t normalize;
  int32_t ex_use_ignore;          /* 0: no ignore index (then focal 'mean' = sum / rows) */
  int32_t reserved;
  int64_t ex_ignore;
  float gamma, smooth;            /* focal */
  float ex_weight[AVF_TASK_LOSS_EX_CLASSES];
  float pos_weight[AVF_TASK_LOSS_AU_UNITS];
  float au_ignore, va_ignore;
  float va_weight[2];
  float reserved2;
} avf_task_loss_cfg;
size_t avf_sizeof_task_loss_cfg(void);
int avf_task_loss(const float* out, int64_t ld_out, const int64_t* y_ex, const float* y_au, int64_t ld_au, const float* y_va,
                  int64_t ld_va, const avf_task_loss_cfg* cfg, int rows, int width, float* losses, float* counts,
                  float* grad_wide, void* stream);
/* Backward of the above in one launch: dout [rows, width] = grad_wide scaled per column block by the incoming gradients of the
 * three losses (device scalars; null: that block is zero).  Columns outside the blocks are zero. */
int avf_task_loss_bwd(const float* grad_wide, const float* g_ex, const float* g_au, const float* g_va,
                      const avf_task_loss_cfg* cfg, int rows, int width, float* dout, void* stream);

/* ---- the evaluation metrics of the validation loop (train.py:106-169; metrics/accf1.py, metrics/cccmetric.py) ----
 * avf_eval_update: ONE single-workgroup launch per validation batch.  It reads the model's rows out [rows, >= 21] (fp32, row
 * stride ld_out) and the label arrays in the layout of the task losses above (any of them null: that task is skipped and its
 * slots are left as they were) and ADDS the batch's sufficient statistics into state, a device array of
 * AVF_EVAL_STATE_WORDS fp64 words which the caller zeroes once per evaluation.  Counts are held as fp64 so that the state is one
 * dtype - one buffer, one collective; they are exact up to 2^53 rows.  Layout:
 *   [AVF_EVAL_EX_CONF + 7 t + p]     EX confusion counts, t the label, p = argmax of the seven EX logits by torch's rule (first
 *                                    maximal index; a NaN logit counts as maximal).  A row whose label equals ex_ignore, or
 *                                    lies outside 0..6, is dropped.
 *   [AVF_EVAL_AU_STATS + 12 k + u]   k = 0..4: true positives, false positives, false negatives, correct, labelled of unit u,
 *                                    over the ENTRIES whose label differs from au_ignore.  The prediction is the reference's
 *                                    round(sigmoid(x)) in fp32: 1 for x > 2^-23 (where a correctly rounded fp32 sigmoid leaves
 *                                    0.5), 0 otherwise.  fp32 sigmoid implementations differ inside (0, 2^-22); outside that band
 *                                    they all agree with this rule.
 *   [AVF_EVAL_VA_MOMENTS + 6 j + k]  column j: n, sum x, sum y, sum x^2, sum y^2, sum x y over the rows whose label differs from
 *                                    va_ignore; x = tanhf(out) in fp32 (out itself when va_tanh is 0), products and sums in fp64.
 *   [AVF_EVAL_LOSS_SUM], [AVF_EVAL_LOSS_STEPS]  sum of *loss and the number of updates that carried one (loss: optional device
 *                                    fp32 scalar; null: both words are left alone).
 *   the remaining words are reserved and never written.
 * Optional per-row outputs, each may be null: pred_au uint8 [rows, 12], pred_ex int64 [rows], pred_va fp32 [rows, 2] (the tanh
 * values).  With state null the call only predicts.  Integer counts are folded through integer additions and the fp64 moments
 * in a fixed order (lane tree, then the waves in index order), so the same sequence of calls gives the same words every time.
 * Neither entry point allocates or synchronises; both can be captured.
 *
 * avf_eval_scores: ONE launch, state -> scores, AVF_EVAL_SCORE_WORDS fp64 words on the device, all arithmetic in fp64:
 *   0 ex_acc, 1 ex_f1, 2 ex_score, 3 au_acc, 4 au_f1, 5 au_score, 6 ccc_v, 7 ccc_a, 8 va_score, 9 avg_loss, 10 ex_kept_rows,
 *   11 au_labelled.
 * EX: accuracy over the kept rows; macro F1 over the classes that occur among the kept rows' labels or predictions (sklearn's
 * label set); score = 0.67 f1 + 0.33 acc; no kept row: NaN.  AU: accuracy over all labelled entries, mean over the 12 units of
 * the binary F1 (0 where 2 tp + fp + fn = 0); score = 0.5 f1 + 0.5 acc.  VA: per column 0 for n <= 1, else with the biased
 * moments 2 cov / (var_x + var_y + (m_x - m_y)^2 + 1e-8); score = their mean.  This is the METRIC's CCC (cccmetric.py:4-34), not
 * the loss's. */
#define AVF_EVAL_STATE_WORDS 128
#define AVF_EVAL_EX_CONF 0
#define AVF_EVAL_AU_STATS 49
#define AVF_EVAL_VA_MOMENTS 109
#define AVF_EVAL_LOSS_SUM 121
#define AVF_EVAL_LOSS_STEPS 122
#define AVF_EVAL_SCORE_WORDS 12
typedef struct avf_eval_cfg {
  int32_t ex_col, au_col, va_col; /* first column of each block in the row: 12, 0, 19 in the reference's layout */
  int32_t va_tanh;                /* 1: predictions and moments on tanh(out) (train.py:154) */
  int64_t ex_ignore;              /* 7 */
  float au_ignore, va_ignore;     /* -1, -5 */
} avf_eval_cfg;
size_t avf_sizeof_eval_cfg(void);
int avf_eval_update(const float* out, int64_t ld_out, const int64_t* y_ex, const float* y_au, int64_t ld_au, const float* y_va,
                    int64_t ld_va, const float* loss, const avf_eval_cfg* cfg, int rows, double* state, uint8_t* pred_au,
                    int64_t* pred_ex, float* pred_va, void* stream);
int avf_eval_scores(const double* state, const avf_eval_cfg* cfg, double* scores, void* stream);

/* ---- audio front-end: waveform -> normalised log-mel spectrogram (dataloader/aff2compdataset.py:47-68, 214-247:
 * torchaudio MelSpectrogram + left zero-padding of short clips; dataloader/clip_transforms.py:59-108: AmplitudeToDB('power',
 * top_db) per clip + Normalize) ---------------------------------------------------------------------------------------------
 * avf_mel_power: audio fp32 [rows, samples] -> mel fp32 [rows, n_mels, out_frames], out_frames = max(frames, full_frames) with
 * frames = 1 + samples / hop.  One memset of peak and ONE kernel launch: centred frames with reflect padding (samples > n_fft / 2),
 * `window` (win_length values, centred in the n_fft-point frame, zero outside), one-sided power spectrum by an fp32 FFT
 * (n_fft = 1024 only), then mel[m] = sum over bins k in [bin_lo[m], bin_hi[m]) of power[k] * fb[k, m] with fb fp32
 * [n_fft / 2 + 1, n_mels] row-major.  bin_lo / bin_hi are DEVICE int32 [n_mels] (the kernel clamps them to 0..n_fft/2+1); bins
 * outside them are taken as zero weights.  A clip with frames < full_frames is written at frame offset full_frames - frames
 * behind zero frames.  peak: device uint32 [rows / rows_per_clip], the bit pattern of the largest mel power of each group of
 * rows_per_clip consecutive rows (a clip and its channels).  The same input gives the same bits, call after call.
 *
 * avf_mel_db_norm: ONE launch, in place on mel [rows, n_mels, frames]:
 *   db = 10 log10(max(x, 1e-10));  db = max(db, 10 log10(max(peak[clip], 1e-10)) - top_db);  x = (db - mean) / std
 * evaluated in fp64 and rounded once to fp32.
 * Neither entry point allocates or synchronises; both can be captured.  Every argument is checked before anything is enqueued. */
int avf_mel_power(const float* audio, int64_t rows, int64_t samples, const float* window, int win_length, int n_fft, int hop,
                  const float* fb, const int32_t* bin_lo, const int32_t* bin_hi, int n_mels, int full_frames, int rows_per_clip,
                  float* mel, uint32_t* peak, void* stream);
int avf_mel_db_norm(float* mel, const uint32_t* peak, int64_t rows, int n_mels, int64_t frames, int rows_per_clip, double top_db,
                    double mean, double std, void* stream);

/* ---- audio windows from a resident waveform bank (dataloader/aff2compdataset.py:214-247; testset.py:164-198) --------------
 * wave: the wavs of a data set split, one after the other, `total` elements of fp32 (wave_dtype 0) or int16 (wave_dtype 1; a
 * sample x is worth x * 2^-15).  wav_start / wav_len int64 [V]: where wav v lies in wave; wav_of int32 [F]: the wav of every
 * sample; end_sample int64 [F]: int((time_stamp / 1000) * sample_rate) of every sample; index int64 [B].  All DEVICE arrays, read
 * by the kernels (no host synchronisation).  With N = sample_len_secs * sample_rate, w = int(window_size * sample_rate), shift =
 * audio_shift_secs * sample_rate, and for sample i = index[b] with E = end_sample[i], whose wav has L samples:
 *   num = min(N, max(E, w));  off = max(E - N + shift, 0);  got = max(0, min(num, L - off))
 *   got > n_fft / 2:   the window is wav[off : off + got]
 *   got <= n_fft / 2:  the window is silent.  So is an index outside [0, F), an absent wav (L == 0) and any table entry that
 *                      points outside its array; nothing outside [wave, wave + total) is read.
 *
 * avf_mel_power_bank: one memset of peak and ONE launch -> mel fp32 [B, n_mels, full_frames], peak uint32 [B].  Row b is what
 * avf_mel_power gives, bit for bit, on the window's own samples (w = win_length): 1 + got / hop frames, reflect padding at the
 * window's own ends, right-aligned behind zero columns; a silent row is all zero columns.  full_frames >= 1 + N / hop.  window,
 * win_length, n_fft, hop, fb, bin_lo, bin_hi, n_mels as avf_mel_power takes them; avf_mel_db_norm then runs on the result with
 * rows_per_clip = 1.
 * avf_wave_gather: ONE launch -> dst fp32 [B, N]: the window's samples right-aligned in N zeros, a silent row all zeros.  dst is
 * 4-byte aligned; 16-byte stores wherever the destination allows them.
 * Neither entry point allocates or synchronises; both can be captured.  dst / mel must not overlap the bank. */
int avf_mel_power_bank(const void* wave, int wave_dtype, int64_t total, const int64_t* wav_start, const int64_t* wav_len, int64_t V,
                       const int32_t* wav_of, const int64_t* end_sample, int64_t F, const int64_t* index, int64_t B, int64_t N,
                       int64_t shift, const float* window, int win_length, int n_fft, int hop, const float* fb,
                       const int32_t* bin_lo, const int32_t* bin_hi, int n_mels, int full_frames, float* mel, uint32_t* peak,
                       void* stream);
int avf_wave_gather(const void* wave, int wave_dtype, int64_t total, const int64_t* wav_start, const int64_t* wav_len, int64_t V,
                    const int32_t* wav_of, const int64_t* end_sample, int64_t F, const int64_t* index, int64_t B, int64_t N,
                    int64_t w, int64_t shift, float* dst, void* stream);

/* ---- video clip front-end: uint8 clips <-> normalised planes (dataloader/clip_transforms.py:31-45 NumpyToTensor, 59-93
 * Normalize, 111-128 RandomClipFlip; dataloader/aff2compdataset.py:69-77; models/sformer.py:365-373) ----------------------------
 * avf_clip_normalize: ONE launch.  src uint8 [B, T, H, W, C] (C in 1..4) -> dst, the last k of the C channels as planes:
 *   layout AVF_CLIP_CTHW: dst [B, k, T, H, W]       layout AVF_CLIP_TCHW: dst [B, T, k, H, W]
 *   dst[.. c .. h, w] = lut[(C - k + c) * 256 + src[b, t, h, w', C - k + c]],  w' = W - 1 - w where flip[b] != 0, else w
 * lut: DEVICE fp32 [C * 256] (the caller's table of (v / 255 - mean) / std); flip: DEVICE bytes [B] or null (no clip is mirrored),
 * read by the kernel at run time.  out_dtype AVF_F32 | AVF_BF16 (round to nearest even).  dst is aligned to its element size;
 * src needs no alignment.
 *
 * avf_clip_denormalize: ONE launch, the inverse direction.  src [B, C, T, H, W] or [B, T, C, H, W] (in_dtype AVF_F32 | AVF_BF16)
 * -> dst uint8 [B, T, H, W, C]:  trunc(min(max(((x * std[c]) + mean[c]) * 255, 0), 255)), each of the three operations rounded
 * to fp32 on its own (no fused multiply-add), NaN -> 0.  mean / std: DEVICE fp32 [C].  A flip is not undone.
 *
 * Sizes are 64-bit, as is every index in the kernels.  Neither entry point allocates or synchronises; both can be captured.
 * Every argument is checked before anything is enqueued. */
#define AVF_CLIP_CTHW 0
#define AVF_CLIP_TCHW 1
int avf_clip_normalize(const uint8_t* src, int64_t B, int64_t T, int64_t H, int64_t W, int C, int k, const float* lut,
                       const uint8_t* flip, void* dst, int out_dtype, int layout, void* stream);
int avf_clip_denormalize(const void* src, int in_dtype, int layout, int64_t B, int64_t T, int64_t H, int64_t W, int C,
                         const float* mean, const float* std, uint8_t* dst, void* stream);

/* ---- clip AutoAugment: the reference's ImageNetPolicy on uint8 clips (dataloader/autoaugment.py, dataloader/ops.py) -------------
 * avf_clip_autoaugment: ONE launch, one workgroup per frame.  src, dst uint8 [B, T, H, W, C], C = 3 or 4: channels 0..2 of every
 * frame go through the two slots of its plan, channel 3 is copied.  plan: DEVICE int32 [B * T * 2 * 8], per frame two slots
 * [op_code, p0 .. p6] applied in order (the encoding is documented in augment.py; the host resolves the random draws and every
 * double-precision constant into these words).  An op code outside 1..10 does nothing.  Each frame is read once and written once;
 * everything between happens in LDS: integer arithmetic, fp32 for the blend, fp64 for the autocontrast table and the bicubic of
 * shearX, no fused multiply-add - the bytes are those of Pillow.  dst == src is allowed (no other overlap); neither needs any
 * alignment.  A frame has at most avf_clip_autoaugment_max_pixels() pixels (C = 3; C = 4: three quarters of it) - both frame
 * buffers live in one workgroup's LDS.  Nothing is allocated or synchronised (capturable); every argument is checked before
 * anything is enqueued.
 *
 * avf_clip_autoaugment_normalize: ONE launch, the reference's whole training transform aug_clip_transform = [ImageNetPolicy(),
 * RandomClipFlip(), NumpyToTensor(), Normalize(...)] (dataloader/aff2compdataset.py:72-74, applied at 163-164): the result is
 * that of avf_clip_normalize on the clip of avf_clip_autoaugment, and no uint8 clip is written.  src, B .. C and plan as
 * avf_clip_autoaugment takes them (the same frame-size limit), k, lut, flip, dst, out_dtype and layout as avf_clip_normalize
 * takes them; dst must not overlap src.  Capturable; every argument is checked before anything is enqueued. */
int avf_clip_autoaugment(const uint8_t* src, uint8_t* dst, int64_t B, int64_t T, int64_t H, int64_t W, int C, const int32_t* plan,
                         void* stream);
int64_t avf_clip_autoaugment_max_pixels(void);
int avf_clip_autoaugment_normalize(const uint8_t* src, int64_t B, int64_t T, int64_t H, int64_t W, int C, const int32_t* plan,
                                   int k, const float* lut, const uint8_t* flip, void* dst, int out_dtype, int layout,
                                   void* stream);

/* ---- clips assembled on the device from a resident frame bank (dataloader/aff2compdataset.py:122-156; testset.py:84-113) --------
 * bank uint8 [F, H, W, C] (C in 1..4, no alignment assumed), video_db_nr int32 [F], present uint8 [F] or null (every frame is
 * present), index int64 [B]: all DEVICE pointers, read by the kernels at run time.  T: clip length, d >= 1: dilation.  Slot t of
 * sample b is frame a = index[b] - d * (T - 1 - t) of the bank - the last slot is index[b] itself - and it is BLACK (every byte 0)
 * where a < 0 or a >= F, where video_db_nr[a] != video_db_nr[index[b]], or where present[a] == 0 (the reference's failed decode).
 * An index[b] outside [0, F) gives an all-black clip and reads nothing of the bank (the reference would raise).  Black is a byte
 * value: normalised it is lut[c * 256 + 0], and a black frame goes through its AutoAugment slots like any other frame.
 *
 * avf_clip_gather:             ONE launch, bank -> dst uint8 [B, T, H, W, C], no alignment assumed (16-byte loads and stores where
 *                              the source and destination ranges sit alike in their 16-byte chunks, staged through LDS where not).
 * avf_clip_gather_normalize:   ONE launch, bank -> planes; k, lut, flip, dst, out_dtype and layout as avf_clip_normalize takes them,
 *                              and the result is that of avf_clip_normalize on the clip of avf_clip_gather.  No uint8 clip is written.
 * avf_clip_gather_autoaugment: ONE launch, bank -> augmented dst uint8 [B, T, H, W, C]; C, plan and the frame-size limit
 *                              (avf_clip_autoaugment_max_pixels) as avf_clip_autoaugment takes them, and the result is that of
 *                              avf_clip_autoaugment on the clip of avf_clip_gather.
 * avf_clip_gather_autoaugment_normalize:
 *                              ONE launch, bank -> augmented, mirrored, normalised planes: the reference's training transform
 *                              (dataloader/aff2compdataset.py:72-74, 163-164) from the bank.  plan as avf_clip_gather_autoaugment,
 *                              k .. layout as avf_clip_gather_normalize take them, and the result is that of avf_clip_normalize on
 *                              the clip of avf_clip_gather_autoaugment: a black slot goes through its plan slots and is then
 *                              normalised.  No uint8 clip is written.
 * dst must not overlap the bank.  Sizes and indices are 64-bit.  Nothing is allocated or synchronised (capturable); every argument
 * is checked before anything is enqueued. */
int avf_clip_gather(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present, const int64_t* index, int64_t F,
                    int64_t B, int64_t T, int64_t d, int64_t H, int64_t W, int C, uint8_t* dst, void* stream);
int avf_clip_gather_normalize(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present, const int64_t* index,
                              int64_t F, int64_t B, int64_t T, int64_t d, int64_t H, int64_t W, int C, int k, const float* lut,
                              const uint8_t* flip, void* dst, int out_dtype, int layout, void* stream);
int avf_clip_gather_autoaugment(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present, const int64_t* index,
                                int64_t F, int64_t B, int64_t T, int64_t d, int64_t H, int64_t W, int C, const int32_t* plan,
                                uint8_t* dst, void* stream);
int avf_clip_gather_autoaugment_normalize(const uint8_t* bank, const int32_t* video_db_nr, const uint8_t* present,
                                          const int64_t* index, int64_t F, int64_t B, int64_t T, int64_t d, int64_t H, int64_t W,
                                          int C, const int32_t* plan, int k, const float* lut, const uint8_t* flip, void* dst,
                                          int out_dtype, int layout, void* stream);

/* ---- TFormer's tokens from a resident bank of per-frame S-Former features (vformer.py:232-293) ----------------------------------
 * The frozen S-Former runs per frame, in eval mode: a frame's features do not depend on the clip it sits in.  feat fp32 [F, D]
 * (rows ldf floats apart) holds them once per frame, black [D] is the feature row of a black frame, and video_db_nr, present
 * (nullable) and index are exactly what avf_clip_gather takes: all DEVICE pointers, read by the kernel at run time.  The rule is
 * the one above, applied to feature rows: slot t of sample b is frame a = index[b] - d * (T - 1 - t), and its row is black where
 * a < 0 or a >= F, where video_db_nr[a] != video_db_nr[index[b]], where present[a] == 0, or where index[b] is outside [0, F) -
 * then the whole sample is black and nothing of feat, video_db_nr or present is read for it; in every other case it is feat[a].
 *   out[b, j, :]          = lead[j, :] + pos[j, :]                 j < n_lead   (lead [n_lead, D]; null iff n_lead == 0)
 *   out[b, n_lead + t, :] = row(b, t)  + pos[n_lead + t, :]        t < T        (pos [n_lead + T, D] or null: no add)
 * out fp32 [B, n_lead + T, D], contiguous, must not overlap feat.  At most one fp32 add per element: bit for bit what
 * avf_assemble_tokens gives on the rows gathered first.  D % 4 == 0 and ldf % 4 == 0, ldf >= D; feat, black, lead, pos and out
 * 16-byte aligned.  ONE launch; sizes and indices are 64-bit; nothing is allocated or synchronised (capturable); every argument
 * is checked before anything is enqueued, and an error names the argument. */
int avf_feature_clip_tokens(const float* feat, int64_t ldf, const float* black, const int32_t* video_db_nr, const uint8_t* present,
                            const int64_t* index, int64_t F, int64_t B, int64_t T, int64_t d, int D, const float* lead, int n_lead,
                            const float* pos, float* out, void* stream);

/* ---- one transformer layer (heads.py:246-255), forward and backward ------------------------ */
size_t avf_layer_saved_bytes(const avf_layer_cfg* cfg);     /* activations kept for backward        */
size_t avf_layer_lowp_bytes(const avf_layer_cfg* cfg);      /* bf16 weight copies (+transposes)     */
size_t avf_layer_workspace_bytes(const avf_layer_cfg* cfg); /* scratch, reusable across layers      */
size_t avf_layer_grad_stream_bytes(const avf_layer_cfg* cfg); /* bytes of one dx_out_lo / dx_in_lo buffer of avf_layer_bwd:
                                                                 R*D bf16, plus the MX-FP8 image behind it when cfg.mx8_bwd */
/* refresh the bf16 weight copies from the fp32 masters (no-op in AVF_F32 mode) */
int avf_layer_prepare_weights(const avf_layer_cfg* cfg, const avf_layer_params* p, void* lowp, void* stream);

/* Adam step of one layer fused with the refresh of its bf16 weight copies - torch.optim.Adam(lr, betas, eps,
 * weight_decay) as the reference's training loop uses it (train.py:318-322; L2 decay added to the gradient, bias
 * correction by `step`, amsgrad off), arithmetic as torch's fused kernel.  p is updated IN PLACE (the const of
 * avf_layer_params is cast away), exp_avg / exp_avg_sq likewise; a tensor whose gradient pointer is null is not
 * updated (its bf16 copies are still rewritten).  `step` is a device float holding the number of THIS update (>= 1),
 * read at run time (graph-capturable); null means 1.  lowp as for avf_layer_fwd (ignored in AVF_F32 mode). */
int avf_layer_adam_step(const avf_layer_cfg* cfg, const avf_layer_params* p, const avf_layer_grads* g,
                        const avf_layer_grads* exp_avg, const avf_layer_grads* exp_avg_sq, void* lowp, float lr,
                        float beta1, float beta2, float eps, float weight_decay, const float* step, void* stream);

/* the same for `layers` consecutive layers of one stack (arrays of `layers` structs, lowp[l] per layer): thirteen layers per
 * launch (the descriptor table is a 12.6 KB kernel argument) */
int avf_stack_adam_step(const avf_layer_cfg* cfg, int layers, const avf_layer_params* p, const avf_layer_grads* g,
                        const avf_layer_grads* exp_avg, const avf_layer_grads* exp_avg_sq, void* const* lowp, float lr,
                        float beta1, float beta2, float eps, float weight_decay, const float* step, void* stream);

/* the same Adam update for `count` arbitrary fp32 tensors (host arrays of device pointers and element counts): the
 * parameters around the stacks (positional embedding, AU head).  A tensor whose gradient pointer is null is skipped. */
int avf_adam_step_tensors(int count, float* const* p, const float* const* g, float* const* exp_avg,
                          float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                          float weight_decay, const float* step, void* stream);

/* One optimizer step's launches, collected (torch.optim.Adam.step() over all parameters, train.py:237): between _begin and _end
 * on the calling thread, avf_layer_adam_step / avf_stack_adam_step / avf_adam_step_tensors append to one descriptor table
 * instead of launching; the table is launched when it is full (143 tensors), when the hyper-parameters, the step pointer or the
 * stream of a call differ from the pending ones, and by _end.  The reference's real model has five small stacks and a dozen
 * loose tensors: one launch instead of six.  Every pointer handed over must stay valid until _end returns.
 * The session is THREAD-LOCAL: _begin, every step call and _end / _abort must come from the same thread, with the same device
 * current (the table is launched on the stream of the calls it collected).  _abort closes the session without launching the
 * pending table (the caller failed while collecting the step); tables that were already launched stay launched.
 * The table is a ~12.6 KB by-value kernel argument: avf_selftest_adam_table() launches a full one (143 descriptors, one element
 * each) and checks every element - run it once per process where kernel arguments above 4 KB are in doubt. */
int avf_adam_batch_begin(void);
int avf_adam_batch_end(void);
int avf_adam_batch_abort(void);
int avf_selftest_adam_table(void* stream);

/* Gradient clipping and the learning-rate schedule of a step, decided on the device (opts.py --grad_clip / --n_warmup_steps,
 * the epoch decays of train()).  ctl is a device block of four floats:
 *   ctl[0] (out) learning-rate multiplier of this update = ctl[3] * min(1, step / n_warmup_steps)  (1 * ctl[3] without warm-up:
 *                LambdaLR(lambda s: min(1, (s + 1) / n)), `step` being the device counter the Adam calls take, from 1)
 *   ctl[1] (out) gradient multiplier min(1, max_norm / (norm + 1e-6)) - torch.nn.utils.clip_grad_norm_'s, in fp32; NaN for a NaN
 *                norm, 0 for an infinite one, 1 when clipping is off
 *   ctl[2] (out) the total L2 norm of the `count` gradients before clipping (0 when clipping is off)
 *   ctl[3] (in)  the caller's learning-rate scale
 * The norm is summed in fp64 in a fixed order (no atomics): the same gradients give the same bits.  g / numel are host arrays;
 * a null gradient pointer or a numel <= 0 is skipped; gradients are fp32, 4-byte aligned, of any length.  max_norm <= 0: no
 * clipping - nothing is read, count may be 0 and ws null.  Otherwise ws holds avf_grad_control_workspace_bytes(count, numel)
 * bytes (8 per 4096 elements of each tensor, skipped tensors included).  Nothing is allocated or synchronised (capturable).
 * The gradients are NOT modified: the multiplier is applied by the Adam kernel (avf_adam_batch_control). */
size_t avf_grad_control_workspace_bytes(int count, const int64_t* numel);
int avf_grad_control(int count, const float* const* g, const int64_t* numel, float max_norm, int n_warmup_steps,
                     const float* step, float* ctl, void* ws, void* stream);

/* Attach a control block to the open Adam session (between avf_adam_batch_begin and _end, same thread): every table collected
 * afterwards runs with lr * ctl[0] and with ctl[1] * g in place of each gradient g (before the weight decay is added), both read
 * at run time.  A change of pointer launches the pending table first, like a change of hyper-parameters; null detaches.  The
 * session ends with the pointer reset to null; without this call the Adam kernel's arithmetic is what it always was. */
int avf_adam_batch_control(const float* ctl);

/* x_out = layer(x_in); x_in, x_out [B*N, D] (may not alias): fp32, or bf16 when cfg.resid_bf16 is set. */
int avf_layer_fwd(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                  void* x_out, void* saved, void* workspace, void* stream);

/* ---- the two ends of a fused stack (the stack's input is cat([clip, audio], 1) + pos) on the all-bf16 streams --------------
 * Both apply to a layer with dtype AVF_BF16, resid_bf16 and grad_stream_bf16 set, dropout_p == 0, no mx8 and no key mask
 * (dim % 8 == 0 follows from resid_bf16); the _ok functions answer 1 where the entry next to them can run, and a caller takes
 * avf_fuse_tokens_bf16 + avf_layer_fwd, or avf_layer_bwd[_dx] + a column sum of dx_in, where they answer 0.
 *   avf_layer_fwd_embed: avf_layer_fwd for the bottom layer without the separate embedding pass.  LayerNorm-1 builds each row as
 *     bf16(clip[b, t] or audio[b, t - t_video], + pos[t]) - avf_fuse_tokens_bf16's values and rounding - and also stores it as
 *     x0 [B*N, D] bf16, the tensor to pass as x_in to the backward of this layer.  clip [B, t_video, D], audio [B, N - t_video,
 *     D], pos [N, D]: fp32, 16-byte aligned, 0 < t_video < N.  x0, x_out and everything saved are bit-identical to the two calls.
 *   avf_layer_bwd_pos / avf_layer_bwd_dx_pos: avf_layer_bwd / avf_layer_bwd_dx for the bottom layer when below it only
 *     d pos_embedding is wanted: d_pos[t, :] = sum_b dx_in[b * N + t, :], fp32 [N, D], written by a token-major LayerNorm-1
 *     backward.  No dx_in, dx_in_lo or dx_in_colsum is produced.  batch must be within the token-major rule (layernorm.hip,
 *     LNR8_TOK_MAX_BATCH).  d_pos and this layer's LayerNorm-1 gradients are summed in another order than by the plain entries
 *     (fp32 rounding level), deterministically; every other gradient is bit-identical. */
int avf_layer_fwd_embed_ok(const avf_layer_cfg* cfg);
/* Which kernels a layer of this configuration runs (pure host code, computed by the expressions the dispatch itself uses): a bit
 * set - bit 0: avf_layer_fwd is the single-launch short-sequence forward; bit 1: avf_layer_bwd runs the two fused short-sequence
 * kernels; bit 2: the second of them also runs the attention backward.  0: the per-operator path (or an invalid cfg).  The
 * short-sequence kernels take dtype AVF_BF16, dim_head 32, 1..16 tokens, dim / heads * dim_head / mlp_dim in {128, 256}, the fp32
 * residual stream, no mx8 and no key mask. */
int avf_layer_small_path(const avf_layer_cfg* cfg);
/* ... and the two LayerNorm launches behind them as operators.  avf_layernorm_fwd_embed: x0 = bf16(cat([clip, audio], 1) + pos)
 * [B*(t_video+t_audio), D] and y (bf16), mean, rstd = LayerNorm(x0); dim % 8 == 0, dim <= 1536, t_video > 0, t_audio > 0.
 * avf_layernorm_bwd_pos: the all-bf16 LayerNorm backward (dy, x, dres [batch*tokens, D] bf16; dres nullable) reduced over the
 * clips: d_pos [tokens, D] fp32, dgamma, dbeta; workspace of avf_layernorm_bwd_pos_workspace_bytes; _ok: the batch is within
 * the token-major rule. */
int avf_layernorm_fwd_embed(const float* clip, const float* audio, const float* pos, int batch, int t_video, int t_audio,
                            void* x0_bf16, const float* gamma, const float* beta, void* y_bf16, float* mean, float* rstd, int dim,
                            float eps, void* stream);
int avf_layernorm_bwd_pos_ok(int batch, int tokens, int dim);
size_t avf_layernorm_bwd_pos_workspace_bytes(int batch, int tokens, int dim);
int avf_layernorm_bwd_pos(const void* dy_bf16, const void* x_bf16, const float* gamma, const float* mean, const float* rstd,
                          const void* dres_bf16, float* d_pos, float* dgamma, float* dbeta, void* workspace, int batch, int tokens,
                          int dim, void* stream);
int avf_layer_fwd_embed(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const float* clip,
                        const float* audio, const float* pos, int t_video, void* x0, void* x_out, void* saved, void* workspace,
                        void* stream);
int avf_layer_bwd_pos_ok(const avf_layer_cfg* cfg);
int avf_layer_bwd_pos(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                      const void* saved, const float* dx_out, const void* dx_out_lo, const float* dx_out_colsum, float* d_pos,
                      const avf_layer_grads* g, void* workspace, void* stream);
int avf_layer_bwd_dx_pos(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                         const void* saved, const float* dx_out, const void* dx_out_lo, const float* dx_out_colsum, float* d_pos,
                         const avf_layer_grads* g, void* workspace, void* dw_block, void* dw_desc, void* stream);

/* dx_in (fp32) and all parameter gradients from dx_out (fp32).  dx_out_lo: optional bf16 copy of dx_out
 * (null => made internally); dx_in_lo: optional bf16 copy of dx_in to hand to the previous layer (with dropout
 * active it already carries layer_index-1's site-2 mask, which is what that layer's MLP gradients consume).
 * dx_out_colsum: optional [D] column sums of dx_out (= this layer's b2 gradient) already computed by the
 * caller's previous call; dx_in_colsum: optional [D] output, column sums of dx_in for the next call.
 * dx_in may alias dx_out (dx_out_lo / dx_in_lo must then be distinct buffers).  x_in: the tensor avf_layer_fwd was given
 * (bf16 when cfg.resid_bf16); the gradients dx_* are fp32 / bf16 images independently of it. */
int avf_layer_bwd(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                  const void* saved, const float* dx_out, const void* dx_out_lo, const float* dx_out_colsum,
                  float* dx_in, void* dx_in_lo, float* dx_in_colsum, const avf_layer_grads* g, void* workspace,
                  void* stream);

/* ---- deferred weight gradients: several layers' dW in one launch (bf16 path) ---------------------------------------------
 * One layer's four weight gradients are 64 tiles of 256 x 128 at dim 512 - a quarter of the chip - so avf_layer_bwd splits their
 * token reduction four ways and folds the partial slabs in a second launch.  A caller that runs a whole stack can instead let
 * the gradients of several layers wait and launch them together: four such layers are exactly one workgroup per CU, with no
 * split, no slabs and no slab fold.
 *   avf_layer_dw_defer_ok(cfg, &tiles, &slots): 1 if the layer's mode allows it (AVF_BF16 on the grouped launch: rows % 64 == 0;
 *     no dropout, no mx8, no key mask, not the short-sequence layer), with the layer's tile count and the workgroup slots of one
 *     round of the kernel its group runs on.  A caller groups at most slots / tiles layers (and at most avf_layers_dw_max()).
 *   avf_layer_bwd_dx: avf_layer_bwd without the weight-gradient launch and the layer's column folds.  dx_in and everything the
 *     layer below needs are written as usual; of the parameter gradients only b2 (when handed over as dx_out_colsum) is final.
 *     The operands the deferred launch reads stay in dw_block (DEVICE, avf_layer_dw_block_bytes(cfg) bytes, 256-byte aligned,
 *     one per deferred layer) and are described in dw_desc (HOST, avf_layer_dw_desc_bytes() bytes).  Until avf_layers_dw has
 *     run, the caller keeps alive and unchanged: dw_block, the layer's `saved` buffer, and dx_out_lo (the bf16 gradient image
 *     the layer read - a caller that ping-pongs two stream buffers gives each deferred layer its own).
 *   avf_layers_dw: the weight gradients and column folds of n_layers (1 .. avf_layers_dw_max()) deferred layers, the order of
 *     cfgs / descs being the order of the launch's tile list (top layer first).  One grouped launch, then one fold launch: the
 *     column folds alone when the group fills a round unsplit, else the slab fold with the column folds riding along
 *     (workspace / workspace_bytes: at least avf_layers_dw_workspace_bytes, which is 0 for a group that ends up unsplit; a
 *     workspace that is too small is an error, nothing is launched).
 * Sums are combined in a fixed order (no atomics): the same inputs give the same bits.  An unsplit group accumulates each
 * element in one fp32 chain where avf_layer_bwd adds four partial chains: the gradients differ at rounding level. */
int avf_layer_dw_defer_ok(const avf_layer_cfg* cfg, int* tiles_per_layer, int* slots);
int avf_layers_dw_max(void);
size_t avf_layer_dw_block_bytes(const avf_layer_cfg* cfg);
size_t avf_layer_dw_desc_bytes(void);
int avf_layer_bwd_dx(const avf_layer_cfg* cfg, const avf_layer_params* p, const void* lowp, const void* x_in,
                     const void* saved, const float* dx_out, const void* dx_out_lo, const float* dx_out_colsum,
                     float* dx_in, void* dx_in_lo, float* dx_in_colsum, const avf_layer_grads* g, void* workspace,
                     void* dw_block, void* dw_desc, void* stream);
size_t avf_layers_dw_workspace_bytes(const avf_layer_cfg* cfgs, int n_layers);
int avf_layers_dw(const avf_layer_cfg* cfgs, int n_layers, const void* const* descs, void* workspace, size_t workspace_bytes,
                  void* stream);

/* ---- frozen ResNet BasicBlock stages, forward only (csrc/conv.hip) ----------------------------------------------------------
 * The conv stages around the S-Former's token section: conv3x3 / conv1x1 (vformer.py:117-125), BasicBlock.forward
 * (vformer.py:149-165: conv1 - bn1 - relu - conv2 - bn2 - += identity - relu, identity = downsample(x) = conv1x1 + BatchNorm2d,
 * vformer.py:218-221), layer1..layer4 and avgpool + flatten of ResFormer.forward (vformer.py:242-244, 261-265).  Activations are
 * NHWC, so the stage-3 map [B', 7, 7, 256] IS the token tensor [B', 49, 256] of vformer.py:247-259 and no permute is run.
 * BatchNorm2d is folded in eval mode (running statistics): "frozen" means eval-mode here.  No gradients.
 *   avf_conv_pack_weight: w [Cout, Cin, k, k] fp32 (nn.Conv2d, bias=False) -> w_packed [Cout, k, k, Cin] bf16 (RNE);
 *     scale[c] = gamma[c] / sqrt(running_var[c] + eps), shift[c] = beta[c] - running_mean[c] * scale[c], computed in fp64 and
 *     stored as fp32 [Cout].  The scale stays in the epilogue: it is not multiplied into the bf16 weights.  Once per weight load.
 *   avf_conv2d_nhwc: out[n, oy, ox, co] = act( (sum_{ky,kx,ci} x[n, oy*stride - pad + ky, ox*stride - pad + kx, ci] *
 *     w_packed[co, ky, kx, ci]) * scale[co] + shift[co] (+ residual[n, oy, ox, co]) ), act = ReLU when relu != 0; positions
 *     outside the image count as zero and are never read.  k = 3 (pad 1) or 1 (pad 0), stride 1 or 2, Ho = (H + 2 pad - k) /
 *     stride + 1; Cin % 32 == 0, Cout % 16 == 0.  x [N, H, W, Cin] fp32 (rounded to bf16, RNE, as it is staged) or bf16;
 *     residual (null: none) and out [N, Ho, Wo, Cout] fp32 or bf16 (RNE), each with its own type.  bf16 products accumulate in
 *     fp32 (v_mfma_f32_16x16x32_bf16); the epilogue is fp32.  Every operand 16-byte aligned; out may not overlap an input.
 *   avf_conv_plan: the tile avf_conv2d_nhwc runs a shape on: *tile = its id (0: 128 pixels x 64 channels, 1: 64 x 32), *tile_m /
 *     *tile_n its extent.  Same argument checks as the launch.
 *   avf_avgpool_nhwc: x [N, HW, C] fp32 or bf16 -> out [N, C] fp32, the mean over HW accumulated in fp32 (C % 4 == 0). */
int avf_conv_pack_weight(const float* w, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, double eps, void* w_packed, float* scale, float* shift, int Cout, int Cin,
                         int k, void* stream);
int avf_conv2d_nhwc(const void* x, int x_dtype, const void* w_packed, const float* scale, const float* shift,
                    const void* residual, int res_dtype, int relu, int k, int stride, void* out, int out_dtype, int N, int H,
                    int W, int Cin, int Cout, void* stream);
int avf_conv_plan(int N, int H, int W, int Cin, int Cout, int k, int stride, int* tile, int* tile_m, int* tile_n);
int avf_avgpool_nhwc(const void* x, int x_dtype, float* out, int64_t N, int HW, int C, void* stream);

/* ---- the same stages in the parity arithmetic (csrc/conv_f32.hip) ------------------------------------------------------------
 * fp32 NHWC in, fp32 NHWC out, every fp32 product computed as three bf16 MFMA products ("bf16x3", as avf_gemm's fp32 mode):
 * v -> hi = bf16(v) (RNE), lo = bf16(v - hi) (the difference is exact in fp32);  x w ~ hi_w lo_x + lo_w hi_x + hi_w hi_x, each
 * product exact in fp32, accumulated in fp32 in that order (v_mfma_f32_16x16x32_bf16); lo_w lo_x is not computed.  At most
 * 3 * 2^-16 relative error per product.  This is the convolution's one parity arithmetic: avf_set_f32_arith does not
 * reach it.
 *   avf_conv_pack_weight_f32x3: w [Cout, Cin, k, k] fp32 -> w_hi, w_lo [Cout, k, k, Cin] bf16, the split above; scale / shift
 *     as avf_conv_pack_weight folds them (fp64, stored as fp32 [Cout]).  Once per weight load.
 *   avf_conv2d_nhwc_f32x3: avf_conv2d_nhwc's operation, shape rules (k = 3 or 1, stride 1 or 2, Cin % 32 == 0, Cout % 16 == 0),
 *     alignment and overlap rules and tile dispatch (avf_conv_plan names the tile for both); x [N, H, W, Cin], residual (null:
 *     none) and out [N, Ho, Wo, Cout] all fp32.  x is split as it is staged; the epilogue is fp32. */
int avf_conv_pack_weight_f32x3(const float* w, const float* gamma, const float* beta, const float* running_mean,
                               const float* running_var, double eps, void* w_hi, void* w_lo, float* scale, float* shift, int Cout,
                               int Cin, int k, void* stream);
int avf_conv2d_nhwc_f32x3(const float* x, const void* w_hi, const void* w_lo, const float* scale, const float* shift,
                          const float* residual, int relu, int k, int stride, float* out, int N, int H, int W, int Cin, int Cout,
                          void* stream);

/* ---- data gradient of the frozen stages (csrc/conv_dgrad.hip, csrc/conv_dgrad_f32.hip) ---------------------------------------
 * What trains pos_embedding and spatial_transformer behind the frozen layer4 (vformer.py:244-265): the gradient with respect to
 * the INPUT of avf_conv2d_nhwc, with the identity add and the ReLU gate of BasicBlock's backward in its epilogue, and the
 * backward of avf_avgpool_nhwc.  The weights are frozen: no weight gradient, no BatchNorm gradient.
 *   wt [Cin, k, k, Cout] bf16: the image of fp32(w[co, ci, ky, kx] * scale[co]), one RNE rounding - the folded BatchNorm scale
 *     is part of it, the shift has no gradient.  It is avf_conv_pack_weight's image of the transposed, pre-scaled weight
 *     [Cin, Cout, k, k] (avf_conv_pack_weight_f32x3's hi / lo pair for the parity form); there is no pack entry of its own.
 *   avf_conv2d_nhwc_dgrad: with pad = 1 for k = 3 and 0 for k = 1, Ho / Wo by avf_conv2d_nhwc's rule,
 *       acc[n, iy, ix, ci] = sum over (ky, kx) with ty = iy + pad - ky, tx = ix + pad - kx, ty % stride == 0, tx % stride == 0,
 *                            oy = ty / stride in [0, Ho), ox = tx / stride in [0, Wo), and co of
 *                            gy[n, oy, ox, co] * wt[ci, ky, kx, co]
 *       v   = acc + addend[n, iy, ix, ci]               (addend null: none)
 *       out = gate[n, iy, ix, ci] > 0 ? v : 0           (gate null: v; a NaN gate gives 0)
 *     A tap off the stride lattice or out of range counts as zero and is never read.  gy [N, Ho, Wo, Cout] fp32 (rounded to
 *     bf16, RNE, as it is staged) or bf16; out [N, H, W, Cin] fp32 or bf16 (RNE); addend and gate, where given, have out's type
 *     and shape.  k = 3 or 1, stride 1 or 2, Cout % 32 == 0 (a reduction chunk is 32 output channels of one tap), Cin % 16 == 0.
 *     bf16 products accumulate in fp32 (v_mfma_f32_16x16x32_bf16); the epilogue is fp32.  Every operand 16-byte aligned; out may
 *     not overlap an input.
 *   avf_conv2d_nhwc_dgrad_f32x3: the same operation, rules and tiles in the parity arithmetic of avf_conv2d_nhwc_f32x3: every
 *     map fp32, gy split into hi + lo as it is staged, wt_hi / wt_lo the split of fp32(w * scale), three bf16 products per pair.
 *   avf_conv_dgrad_plan: the tile both run a shape on, avf_conv_plan's rule on N*H*W rows and Cin columns: *tile = its id
 *     (0: 128 pixels x 64 channels, 1: 64 x 32), *tile_m / *tile_n its extent.  Same shape checks as the launch.
 *   avf_avgpool_nhwc_bwd: out[n, p, c] = gate[n, p, c] > 0 ? dout[n, c] / HW : 0 (gate null: dout[n, c] / HW); dout [N, C] fp32,
 *     gate (of out's type) and out [N, HW, C] fp32 or bf16; C % 8 == 0, every operand 16-byte aligned. */
int avf_conv2d_nhwc_dgrad(const void* gy, int gy_dtype, const void* wt_packed, const void* addend, const void* gate, int k,
                          int stride, void* out, int out_dtype, int N, int H, int W, int Cin, int Cout, void* stream);
int avf_conv2d_nhwc_dgrad_f32x3(const float* gy, const void* wt_hi, const void* wt_lo, const float* addend, const float* gate, int k,
                                int stride, float* out, int N, int H, int W, int Cin, int Cout, void* stream);
int avf_conv_dgrad_plan(int N, int H, int W, int Cin, int Cout, int k, int stride, int* tile, int* tile_m, int* tile_n);
int avf_avgpool_nhwc_bwd(const float* dout, const void* gate, void* out, int out_dtype, int64_t N, int HW, int C, void* stream);

/* ---- frozen ResNet stem, forward only (csrc/stem.hip) -----------------------------------------------------------------------
 * What stands in front of layer1: conv1 (7x7, stride 2, pad 3, bias=False) - bn1 - relu - maxpool (3x3, stride 2, pad 1) of
 * ResFormer.forward (vformer.py:238-241) and of the audio stream's ResNet18 (audio.py:22-39, one input channel), in ONE launch
 * from the front ends' NCHW planes to the NHWC map avf_conv2d_nhwc reads.  BatchNorm2d is folded in eval mode.  No gradients.
 *   avf_stem_packed_k: Kp, the row length of the packed weight image for Cin input channels (Cin in {1, 3, 4}: 64 / 192 / 224);
 *     0 and an error message for any other Cin.
 *   avf_stem_pack_weight: w [64, Cin, 7, 7] fp32 -> w_packed [64, Kp] bf16 (RNE); the order of a row and its zero padding are the
 *     kernel's own (csrc/stem.hip).  scale / shift [64] fp32 as avf_conv_pack_weight folds them (fp64), not multiplied into the
 *     weights.  Cout must be 64 and Cin in {1, 3, 4}: anything else is an error that names the limit.  Once per weight load.
 *   avf_stem_nchw: out[n, py, px, co] = max over the 3x3 window (2 py - 1 + dy, 2 px - 1 + dx) INSIDE the Hc x Wc conv map of
 *     relu( (sum_{ci,ky,kx} x[n, ci, 2 cy - 3 + ky, 2 cx - 3 + kx] * w[co, ci, ky, kx]) * scale[co] + shift[co] ); positions outside
 *     the image count as zero for the convolution and are never read, positions outside the conv map take no part in the max.
 *     Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1, the same for W; any H, W >= 1.  x [N, Cin, H, W] contiguous planes, fp32
 *     (rounded to bf16, RNE, as it is staged) or bf16, aligned to its element only (a 1001-wide row is not 16-byte aligned);
 *     nothing outside [x, x + N*Cin*H*W) is read.  out [N, Hp, Wp, 64] NHWC, fp32 or bf16 (RNE), 16-byte aligned as are
 *     w_packed / scale / shift; out may not overlap an input.  bf16 products accumulate in fp32 (v_mfma_f32_16x16x32_bf16); the
 *     epilogue and the max are fp32 arithmetic with one rounding per stored value.  Every global index is 64-bit.
 *   avf_stem_plan: the tile of POOLED outputs (of one image) a workgroup owns for this shape: *tile_h x *tile_w.  It computes the
 *     (2 tile_h + 1) x (2 tile_w + 1) conv pixels the tile needs itself (halo recompute).  Same argument checks as the launch.
 * The pool has a second geometry, that of the frozen VGGFace2 ResNet-50 (vggformer.py:71: MaxPool2d(3, 2, padding=0,
 * ceil_mode=True)), picked by pool_mode:
 *   AVF_STEM_POOL_PAD1 (0)  3x3 / 2 / pad 1, floor: windows start at 2 p - 1, Hp = (Hc - 1) / 2 + 1.  What avf_stem_nchw runs.
 *   AVF_STEM_POOL_CEIL (1)  3x3 / 2 / pad 0, ceil_mode: windows start at 2 p, Hp = (Hc - 2) / 2 + 1 (torch's max_pool2d rule); a
 *     window that hangs over the bottom / right edge of the conv map takes the max over the pixels inside the map.  torch has no
 *     output for a conv map smaller than 2 x 2: H < 3 or W < 3 is an error that says so.
 *   avf_stem_nchw_pool: avf_stem_nchw with the pool geometry as an argument (a template parameter of the same kernel: the tile,
 *     the packed image and every other contract above are unchanged; mode 0 IS avf_stem_nchw, bit for bit).  Any other pool_mode
 *     is an error that names the two.
 *   avf_stem_out_hw: host only, no device call: the shape rule the launch itself acts on - *Hc x *Wc the conv map, *Hp x *Wp the
 *     pooled map of an H x W image under pool_mode.  Same errors as the launch for the mode and the sizes. */
#define AVF_STEM_POOL_PAD1 0
#define AVF_STEM_POOL_CEIL 1
int avf_stem_packed_k(int Cin);
int avf_stem_pack_weight(const float* w, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, double eps, void* w_packed, float* scale, float* shift, int Cout, int Cin,
                         void* stream);
int avf_stem_nchw(const void* x, int x_dtype, const void* w_packed, const float* scale, const float* shift, void* out,
                  int out_dtype, int N, int Cin, int H, int W, void* stream);
int avf_stem_plan(int N, int Cin, int H, int W, int* tile_h, int* tile_w);
int avf_stem_nchw_pool(const void* x, int x_dtype, const void* w_packed, const float* scale, const float* shift, void* out,
                       int out_dtype, int N, int Cin, int H, int W, int pool_mode, void* stream);
int avf_stem_out_hw(int H, int W, int pool_mode, int* Hc, int* Wc, int* Hp, int* Wp);

/* test aid: the keep/(1-p) factors (0 or 1/(1-p_eff)) dropout site `site` (0 after to_out, 1 after GELU, 2 after
 * net.3) of layer `layer_index` applies to a [rows, cols] activation, as fp32 [rows, cols] (cols % 4 == 0). */
int avf_dropout_factors(uint32_t seed_lo, uint32_t seed_hi, int layer_index, int site, float p, int64_t rows, int cols,
                        float* out, void* stream);

/* ---- arithmetic of the AVF_F32 (parity) mode (round 6) ------------------------------------------------------------
 * The AVF_F32 GEMMs and the attention core (the fp32 aten::mm / bmm / softmax under models/heads.py:191-196, 212-238) run
 *   mode 1 ("bf16x3", default): every fp32 operand split as x = hi + lo (two bf16), a b ~ hi hi + hi lo + lo hi on
 *           v_mfma_f32_16x16x32_bf16 with fp32 accumulation: <= 3 * 2^-16 = 4.6e-5 relative error per product in the worst case,
 *           4e-6 typical (measured relative Frobenius error of a GEMM), 3 MFMAs per product;
 *   mode 0 ("f32"): the f32-input MFMA v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain, 1/16 of the bf16 rate).
 * Both hold north_star's logits rtol 1e-3; shapes the bf16x3 kernels do not take (fewer than 96 rows or columns, ragged K on the
 * contiguous axis, token masks, bf16 storage) run the mode-0 kernels in either mode.
 * The arithmetic travels with the call.  avf_layer_cfg carries its own (f32_arith).  The operator-level entry points have no
 * argument for it (avf_gemm, avf_gemm_f32_ex, avf_gemm_f32_plan, avf_gemm_f32_tn_group*, avf_attn_fwd, avf_attn_bwd,
 * avf_attn_*_masked, avf_attn_parity_plan): each reads the process-wide DEFAULT set here, once, when it is called.
 * avf_set_f32_arith returns the previous default. */
int avf_set_f32_arith(int mode);
int avf_get_f32_arith(void);

/* After a FAILED hipGraph capture of a step (something that cannot be recorded was issued while `stream` was capturing - e.g. a
 * host-synchronising collective): ends a capture still open on `stream`, discards its graph and clears the runtime's sticky
 * last-error so that the caller can continue with eager launches.  Returns the HIP error code that was pending (0: none). */
int avf_hip_error_reset(void* stream);

/* A last line for a process that may die inside an OPTIONAL step (bench.py's multi-rank hipGraph attempt, which follows a completed
 * eager measurement): while armed, SIGSEGV / SIGBUS / SIGABRT / SIGFPE / SIGILL write `line` to `fd` (write(2); fd < 0: nothing) and
 * leave with _exit(0).  _disarm restores the previous handlers.  Process-wide; not for product code paths. */
int avf_crash_line_arm(const char* line, int fd);
int avf_crash_line_disarm(void);

/* ---- optional HIP-event timing per kernel class (bench.py's roofline line) --------------------------
 * classes: 0 gemm_bf16_nt, 1 gemm_bf16_tn(+fold), 2 gemm_f32, 3 attn_fwd, 4 attn_bwd, 5 layernorm, 6 other, 7 gemm_mx8_nt.
 * enable(1) resets the records; read() synchronises the recorded events and sums them.  Every class but 2 and 6
 * attaches one event pair to each kernel dispatch (its own begin / end timestamps, as a profiler reports them; `launches`
 * counts dispatches); 2 and 6 record a pair around the launches of one call (~2 us of command-processor time each). */
int avf_timing_enable(int on);
int avf_timing_read(int cls, double* total_ms, int64_t* launches, double* flops, double* bytes);

/* ---- hardware self-tests used by tests/ (MFMA fragment maps, transposed LDS read) ----------- */
int avf_selftest_mfma_bf16(const void* a_bf16_16x32, const void* b_bf16_32x16, float* c_16x16, void* stream);
int avf_selftest_mfma_f32(const float* a_16x4, const float* b_4x16, float* c_16x16, void* stream);
int avf_selftest_tr16(const void* tile_bf16_32x16, void* out_bf16_64x8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AVFORMER_HIP_H */
