// conv_common.hpp - the host side of the NHWC implicit-GEMM convolution (conv_kernel.hpp; conv.hip instantiates it with bf16
// operands, conv_f32.hip with fp32 operands in the bf16x3 parity arithmetic): the argument block, the LDS swizzle, the shape
// rules, the tile table and its dispatch rule, the operand checks of the entry points - and what stem.hip shares with them: the
// small predicates and the BatchNorm fold.  Everything has internal linkage: each source gets its own copy.
#pragma once
#include "common.hpp"

namespace avf {
namespace {

constexpr int kConvThreads = 256;  // four waves, stacked along the pixel axis of the tile
constexpr int kConvBK = 32;        // one MFMA deep

struct ConvArgs {
  const void* x;
  const bf16* w;  // packed [Cout][K]: the one bf16 image, or the hi image of the bf16x3 form
  const float *scale, *shift;
  const void* res;
  void* out;
  int N, H, W, Cin, Cout, k, stride, pad, Ho, Wo, K;
  int64_t M;
  const bf16* w_lo;  // the lo image, as w (bf16x3 form; else null)
};

// A tile row is one chunk of one pixel / one output channel: 32 bf16 = four 16-byte pieces, four rows per 256-byte bank row.
// A fragment read takes row (lane & 15), piece (lane >> 4); ds_read_b128 serves lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
// (and the same + 32) together.  With the piece index XORed by f(row / 4), f = (0, 2, 3, 1), each of those groups lands on 16
// distinct 16-byte slots of the bank row: group one reads rows 0-3 and 12-15 at piece 0 (slots 4r + 0, 4r + 1) and rows 4-11 at
// piece 1 (slots 4r + 3, 4r + 2); the others follow by symmetry.
__device__ __forceinline__ int conv_lds_off(int row, int piece) {
  return row * 64 + ((piece ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3)) << 4);
}

// the tile shapes; conv_plan picks one, the launcher acts on exactly that
struct ConvTile { int bm, bn; };
constexpr ConvTile kConvTiles[2] = {{128, 64}, {64, 32}};

int conv_shape(const char* who, int N, int H, int W, int Cin, int Cout, int k, int stride, ConvArgs* a) {
  AVF_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "%s: empty shape (N=%d H=%d W=%d Cin=%d Cout=%d)", who, N, H, W, Cin, Cout);
  AVF_REQUIRE(k == 3 || k == 1, "%s: kernel size %d: 3 (pad 1) or 1 (pad 0)", who, k);
  AVF_REQUIRE(stride == 1 || stride == 2, "%s: stride %d: 1 or 2", who, stride);
  AVF_REQUIRE(Cin % kConvBK == 0, "%s: Cin=%d: Cin %% 32 == 0 (a reduction chunk is 32 channels of one tap)", who, Cin);
  AVF_REQUIRE(Cout % 16 == 0, "%s: Cout=%d: Cout %% 16 == 0", who, Cout);
  AVF_REQUIRE((int64_t)k * k * Cin < (1 << 30), "%s: reduction too deep", who);
  a->N = N; a->H = H; a->W = W; a->Cin = Cin; a->Cout = Cout; a->k = k; a->stride = stride;
  a->pad = k == 3 ? 1 : 0;
  a->Ho = (H + 2 * a->pad - k) / stride + 1;
  a->Wo = (W + 2 * a->pad - k) / stride + 1;
  a->K = k * k * Cin;
  a->M = (int64_t)N * a->Ho * a->Wo;
  AVF_REQUIRE((int64_t)a->Ho * a->Wo < (1ll << 31) && ceil_div(a->M, 64) < (1ll << 31), "%s: too many output pixels", who);
  return 0;
}

// the large tile once it gives every CU a workgroup, else the small one (batch-1 inference: M = 256 ... 12544)
int conv_plan(const ConvArgs& a) {
  const int64_t big = ceil_div(a.M, kConvTiles[0].bm) * ceil_div(a.Cout, kConvTiles[0].bn);
  return big >= kWorkgroupSlots / 2 ? 0 : 1;
}

bool is_dtype(int d) { return d == AVF_F32 || d == AVF_BF16; }
size_t elt(int d) { return d == AVF_F32 ? 4 : 2; }
bool apart(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a + pn <= b || b + qn <= a;
}
bool aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }  // n: a power of two

// What the two conv entry points check before they launch, in this order: no null operand, the dtypes, the shape (conv_shape
// fills a's geometry), 16-byte alignment, out apart from every input.  a comes with its pointers set; images = 2 needs w_lo.
int conv_operands(const char* who, ConvArgs* a, int images, int x_dtype, int res_dtype, int out_dtype, int N, int H, int W, int Cin,
                  int Cout, int k, int stride) {
  AVF_REQUIRE(a->x && a->w && (images == 1 || a->w_lo) && a->scale && a->shift && a->out, "%s: null pointer", who);
  AVF_REQUIRE(is_dtype(x_dtype) && is_dtype(out_dtype) && (!a->res || is_dtype(res_dtype)), "%s: bad dtype (x %d, out %d, residual %d)", who,
              x_dtype, out_dtype, res_dtype);
  AVF_TRY(conv_shape(who, N, H, W, Cin, Cout, k, stride, a));
  const void* in[] = {a->x, a->w, a->w_lo, a->scale, a->shift, a->res};
  const size_t wn = (size_t)Cout * a->K * 2, cn = (size_t)Cout * 4, on = (size_t)a->M * Cout * elt(out_dtype);
  const size_t bytes[] = {(size_t)N * H * W * Cin * elt(x_dtype), wn, wn, cn, cn, (size_t)a->M * Cout * elt(res_dtype)};
  bool al = aligned(a->out, 16), ap = true;
  for (int i = 0; i < 6; ++i) {
    al = al && aligned(in[i], 16);
    ap = ap && (!in[i] || apart(a->out, on, in[i], bytes[i]));
  }
  AVF_REQUIRE(al, "%s: every operand must be 16-byte aligned", who);
  AVF_REQUIRE(ap, "%s: out overlaps an input (a tile reads pixels other tiles write)", who);
  return 0;
}

// eval-mode BatchNorm2d of channel c as one (scale, shift) pair: y = x * scale + shift, folded in fp64
__device__ __forceinline__ void bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, double eps, int64_t c,
                                        float* scale, float* shift) {
  const double s = (double)gamma[c] / sqrt((double)var[c] + eps);
  scale[c] = (float)s;
  shift[c] = (float)((double)beta[c] - (double)mean[c] * s);
}

}  // namespace
}  // namespace avf
