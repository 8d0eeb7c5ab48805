// conv_common.hpp - what the two NHWC implicit-GEMM convolutions share (conv.hip: bf16 operands; conv_f32.hip: fp32 operands in
// the bf16x3 parity arithmetic): the argument block, the LDS swizzle, the shape rules, the tile table and its dispatch rule, and
// the small predicates of the entry points.  Everything has internal linkage: each source gets its own copy.
#pragma once
#include "common.hpp"

namespace avf {
namespace {

constexpr int kConvThreads = 256;  // four waves, stacked along the pixel axis of the tile
constexpr int kConvBK = 32;        // one MFMA deep

struct ConvArgs {
  const void* x;
  const bf16* w;  // packed [Cout][K]
  const float *scale, *shift;
  const void* res;
  void* out;
  int N, H, W, Cin, Cout, k, stride, pad, Ho, Wo, K;
  int64_t M;
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
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace avf
