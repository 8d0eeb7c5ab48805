// stem.hip - the frozen ResNet stem in front of layer1 (vformer.py:238-241; audio.py:22-39 with one input channel), forward only:
//   stem_nchw_kernel         conv 7x7 / stride 2 / pad 3 -> folded eval-mode BatchNorm -> ReLU -> maxpool 3x3 / stride 2 in one
//                            launch: NCHW planes (fp32 or bf16, Cin = 1 / 3 / 4) in, NHWC [N, Hp, Wp, 64] out - what layer1 reads.
//                            The pool is pad 1 / floor (AVF_STEM_POOL_PAD1: vformer.py:241, torchvision's ResNet) or pad 0 /
//                            ceil_mode (AVF_STEM_POOL_CEIL: VGGFace2's ResNet-50, vggformer.py:71)
//   stem_pack_weight_kernel  nn.Conv2d's [64, Cin, 7, 7] fp32 weight -> the [64, Kp] bf16 image below, BatchNorm2d's running
//                            statistics -> one (scale, shift) pair per channel
//
// A workgroup owns a 7 x 7 tile of POOLED outputs of one image (28 x 28 pooled pixels of a 112 x 112 frame are 4 x 4 tiles).
// The tile needs the 15 x 15 conv pixels (2 * py0 - pad .. 2 * py0 - pad + 14, pad the pool's padding: 1 or 0) and those the
// 35 x 35 input pixels from 4 * py0 - 2 * pad - 3 on (-5 or -3 at the image corner), of every channel: only these two origins
// depend on the pool geometry, a template parameter of the kernel (PAD; the pad-1 instantiation is the kernel as it was).  The
// patch is staged in LDS as bf16, zero where it leaves the image (no load is issued there).  The halo conv pixels are recomputed
// by the neighbouring tiles (225 / 196 = 1.15 x the convolution) so that no tile reads another's.
//
// GEMM view of the convolution: rows = the 64 channels (the MFMA's A operand), columns = the tile's 225 conv pixels in 15
// fragments of 16 (the B operand), reduction ordered (ci, ky, kx padded to 8): the eight k-values of a lane are eight
// consecutive columns of ONE patch row - pixel (cy, cx), row (ci, ky) reads patch[ci][2 cy + ky][2 cx .. 2 cx + 7] - and the
// eighth is a padded tap: its weight is zero and the lane zeroes its value too (a NaN beside the window stays outside).
// Kp = Cin * 56 rounded up to the MFMA's 32: 64 / 192 / 224, the rows past Cin * 7 zero on both sides.  The weights are read
// once per workgroup into registers (the grid is persistent: a workgroup walks tiles blockIdx.x, + gridDim.x, ...).  scale /
// shift wait in LDS for the epilogues.
//
// The conv map of the tile goes to LDS after the epilogue (y = acc * scale + shift, ReLU; fp32), in the OUTPUT's type - max and
// a monotone rounding commute, so rounding before the max gives the bits of rounding after it - with -inf at the pixels outside
// the Hc x Wc map, which therefore never win a max.  The pool reads 3 x 3 windows of it, eight channels (16 bytes of bf16) per
// lane, and stores them: one rounding on the way to memory.
#include "conv_common.hpp"  // the entry points' predicates and the BatchNorm fold

namespace avf {
namespace {

constexpr int kStemThreads = 256;            // four waves; a wave takes conv-pixel fragments wave, wave + 4, ...
constexpr int kStemCout = 64;
constexpr int kStemTH = 7, kStemTW = 7;      // the pooled tile
constexpr int kStemCH = 2 * kStemTH + 1, kStemCW = 2 * kStemTW + 1;      // its conv pixels: 15 x 15
constexpr int kStemPix = kStemCH * kStemCW;                              // 225
constexpr int kStemFrags = (kStemPix + 15) / 16;                         // 15
constexpr int kStemPH = 4 * kStemTH + 7, kStemPW = 4 * kStemTW + 8;      // the input patch: 35 rows, 35 columns + the padded tap's
constexpr int kStemMapPad = 8;               // conv-map row = 64 + 8 elements: 16-byte aligned rows that do not share banks

constexpr int stem_kp(int cin) { return (cin * 56 + 31) / 32 * 32; }
constexpr size_t stem_lds_bytes(int cin, size_t out_elt) {
  return (size_t)cin * kStemPH * kStemPW * 2 + (size_t)kStemPix * (kStemCout + kStemMapPad) * out_elt + 2 * kStemCout * sizeof(float);
}

struct StemArgs {
  const void* x;
  const bf16* w;  // packed [64][Kp]
  const float *scale, *shift;
  void* out;
  int N, H, W, Hc, Wc, Hp, Wp, tiles_y, tiles_x;
  int pad;        // the pool's padding: 1 (AVF_STEM_POOL_PAD1) or 0 (AVF_STEM_POOL_CEIL), the kernel's PAD; Hp, Wp follow the mode's size rule
  int64_t tiles;  // N * tiles_y * tiles_x
};

// NaN-propagating max, as torch's max_pool2d
__device__ __forceinline__ float stem_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <typename OT>
struct MapIO;
template <>
struct MapIO<bf16> {  // four / eight consecutive channels of one conv pixel
  static __device__ __forceinline__ void put4(bf16* p, const float (&v)[4]) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
  }
  static __device__ __forceinline__ void get8(const bf16* p, float (&v)[8]) { unpack8(*reinterpret_cast<const uint4*>(p), v); }
  static __device__ __forceinline__ void store8(bf16* p, const float (&v)[8]) { *reinterpret_cast<uint4*>(p) = pack8(v); }
};
template <>
struct MapIO<float> {
  static __device__ __forceinline__ void put4(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
  static __device__ __forceinline__ void get8(const float* p, float (&v)[8]) { load8f(p, v); }
  static __device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
};

template <typename XT, typename OT, int CIN, int PAD>
__global__ __launch_bounds__(kStemThreads) __attribute__((amdgpu_waves_per_eu(2))) void stem_nchw_kernel(const StemArgs a) {
  static_assert(PAD == 0 || PAD == 1, "the pool's padding");
  constexpr int KP = stem_kp(CIN), NS = KP / 32, ROWS = CIN * 7;  // k-steps; the (ci, ky) rows that exist
  constexpr int MAPW = kStemCout + kStemMapPad;
  constexpr int PLANE = kStemPH * kStemPW;
  extern __shared__ __attribute__((aligned(16))) unsigned char stem_lds[];
  OT* cmap = reinterpret_cast<OT*>(stem_lds);                                                      // [225][72], 16-byte rows
  float* ss = reinterpret_cast<float*>(stem_lds + (size_t)kStemPix * MAPW * sizeof(OT));            // scale[64], shift[64]
  uint16_t* patch = reinterpret_cast<uint16_t*>(ss + 2 * kStemCout);                               // [CIN][35][36] bf16
  static_assert((kStemPix * MAPW * sizeof(OT)) % 16 == 0 && (MAPW * sizeof(OT)) % 16 == 0 && PLANE % 2 == 0 && kStemPW % 2 == 0, "alignment");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const XT* x = reinterpret_cast<const XT*>(a.x);
  OT* out = reinterpret_cast<OT*>(a.out);

  // the weights, once: fragment (step s, channel group f) holds channel f * 16 + (lane & 15), k = s * 32 + g * 8 .. + 7
  bf16x8_t wf[NS][4];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      wf[s][f] = *reinterpret_cast<const bf16x8_t*>(a.w + (f * 16 + (lane & 15)) * KP + s * 32 + g * 8);
  // scale and shift wait in LDS for the epilogues (32 registers fewer per lane: what the patch prefetch lives in); the first
  // barrier of the tile loop stands between this write and their first read
  if (tid < 2 * kStemCout) ss[tid] = tid < kStemCout ? a.scale[tid] : a.shift[tid - kStemCout];
  // patch offset of this lane's (ci, ky) row in step s; a row past the last has zero weights and gets a zero fragment
  int roff[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int r = s * 4 + g;
    roff[s] = r < ROWS ? ((r / 7) * kStemPH + r % 7) * kStemPW : -1;
  }

  // The patch of a tile: fetch() issues every load of it (a thread takes two neighbouring columns per turn; x needs element
  // alignment only) and keeps the raw values, stash() rounds them to bf16 and writes 4 bytes per turn.  Up to three channels
  // the NEXT tile is fetched before the MFMA phase of this one and stashed after its pool, so the loads travel behind the
  // arithmetic; with four channels the registers for that are not there and the tile is fetched where it is stashed.
  constexpr int PAIRS = CIN * kStemPH * (kStemPW / 2), TURNS = (PAIRS + kStemThreads - 1) / kStemThreads;
  constexpr bool PREFETCH = CIN <= 3;
  using Raw = typename std::conditional<std::is_same<XT, float>::value, float, uint32_t>::type;  // a bf16 comes as its 16 bits
  Raw r0[TURNS], r1[TURNS];
  auto fetch = [&](int64_t t) {
    const int64_t n = t / (a.tiles_y * a.tiles_x);
    const int tr = (int)(t - n * (a.tiles_y * a.tiles_x));
    const int ty = tr / a.tiles_x, tx = tr - ty * a.tiles_x;
    const int iy0 = 4 * ty * kStemTH - 2 * PAD - 3, ix0 = 4 * tx * kStemTW - 2 * PAD - 3;  // the first input pixel: 2 * (2 * py0 - PAD) - 3
#pragma unroll
    for (int i = 0; i < TURNS; ++i) {
      const int q = tid + i * kStemThreads;
      const int ci = q / (kStemPH * (kStemPW / 2)), rq = q - ci * (kStemPH * (kStemPW / 2));
      const int r = rq / (kStemPW / 2), c = (rq - r * (kStemPW / 2)) * 2;
      const int iy = iy0 + r, ix = ix0 + c;
      r0[i] = r1[i] = Raw(0);
      if (q < PAIRS && (unsigned)iy < (unsigned)a.H) {
        const XT* row = x + ((n * CIN + ci) * a.H + iy) * (int64_t)a.W;
        if constexpr (std::is_same<XT, float>::value) {
          if ((unsigned)ix < (unsigned)a.W) r0[i] = row[ix];
          if ((unsigned)(ix + 1) < (unsigned)a.W) r1[i] = row[ix + 1];
        } else {
          if ((unsigned)ix < (unsigned)a.W) r0[i] = row[ix].x;
          if ((unsigned)(ix + 1) < (unsigned)a.W) r1[i] = row[ix + 1].x;
        }
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < TURNS; ++i) {
      const int q = tid + i * kStemThreads;
      if (q >= PAIRS) continue;
      uint32_t v;
      if constexpr (std::is_same<XT, float>::value) v = pack_bf16x2(r0[i], r1[i]);  // RNE
      else v = r0[i] | (r1[i] << 16);
      *reinterpret_cast<uint32_t*>(patch + 2 * q) = v;  // pair q IS bytes 4 q .. 4 q + 3 of [CIN][35][36]
    }
  };

  if (PREFETCH && (int64_t)blockIdx.x < a.tiles) fetch(blockIdx.x);
  for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const int64_t n = t / (a.tiles_y * a.tiles_x);
    const int tr = (int)(t - n * (a.tiles_y * a.tiles_x));
    const int ty = tr / a.tiles_x, tx = tr - ty * a.tiles_x;
    const int py0 = ty * kStemTH, px0 = tx * kStemTW;
    const int cy0 = 2 * py0 - PAD, cx0 = 2 * px0 - PAD;      // the tile's first conv pixel

    if (!PREFETCH) fetch(t);
    stash();
    __syncthreads();
    if (PREFETCH && t + gridDim.x < a.tiles) fetch(t + gridDim.x);

    // ---- the convolution of the tile's 225 pixels, 16 at a time, and its epilogue into the conv map
    for (int fi = wave; fi < kStemFrags; fi += 4) {
      const int p = fi * 16 + (lane & 15);
      const int pc = p < kStemPix ? p : kStemPix - 1;  // the last fragment's spare columns compute a pixel nobody keeps
      const int cyl = pc / kStemCW, cxl = pc - cyl * kStemCW;
      const uint16_t* base = patch + 2 * cyl * kStemPW + 2 * cxl;
      f32x4_t acc[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(base + (roff[s] < 0 ? 0 : roff[s]));  // 4-byte aligned: 2 cx is even
        uint4 v = make_uint4(src[0], src[1], src[2], src[3] & 0xffffu);                               // kx = 7: the padded tap
        if (NS * 4 > ROWS && roff[s] < 0) v = make_uint4(0u, 0u, 0u, 0u);
        const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, v);
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][f], pf, acc[f], 0, 0, 0);
      }
      if (p < kStemPix) {
        const int cy = cy0 + cyl, cx = cx0 + cxl;
        const bool inside = (unsigned)cy < (unsigned)a.Hc && (unsigned)cx < (unsigned)a.Wc;
#pragma unroll
        for (int f = 0; f < 4; ++f) {  // channels f * 16 + g * 4 + r
          const float4 s4 = *reinterpret_cast<const float4*>(ss + f * 16 + g * 4), h4 = *reinterpret_cast<const float4*>(ss + kStemCout + f * 16 + g * 4);
          const float sc[4] = {s4.x, s4.y, s4.z, s4.w}, sh[4] = {h4.x, h4.y, h4.z, h4.w};
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float y = acc[f][r] * sc[r] + sh[r];
            v[r] = inside ? (y < 0.f ? 0.f : y) : -INFINITY;  // (a NaN stays a NaN)
          }
          MapIO<OT>::put4(cmap + p * MAPW + f * 16 + g * 4, v);
        }
      }
    }
    __syncthreads();

    // ---- the pool: a lane takes eight channels of one pooled pixel; window rows 2 py - PAD .. + 2 are map rows 2 ply .. + 2 in
    // either geometry.  A ceil-mode window that hangs over the bottom / right edge of the conv map reads the -inf written above
    // at cy >= Hc / cx >= Wc, as the pad-1 window does at cy = -1: the max is over the pixels inside the map
    for (int q = tid; q < kStemTH * kStemTW * 8; q += kStemThreads) {
      const int pp = q >> 3, c8 = (q & 7) * 8;
      const int ply = pp / kStemTW, plx = pp - ply * kStemTW;
      const int py = py0 + ply, px = px0 + plx;
      if (py >= a.Hp || px >= a.Wp) continue;
      float m[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          float v[8];
          MapIO<OT>::get8(cmap + ((2 * ply + dy) * kStemCW + 2 * plx + dx) * MAPW + c8, v);
#pragma unroll
          for (int e = 0; e < 8; ++e) m[e] = stem_max(m[e], v[e]);
        }
      MapIO<OT>::store8(out + ((n * a.Hp + py) * a.Wp + px) * kStemCout + c8, m);
    }
    // the next turn's stash writes the patch only, which nobody reads here; its barrier stands before the next map write
  }
}

// one thread per element of the packed image; the first 64 threads also fold their channel's BatchNorm in fp64
__global__ __launch_bounds__(256) void stem_pack_weight_kernel(const float* w, const float* gamma, const float* beta, const float* mean,
                                                               const float* var, double eps, bf16* wp, float* scale, float* shift,
                                                               int Cin, int Kp) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kStemCout * Kp) return;
  const int co = idx / Kp, k = idx - co * Kp;
  const int row = k >> 3, kx = k & 7;  // row = ci * 7 + ky
  float v = 0.f;
  if (row < Cin * 7 && kx < 7) v = w[(co * Cin * 7 + row) * 7 + kx];
  wp[idx] = from_f32<bf16>(v);
  if (idx < kStemCout) bn_fold(gamma, beta, mean, var, eps, idx, scale, shift);
}

bool stem_cin_ok(int Cin) { return Cin == 1 || Cin == 3 || Cin == 4; }

// The shape rule of both pool geometries, torch's max_pool2d output size: conv map L -> floor((L + 2 - 3) / 2) + 1 with pad 1;
// ceil((L - 3) / 2) + 1 = (L - 2) / 2 + 1 with pad 0 and ceil_mode (L >= 2; the last window starts at 2 * ((L - 2) / 2) <= L - 2,
// inside the map, so torch's "last window must start inside the input" correction never applies).
int stem_out_hw(const char* who, int H, int W, int pool_mode, int* Hc, int* Wc, int* Hp, int* Wp) {
  AVF_REQUIRE(pool_mode == AVF_STEM_POOL_PAD1 || pool_mode == AVF_STEM_POOL_CEIL,
              "%s: pool_mode=%d: the stem pool is AVF_STEM_POOL_PAD1 (0: 3x3 / 2 / pad 1, floor) or AVF_STEM_POOL_CEIL (1: 3x3 / 2 / pad 0, "
              "ceil_mode)", who, pool_mode);
  AVF_REQUIRE(H > 0 && W > 0, "%s: empty shape (H=%d W=%d)", who, H, W);
  *Hc = (H - 1) / 2 + 1; *Wc = (W - 1) / 2 + 1;
  if (pool_mode == AVF_STEM_POOL_CEIL) {
    AVF_REQUIRE(H >= 3 && W >= 3, "%s: H=%d W=%d with AVF_STEM_POOL_CEIL: the conv map %d x %d is smaller than 2 x 2, for which "
                "max_pool2d(3, 2, padding=0, ceil_mode=True) has no output; H and W must be at least 3", who, H, W, *Hc, *Wc);
    *Hp = (*Hc - 2) / 2 + 1; *Wp = (*Wc - 2) / 2 + 1;
  } else {
    *Hp = (*Hc - 1) / 2 + 1; *Wp = (*Wc - 1) / 2 + 1;
  }
  return 0;
}

int stem_shape(const char* who, int N, int Cin, int H, int W, int pool_mode, StemArgs* a) {
  AVF_REQUIRE(N > 0 && H > 0 && W > 0, "%s: empty shape (N=%d H=%d W=%d)", who, N, H, W);
  AVF_REQUIRE(stem_cin_ok(Cin), "%s: Cin=%d: the stem kernel takes 1, 3 or 4 input channels (and writes 64)", who, Cin);
  a->N = N; a->H = H; a->W = W;
  AVF_TRY(stem_out_hw(who, H, W, pool_mode, &a->Hc, &a->Wc, &a->Hp, &a->Wp));
  a->pad = pool_mode == AVF_STEM_POOL_CEIL ? 0 : 1;
  a->tiles_y = (int)ceil_div(a->Hp, kStemTH);
  a->tiles_x = (int)ceil_div(a->Wp, kStemTW);
  AVF_REQUIRE((int64_t)a->tiles_y * a->tiles_x < (1ll << 31), "%s: too many tiles per image", who);
  a->tiles = (int64_t)N * a->tiles_y * a->tiles_x;
  return 0;
}

template <typename XT, typename OT, int CIN, int PAD>
int stem_launch_pad(const StemArgs& a, hipStream_t s) {
  constexpr size_t lds = stem_lds_bytes(CIN, sizeof(OT));
  static_assert(lds <= 80 * 1024, "two workgroups per CU");
  static PerDeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)stem_nchw_kernel<XT, OT, CIN, PAD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    AVF_REQUIRE(e == hipSuccess, "stem_nchw: cannot raise dynamic LDS limit: %s", hipGetErrorString(e));
    raised.mark();
  }
  // persistent: as many workgroups as stay resident - two per CU by registers, four for one channel and a bf16 map
  constexpr int64_t slots = (CIN == 1 && sizeof(OT) == 2) ? 2 * kWorkgroupSlots : kWorkgroupSlots;
  const unsigned grid = (unsigned)(a.tiles < slots ? a.tiles : slots);
  stem_nchw_kernel<XT, OT, CIN, PAD><<<grid, kStemThreads, lds, s>>>(a);
  return check_launch("stem_nchw");
}
template <typename XT, typename OT, int CIN>
int stem_launch_cin(const StemArgs& a, hipStream_t s) {
  return a.pad ? stem_launch_pad<XT, OT, CIN, 1>(a, s) : stem_launch_pad<XT, OT, CIN, 0>(a, s);
}
template <typename XT, typename OT>
int stem_launch_out(const StemArgs& a, int Cin, hipStream_t s) {
  if (Cin == 1) return stem_launch_cin<XT, OT, 1>(a, s);
  if (Cin == 3) return stem_launch_cin<XT, OT, 3>(a, s);
  return stem_launch_cin<XT, OT, 4>(a, s);
}
template <typename XT>
int stem_launch_x(const StemArgs& a, int Cin, int out_dtype, hipStream_t s) {
  return out_dtype == AVF_F32 ? stem_launch_out<XT, float>(a, Cin, s) : stem_launch_out<XT, bf16>(a, Cin, s);
}

}  // namespace
}  // namespace avf

using namespace avf;

extern "C" int avf_stem_packed_k(int Cin) {
  if (!stem_cin_ok(Cin)) {
    set_error("stem_packed_k: Cin=%d: the stem kernel takes 1, 3 or 4 input channels", Cin);
    return 0;
  }
  return stem_kp(Cin);
}

extern "C" int avf_stem_plan(int N, int Cin, int H, int W, int* tile_h, int* tile_w) {
  AVF_REQUIRE(tile_h && tile_w, "stem_plan: null pointer");
  StemArgs a;
  AVF_TRY(stem_shape("stem_plan", N, Cin, H, W, AVF_STEM_POOL_PAD1, &a));
  *tile_h = kStemTH;
  *tile_w = kStemTW;
  return 0;
}

extern "C" int avf_stem_pack_weight(const float* w, const float* gamma, const float* beta, const float* running_mean,
                                    const float* running_var, double eps, void* w_packed, float* scale, float* shift, int Cout,
                                    int Cin, void* stream) {
  AVF_REQUIRE(w && gamma && beta && running_mean && running_var && w_packed && scale && shift, "stem_pack_weight: null pointer");
  AVF_REQUIRE(Cout == kStemCout, "stem_pack_weight: Cout=%d: the stem kernel writes 64 channels", Cout);
  AVF_REQUIRE(stem_cin_ok(Cin), "stem_pack_weight: Cin=%d: the stem kernel takes 1, 3 or 4 input channels", Cin);
  AVF_REQUIRE(eps >= 0.0, "stem_pack_weight: eps %g", eps);
  const int Kp = stem_kp(Cin);
  AVF_REQUIRE(apart(w_packed, (size_t)Cout * Kp * 2, w, (size_t)Cout * Cin * 49 * 4) && apart(scale, (size_t)Cout * 4, shift, (size_t)Cout * 4),
              "stem_pack_weight: an output overlaps an input or another output");
  stem_pack_weight_kernel<<<(unsigned)ceil_div((int64_t)Cout * Kp, 256), 256, 0, (hipStream_t)stream>>>(
      w, gamma, beta, running_mean, running_var, eps, (bf16*)w_packed, scale, shift, Cin, Kp);
  return check_launch("stem_pack_weight");
}

extern "C" int avf_stem_out_hw(int H, int W, int pool_mode, int* Hc, int* Wc, int* Hp, int* Wp) {
  AVF_REQUIRE(Hc && Wc && Hp && Wp, "stem_out_hw: null pointer");
  return stem_out_hw("stem_out_hw", H, W, pool_mode, Hc, Wc, Hp, Wp);
}

extern "C" int avf_stem_nchw(const void* x, int x_dtype, const void* w_packed, const float* scale, const float* shift, void* out,
                             int out_dtype, int N, int Cin, int H, int W, void* stream) {
  return avf_stem_nchw_pool(x, x_dtype, w_packed, scale, shift, out, out_dtype, N, Cin, H, W, AVF_STEM_POOL_PAD1, stream);
}

extern "C" int avf_stem_nchw_pool(const void* x, int x_dtype, const void* w_packed, const float* scale, const float* shift, void* out,
                                  int out_dtype, int N, int Cin, int H, int W, int pool_mode, void* stream) {
  AVF_REQUIRE(x && w_packed && scale && shift && out, "stem_nchw: null pointer");
  AVF_REQUIRE(is_dtype(x_dtype) && is_dtype(out_dtype), "stem_nchw: bad dtype (x %d, out %d)", x_dtype, out_dtype);
  StemArgs a;
  AVF_TRY(stem_shape("stem_nchw", N, Cin, H, W, pool_mode, &a));
  AVF_REQUIRE(aligned(x, elt(x_dtype)), "stem_nchw: x must be aligned to its element");
  AVF_REQUIRE(aligned(w_packed, 16) && aligned(scale, 16) && aligned(shift, 16) && aligned(out, 16),
              "stem_nchw: w_packed, scale, shift and out must be 16-byte aligned");
  const size_t xn = (size_t)N * Cin * H * W * elt(x_dtype), on = (size_t)N * a.Hp * a.Wp * kStemCout * elt(out_dtype);
  AVF_REQUIRE(apart(out, on, x, xn) && apart(out, on, w_packed, (size_t)kStemCout * stem_kp(Cin) * 2) &&
                  apart(out, on, scale, (size_t)kStemCout * 4) && apart(out, on, shift, (size_t)kStemCout * 4),
              "stem_nchw: out overlaps an input (a tile reads pixels other tiles' outputs would cover)");
  a.x = x; a.w = (const bf16*)w_packed; a.scale = scale; a.shift = shift; a.out = out;
  const hipStream_t s = (hipStream_t)stream;
  return x_dtype == AVF_F32 ? stem_launch_x<float>(a, Cin, out_dtype, s) : stem_launch_x<bf16>(a, Cin, out_dtype, s);
}
