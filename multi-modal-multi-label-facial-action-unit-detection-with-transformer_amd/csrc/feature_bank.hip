// feature_bank.hip - TFormer's token tensor built from a resident bank of per-frame S-Former features: feat fp32 [F, D] (rows ldf
// floats apart), black [D] (the feature row of a black frame), video_db_nr int32 [F], present uint8 [F] (or null) and index
// int64 [B] -> out fp32 [B, n_lead + T, D] = cat(lead, rows of the clip) + pos, by the data loader's clip rule
// (dataloader/aff2compdataset.py:122-156; clip_source.hpp restates it and ClipBankSource::frame applies it - here a "frame" is a
// feature row of ldf * 4 bytes).  The frozen S-Former runs in eval mode, so a frame's features do not depend on the clip it sits
// in (vformer.py:232-268 flattens [b, t] into the batch); neighbouring samples share T - 1 of their T frames, which the bank
// holds once.
//
// avf_feature_clip_tokens   one launch.  A workgroup owns one output row (b, j): its source row - lead[j], feat[a] or black - is
//                           found with the two dependent index loads of clip_bank.hip (index[b], then video_db_nr / present of
//                           the two frames), all uniform over the workgroup; a derived frame index is range-checked before any of
//                           them.  Each lane then moves 16 bytes per step, consecutive lanes on consecutive addresses: one load of
//                           the source, one of pos, one fp32 add per element, one store.  Plain stores, as the token kernels of
//                           heads.hip (DESIGN.md section 10 item 9 measured write-through as no gain for them).
//
// gfx950 resources: see DESIGN.md section 9.
#include "clip_source.hpp"

namespace avf {
namespace {

constexpr int FEAT_THREADS = 128;   // one 16-byte access per lane covers a row of D = 512

__global__ __launch_bounds__(FEAT_THREADS) void feature_clip_tokens_kernel(const ClipBankSource src, int64_t row_bytes,
                                                                           const float* __restrict__ black,
                                                                           const float* __restrict__ lead, int n_lead,
                                                                           const float* __restrict__ pos, float* __restrict__ out,
                                                                           int64_t T, int D) {
  const int64_t rows = T + n_lead;
  const int64_t r = blockIdx.x;              // (b, j): the host keeps B * rows below 2^31
  const int64_t b = r / rows, j = r - b * rows;
  const float* from;
  if (j < n_lead) {
    from = lead + j * D;
  } else {
    const uint8_t* fr = src.frame(b, j - n_lead, T, row_bytes);   // uniform over the workgroup; nullptr: a black slot
    from = fr != nullptr ? reinterpret_cast<const float*>(fr) : black;
  }
  const float* p = pos != nullptr ? pos + j * D : nullptr;
  float* o = out + r * D;
  for (int c = 4 * threadIdx.x; c < D; c += 4 * FEAT_THREADS) {
    float4 v = *reinterpret_cast<const float4*>(from + c);
    if (p != nullptr) {
      const float4 q = *reinterpret_cast<const float4*>(p + c);
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    *reinterpret_cast<float4*>(o + c) = v;
  }
}

}  // namespace
}  // namespace avf

extern "C" int avf_feature_clip_tokens(const float* feat, int64_t ldf, const float* black, const int32_t* video_db_nr,
                                       const uint8_t* present, const int64_t* index, int64_t F, int64_t B, int64_t T, int64_t d, int D,
                                       const float* lead, int n_lead, const float* pos, float* out, void* stream) {
  using namespace avf;
  const char* who = "feature_clip_tokens";
  AVF_REQUIRE(feat, "%s: feat is null", who);
  AVF_REQUIRE(black, "%s: black is null", who);
  AVF_REQUIRE(video_db_nr, "%s: video_db_nr is null", who);
  AVF_REQUIRE(index, "%s: index is null", who);
  AVF_REQUIRE(out, "%s: out is null", who);
  AVF_REQUIRE(n_lead >= 0, "%s: n_lead is %d, below 0", who, n_lead);
  AVF_REQUIRE(lead || n_lead == 0, "%s: lead is null with n_lead = %d", who, n_lead);
  AVF_REQUIRE(D >= 4 && D % 4 == 0, "%s: D is %d, not a positive multiple of 4", who, D);
  AVF_REQUIRE(ldf >= D, "%s: ldf is %lld, below D = %d", who, (long long)ldf, D);
  AVF_REQUIRE(ldf % 4 == 0, "%s: ldf is %lld, not a multiple of 4", who, (long long)ldf);
  AVF_REQUIRE(F >= 1, "%s: F is %lld, below 1", who, (long long)F);
  AVF_REQUIRE(B >= 1, "%s: B is %lld, below 1", who, (long long)B);
  AVF_REQUIRE(T >= 1, "%s: T is %lld, below 1", who, (long long)T);
  AVF_REQUIRE(d >= 1, "%s: d is %lld, below 1", who, (long long)d);
  const int64_t lim = 1LL << 31;
  AVF_REQUIRE(T < lim, "%s: T is too large", who);
  AVF_REQUIRE(d < lim, "%s: d is too large", who);                            // with T < 2^31: d * T < 2^62
  AVF_REQUIRE(ldf < lim && F <= (INT64_MAX / 16) / ldf, "%s: F * ldf is too large", who);
  const int64_t rows = T + n_lead;
  AVF_REQUIRE(B < lim && B * rows < lim, "%s: B * (n_lead + T) gives too many rows", who);
  AVF_REQUIRE(((uintptr_t)feat & 15u) == 0, "%s: feat is not 16-byte aligned", who);
  AVF_REQUIRE(((uintptr_t)black & 15u) == 0, "%s: black is not 16-byte aligned", who);
  AVF_REQUIRE(((uintptr_t)lead & 15u) == 0, "%s: lead is not 16-byte aligned", who);
  AVF_REQUIRE(((uintptr_t)pos & 15u) == 0, "%s: pos is not 16-byte aligned", who);
  AVF_REQUIRE(((uintptr_t)out & 15u) == 0, "%s: out is not 16-byte aligned", who);
  AVF_REQUIRE(((uintptr_t)video_db_nr & 3u) == 0, "%s: video_db_nr is not aligned to its element", who);
  AVF_REQUIRE(((uintptr_t)index & 7u) == 0, "%s: index is not aligned to its element", who);
  const int64_t row_bytes = ldf * 4, feat_bytes = ((F - 1) * ldf + D) * 4, out_bytes = B * rows * D * 4;
  const uintptr_t f0 = (uintptr_t)feat, o0 = (uintptr_t)out;
  AVF_REQUIRE(o0 + (uintptr_t)out_bytes <= f0 || f0 + (uintptr_t)feat_bytes <= o0, "%s: out overlaps feat", who);
  const ClipBankSource from{reinterpret_cast<const uint8_t*>(feat), video_db_nr, present, index, F, d, feat_bytes};
  feature_clip_tokens_kernel<<<(unsigned)(B * rows), FEAT_THREADS, 0, (hipStream_t)stream>>>(from, row_bytes, black, lead, n_lead, pos,
                                                                                            out, T, D);
  return check_launch("feature_clip_tokens_kernel");
}
