// mfma_frag.hpp - the device primitives every MFMA kernel here is built from, one copy each, with the hardware rule behind
// each written once: operand fragments (from LDS, transposed or by rows, and from global memory), the accumulator-to-operand
// pack, LDS-DMA, counted waits, reductions and the 4 x 4 transpose over the four lane groups, the per-XCD block order.
// Everything is __forceinline__.  What belongs to one kernel's private LDS image (swizzles, per-lane offset tables, schedules)
// stays in that kernel.
//
// Lane names: li = lane & 15, lg = lane >> 4 - the four LANE GROUPS of a 16x16 MFMA are the lanes li, li + 16, li + 32, li + 48.
#pragma once
#include "common.hpp"

namespace avf {

typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;  // MFMA 32x32 accumulator
typedef __attribute__((address_space(1))) const void gptr_t;  // the LDS-DMA builtin's global source ...
typedef __attribute__((address_space(3))) void lptr_t;        // ... and LDS destination

// Phase stamps of the attention kernels for tools/diag/attn_phases.hip and attn_m4_phases.hip (those files define the three
// macros and then include the kernel file); nothing in the product.
#ifndef AVF_PHASE_MARK
#define AVF_PHASE_INIT()
#define AVF_PHASE_MARK(slot)
#define AVF_PHASE_FLUSH()
#endif

// ---------------------------------------------------------------------------------------------
// transposed fragment (ds_read_b64_tr_b16): the A / B operand of v_mfma_f32_16x16x32_bf16 whose 32 reduction values run DOWN
// the rows of a row-major LDS image.  One read takes 4 rows x 16 columns per lane group: lane li of the group supplies the
// address of row (li >> 2), columns 4 (li & 3) .. + 3 and receives the four rows' values of column li.  Two reads, 16 rows
// apart, make the 32-row k-step, so the k-slot map of the fragment - and of a packed accumulator pair (pack_pair), which is
// why one MFMA's result can be the next one's operand - is
//   slot j of lane group g  <->  row 16*(j>>2) + 4*g + (j&3).
// api.hip's selftest_tr16_kernel checks this map on the hardware through tr_frag<32>.
// ---------------------------------------------------------------------------------------------
// p0, p1: this lane's addresses in the two 4-row blocks of the k-step
__device__ __forceinline__ bf16x8_t tr_frag_at(const lds_char* p0, const lds_char* p1) {
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p0);
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p1);
  s16x8_t r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);
}
// (generic pointers that the kernel knows to be LDS: the address-space cast happens here, per read)
__device__ __forceinline__ bf16x8_t tr_frag_at(const char* p0, const char* p1) {
  return tr_frag_at((const lds_char*)p0, (const lds_char*)p1);
}
// the second block lies 16 rows of LD bytes below the first
template <int LD>
__device__ __forceinline__ bf16x8_t tr_frag(const lds_char* p0) {
  return tr_frag_at(p0, p0 + 16 * LD);
}
// plain row-major image, row stride LD bytes: reduction rows row_base .. + 31, columns col_base .. + 15
template <int LD>
__device__ __forceinline__ bf16x8_t tr_frag(const lds_char* tile, int row_base, int col_base, int li, int lg) {
  return tr_frag<LD>(tile + (row_base + 4 * lg + (li >> 2)) * LD + (col_base + 4 * (li & 3)) * 2);
}
// chunk-XOR image of the grouped TN kernels (rows of ROWB bytes, a multiple of 256; 16-byte chunk c of row r sits at slot
// c ^ ((r & 7) << 1)); row & 7 is the same for the +16 read
template <int ROWB>
__device__ __forceinline__ bf16x8_t tr_frag_swz(const lds_char* tile, int row_base, int col_base, int li, int lg) {
  const int row = row_base + 4 * lg + (li >> 2);
  const int chunk = (col_base >> 3) + ((li & 3) >> 1);
  const int off = ((chunk ^ ((row & 7) << 1)) << 4) + ((li & 1) << 3);
  return tr_frag<ROWB>(tile + row * ROWB + off);
}

// row fragment: 8 consecutive bf16 of one row (ds_read_b128)
__device__ __forceinline__ bf16x8_t row_frag(const char* p) { return *reinterpret_cast<const bf16x8_t*>(p); }
template <int LD>
__device__ __forceinline__ bf16x8_t row_frag(const char* tile, int row, int col) {
  return row_frag(tile + row * LD + col * 2);
}

// fragment straight from global memory (16 bytes); with a predicate, zeros where it is false
__device__ __forceinline__ bf16x8_t ldg_frag(const bf16* p) {
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(p));
}
__device__ __forceinline__ bf16x8_t ldg_frag(const bf16* p, bool ok) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (ok) v = *reinterpret_cast<const uint4*>(p);
  return __builtin_bit_cast(bf16x8_t, v);
}

// two 16x16 accumulators (reduction rows 0 .. 15 and 16 .. 31 of the next product) rounded to bf16 (nearest even) as ONE
// operand fragment in the k-slot map above
__device__ __forceinline__ bf16x8_t pack_pair(const f32x4_t& a, const f32x4_t& b) {
  u32x4_t r = {pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3])};
  return __builtin_bit_cast(bf16x8_t, r);
}

// ---------------------------------------------------------------------------------------------
// Waits and LDS accesses as inline asm.  hipcc (ROCm 7.2) takes an LDS-DMA in flight for an LDS store that may alias any
// later LDS read: its wait-count pass drains vmcnt to 0 in front of the first compiler-visible ds_read that follows a
// compiler-visible DMA, which cuts a DMA ring to depth one whatever the counted waits in the source say (DESIGN_HISTORY.md
// section 12(a)).  Either side can be hidden from that pass: the reads below (the tiled NT and the big grouped TN GEMM, on
// the builtin DMA), the DMA (glds16_asm: the attention kernels, on ordinary reads), or both (the weight-stationary GEMM).
// Ordering is then the kernel's own business: a counted wait_vmcnt<N>() + s_barrier between a tile's arrival and its reads
// - vmcnt retires in order, so the compiler's own counted waits for its global loads only become more conservative - and,
// after asm reads, wait_lgkmcnt<N>() followed by sched_barrier(0) before the first use of the destination registers (the
// hardware does not interlock LDS returns, and the compiler may otherwise hoist register-only MFMAs above the wait).
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_lgkmcnt() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
// addr: LDS byte address; OFF: the instruction's immediate offset
template <typename V, int OFF>
__device__ __forceinline__ V lds_read_b128(uint32_t addr) {
  V v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ uint32_t lds_read_b32(uint32_t addr) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ s16x4_t lds_tr16_asm(uint32_t addr) {
  s16x4_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF_LO, int OFF_HI>  // tr_frag_at with the two blocks at immediate offsets of one address
__device__ __forceinline__ bf16x8_t tr_frag_asm(uint32_t addr) {
  const s16x4_t lo = lds_tr16_asm<OFF_LO>(addr), hi = lds_tr16_asm<OFF_HI>(addr);
  const s16x8_t r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA (global_load_lds): every lane gives a global address, the wave's BYTES x 64 bytes land lane-linear at ONE LDS
// address, so an image's layout is made by permuting the SOURCE.  No staging registers; counted in vmcnt.
// ---------------------------------------------------------------------------------------------
template <int BYTES>  // per lane: 16 or 4 (the builtin checks its size argument before templates are instantiated: literals)
__device__ __forceinline__ void glds(const void* g, char* l) {
  static_assert(BYTES == 16 || BYTES == 4, "LDS-DMA sizes in use");
  if constexpr (BYTES == 16) __builtin_amdgcn_global_load_lds((gptr_t*)g, (lptr_t*)l, 16, 0, 0);
  else __builtin_amdgcn_global_load_lds((gptr_t*)g, (lptr_t*)l, 4, 0, 0);
}
// The 16-byte DMA as asm, opaque to the wait-count pass (above).  The instruction takes its LDS address from m0; m0 is a
// register the compiler reserves for itself, so it is saved and restored and whatever the compiler keeps in it survives.
// lds_addr: LDS byte address, wave-uniform (an SGPR).
__device__ __forceinline__ void glds16_asm(const void* g, uint32_t lds_addr) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "s"(lds_addr), "v"(g)
               : "memory");
}
__device__ __forceinline__ void glds16_asm(const void* g, char* l) {  // l: the same for every lane, not yet known uniform
  glds16_asm(g, (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_char*)l));
}

// ---------------------------------------------------------------------------------------------
// over the four lane groups: the lanes li, li + 16, li + 32, li + 48 (one column of a 16x16 accumulator) end with the same value
// ---------------------------------------------------------------------------------------------
// by __shfl_xor (ds_bpermute round trips), fmaxf semantics
__device__ __forceinline__ float groups_max_shfl(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float groups_sum_shfl(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
// by v_permlane32_swap / v_permlane16_swap: VALU only, no LDS traffic
__device__ __forceinline__ float vmax(float a, float b) {  // v_max_f32 without the NaN-canonicalising pre-ops of fmaxf
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float groups_max_swap(float v) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = vmax(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return vmax(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float groups_sum_swap(float v) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// 4 x 4 transpose of one dword between the register index and the lane group:
// in: a[d] of lane group g = X[d][g]; out: a[k] of lane group g = X[g][k]
__device__ __forceinline__ void tr4x4(uint32_t (&a)[4]) {
  // lane groups g <-> g ^ 1: even groups keep X[d0][g] and take X[d0][g + 1], odd groups take X[d1][g - 1] and keep X[d1][g]
  const auto p01 = __builtin_amdgcn_permlane16_swap(a[0], a[1], false, false);
  const auto p23 = __builtin_amdgcn_permlane16_swap(a[2], a[3], false, false);
  // lane groups g <-> g ^ 2 on the first / second words of the two pairs
  const auto x = __builtin_amdgcn_permlane32_swap(p01[0], p23[0], false, false);
  const auto y = __builtin_amdgcn_permlane32_swap(p01[1], p23[1], false, false);
  a[0] = x[0]; a[1] = y[0]; a[2] = x[1]; a[3] = y[1];
}

// Hardware deals consecutive block ids of a 1-D grid round-robin over the 8 XCDs; this bijection of 0 .. nwg - 1 hands each
// XCD a CONTIGUOUS range of logical ids, so neighbouring logical blocks - which share operands - hit in one XCD's L2.
__device__ __forceinline__ int xcd_remap(int id, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = id & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (id >> 3);
}

}  // namespace avf
