// bf16x3.h -- fp32 products on v_mfma_f32_32x32x16_bf16 from three bf16 pieces per operand: the split, the six piece products, and
// the one-instruction-at-a-time forms of both for schedules that place every instruction in an MFMA gap by hand.
#pragma once
#include "mfma_prims.h"

namespace mjx {

// bf16x3 (the cached Fisher-vector product's 64x64 products on v_mfma_f32_32x32x16_bf16): x = hi + mid + lo EXACTLY, each piece a
// bf16 -- hi = x with the low 16 bits cleared, r = x - hi (exact), mid = r truncated the same way, lo = r - mid (exact; at most 8
// significant bits, so a bf16 as it stands).  The upper halves of x, r, lo ARE the three bf16 pieces: two values per register by
// one v_perm_b32.  Only single-issue 4-cycle instructions (no packed fp32: beside MFMAs each costs +22-26 cycles).  Of the 9 piece
// products the 6 with i + j <= 2 are formed (tools/probe_split_error.py: FVP / CG-10 at native-fp32 distance from fp64).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define MJX_MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (a)), __builtin_bit_cast(bf16x8, (b)), (c), 0, 0, 0)
struct Pc3 { u32x4 p[3]; };                      // hi, mid, lo: 8 bf16 each (one operand of v_mfma_f32_32x32x16_bf16)
// values 2 k, 2 k + 1 of an operand -> register k of its three pieces (11 vector-ALU instructions)
__device__ __forceinline__ void split3_pair(Pc3& o, int k, float xa, float xb) {
  const uint32_t ua = __float_as_uint(xa), ub = __float_as_uint(xb);
  const float ra = xa - __uint_as_float(ua & 0xffff0000u), rb = xb - __uint_as_float(ub & 0xffff0000u);
  const uint32_t va = __float_as_uint(ra), vb = __float_as_uint(rb);
  const float la = ra - __uint_as_float(va & 0xffff0000u), lb = rb - __uint_as_float(vb & 0xffff0000u);
  o.p[0][k] = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
  o.p[1][k] = __builtin_amdgcn_perm(vb, va, 0x07060302u);
  o.p[2][k] = __builtin_amdgcn_perm(__float_as_uint(lb), __float_as_uint(la), 0x07060302u);
}
__device__ __forceinline__ Pc3 split3(const float (&x)[8]) {
  Pc3 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) split3_pair(o, k, x[2 * k], x[2 * k + 1]);
  return o;
}
// the pieces of registers 8 s .. 8 s + 7 of a 32x32 accumulator (K-step s of the next layer's operand)
__device__ __forceinline__ Pc3 split3_of(const f32x16& v, int s) {
  float x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = v[8 * s + i];
  return split3(x);
}
// acc += a * b over the six piece products, the small ones first
__device__ __forceinline__ f32x16 mfma_bf3(const Pc3& a, const Pc3& b, f32x16 c) {
  c = MJX_MFMA_BF16(a.p[2], b.p[0], c);
  c = MJX_MFMA_BF16(a.p[0], b.p[2], c);
  c = MJX_MFMA_BF16(a.p[1], b.p[1], c);
  c = MJX_MFMA_BF16(a.p[1], b.p[0], c);
  c = MJX_MFMA_BF16(a.p[0], b.p[1], c);
  c = MJX_MFMA_BF16(a.p[0], b.p[0], c);
  return c;
}
// ... and one of the six at a time (p = 0 .. 5 in mfma_bf3's order), for schedules that place every MFMA by hand
__device__ __forceinline__ f32x16 mfma_bf3_step(const Pc3& a, const Pc3& b, f32x16 c, int p) {
  const int pa = p == 0 ? 2 : (p == 2 || p == 3) ? 1 : 0, pb = p == 1 ? 2 : (p == 2 || p == 4) ? 1 : 0;
  return MJX_MFMA_BF16(a.p[pa], b.p[pb], c);
}
// split3() one instruction at a time: step idx = 0 .. 43 of the 44 that split eight values, the same operations on the same
// values as split3_pair.  Two register pairs (four values) advance together, so that four consecutive steps never depend on
// each other -- what one MFMA gap carries: 4 ands (hi masks), 4 subtractions (r), 2 perms (hi pieces), 4 ands, 4 subtractions
// (lo), 2 + 2 perms (mid, lo pieces); then the other two pairs.  w holds the intermediate values between the steps.
// The steps are plain arithmetic, which the compiler places wherever the data flow allows -- scheduling barriers alone left the
// 44 steps of a group in lumps of 0 .. 10 per gap.  So every step is tied to its gap from both sides: its constant (the mask, the
// perm selector) comes from the gap's opening statement (SplitGap::open: an empty volatile asm that passes the two constants on
// in their scalar registers and, as a memory barrier, keeps the gap's LDS accesses behind it), and its result passes through an
// empty volatile asm of its own before anything uses it.  No instruction comes of either: one wave per SIMD issues in order, and
// even a scalar move per gap would take an issue slot of the 8 a 32-cycle MFMA gap has.
// The 44 steps over the 12 gaps of a K-step group: 3 in each of the first four, 4 in the other eight.  (The first gaps of a
// phase are where the register allocator parks one or two values in AGPRs in the instances with the most registers; with
// three steps they stay within the five vector instructions a gap hides.)  Steps of one gap never depend on each other.
__device__ __forceinline__ constexpr int split3_first(int gap) { return gap < 4 ? 3 * gap : 4 * gap - 4; }
struct Split3Tmp { uint32_t h[8], m[8]; float r[8], l[8]; };
struct SplitGap {
  uint32_t mask = 0xffff0000u, sel = 0x07060302u;
  __device__ __forceinline__ void open() { asm volatile("" : "+s"(mask), "+s"(sel) : : "memory"); }
};
// (an MFMA builtin is as free to move as the arithmetic: its result takes the same way)
__device__ __forceinline__ void mfma_pin(f32x16& c) { asm volatile("" : "+v"(c)); }
__device__ __forceinline__ uint32_t split3_pin(uint32_t v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ float split3_pin(float v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ void split3_step(Pc3& o, Split3Tmp& w, const float (&x)[8], int idx, const SplitGap& c) {
  const int b = idx / 22, t = idx % 22;
  if (t < 4) { const int i = 4 * b + t; w.h[i] = split3_pin(__float_as_uint(x[i]) & c.mask); }
  else if (t < 8) { const int i = 4 * b + t - 4; w.r[i] = split3_pin(x[i] - __uint_as_float(w.h[i])); }
  else if (t < 10) { const int k = 2 * b + t - 8; o.p[0][k] = split3_pin(__builtin_amdgcn_perm(__float_as_uint(x[2 * k + 1]), __float_as_uint(x[2 * k]), c.sel)); }
  else if (t < 14) { const int i = 4 * b + t - 10; w.m[i] = split3_pin(__float_as_uint(w.r[i]) & c.mask); }
  else if (t < 18) { const int i = 4 * b + t - 14; w.l[i] = split3_pin(w.r[i] - __uint_as_float(w.m[i])); }
  else if (t < 20) { const int k = 2 * b + t - 18; o.p[1][k] = split3_pin(__builtin_amdgcn_perm(__float_as_uint(w.r[2 * k + 1]), __float_as_uint(w.r[2 * k]), c.sel)); }
  else { const int k = 2 * b + t - 20; o.p[2][k] = split3_pin(__builtin_amdgcn_perm(__float_as_uint(w.l[2 * k + 1]), __float_as_uint(w.l[2 * k]), c.sel)); }
}

}  // namespace mjx
