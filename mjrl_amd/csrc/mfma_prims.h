// mfma_prims.h -- the MFMA primitives every kernel family of the library is written with (gfx950): the vector types, the fp32 MFMA
// builtin and its inline-assembly forms with AGPR accumulators, pinned LDS addresses, the wave-level hand-off, fast tanh / division,
// lane-half and DPP row sums, packed fp32 element-wise helpers on 16-register tiles, a compile-time loop and the accumulator's
// register -> unit map.  Includes nothing of the project.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mjx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define MJX_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
// Accumulators that live across ALL tiles of a wave (the weight gradients of the cached Fisher-vector product) stay in the
// accumulation registers: with -amdgpu-mfma-vgpr-form the builtins put every MFMA result in an architectural VGPR and hipcc then
// shuttles the persistent ones to AGPRs and back around each use (120 v_accvgpr moves per tile, 6 cycles each: probe_fill.hip).
// Written as inline assembly with an "a" constraint they are AGPR operands of the instruction itself.  The compiler does not see an
// MFMA in them, so it inserts none of the wait states MFMA hazards need: (i) their results are only read after the tile loop;
// (ii) `volatile` keeps them in program order, which walks the accumulators round-robin -- measured (r03): with the statements
// free to move, hipcc grouped the 4x4x1 ones by accumulator, back to back with one s_nop, and the sums came out wrong (a
// dependent 4x4x1 needs more wait states than that; the builtin form gets them from the hazard recogniser).  Used only where
// >= 4 accumulators alternate (gW2, the 4x4x1 form of gW1) or the chain is made of 64-cycle 32x32x2 instructions.
#define MJX_MFMA_ACC(acc, a, b) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b))
#define MJX_MFMA4_ACC(acc, a, b) asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b))
// The bf16 counterpart (R9 of the bf16x3 cached Fisher-vector product; a, b: four registers of 8 bf16 each).  Its operands are
// pieces a vector-ALU instruction has just written, and a VGPR written by the VALU needs 2 wait states before an MFMA reads it as
// SrcA / SrcB; the hazard recogniser pads nothing around inline assembly, so the two states open the statement itself (they
// pass in the shadow of the MFMA in front: the matrix pipe is busy for 32 cycles per instruction).
#define MJX_MFMA_BF16_ACC(acc, a, b) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b))
// 4- and 8-byte LDS accesses of the cached Fisher-vector product.  (Measured, r03: making them volatile LDS-space accesses keeps
// hipcc from pairing them into ds_read2 / ds_write2 -- whose 8-bit offset fields cost a vector add per pair to re-base the
// address, 48 per tile -- and saves 2.5 % of the kernel's cycles, but the chip gives the same 2.5 % back in clock: no
// change in time, and hipcc 7.2 crashes on the volatile form in one instance.  Plain accesses it is.)
typedef __attribute__((address_space(3))) float lds_float;
// LDS byte address of a shared-memory pointer as an opaque 32-bit value: the compiler must keep it in a register (it would
// otherwise re-derive `base + constant` with a v_add_u32 next to every ds_write2 / ds_read2 whose 8-bit offsets do not reach --
// ~25 single vector-ALU instructions inside the MFMA phases of a cached Fisher-vector-product tile, 12 cycles each there)
__device__ __forceinline__ uint32_t lds_pin(const float* p) {
  uint32_t a = (uint32_t)(uintptr_t)(const lds_float*)p;
  asm volatile("" : "+v"(a));
  return a;
}
#define LDS_AT(addr) ((lds_float*)(uintptr_t)(addr))
#define LDS_ST(p, v) (*(p) = (v))
#define LDS_LD(p) (*(p))
#define LDS_LD2(p) (*(const f32x2*)(p))

__device__ __forceinline__ void wave_sync() {
  // LDS traffic between lanes of ONE wave: hardware executes a wave's DS ops in order,
  // this only stops the compiler from moving them across the hand-off.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tanh(x) = 1 - 2 / (1 + exp2(2 log2(e) x)): branch-free, v_exp_f32 + v_rcp_f32 + one FMA; no |x|, no sign transfer, no
// Newton step (exp2 -> inf gives rcp -> 0 -> +1, exp2 -> 0 gives -1; a Newton step would form inf * 0 there).  Max abs error
// ~1.2e-7 (1 ulp of the reciprocal doubled + the exponential's ulp; ocml tanhf: 6e-8, branchy).  fp32 MFMAs do not hide
// vector-ALU work (DESIGN "what an fp32 MFMA hides"), so every instruction here is paid in full: r02's form -- sign(x)(1 - t)/(1 + t),
// t = exp2(-2 log2(e)|x|), Newton-refined -- cost 6 packed + 4 quarter-rate + 2 v_bfi per register pair, this one 3 + 4
// (K1 0.379 -> 0.361 ms, K3 0.177 -> 0.155 ms; step direction vs the reference at 1M: 2.90e-6 -> 2.95e-6, bar 1e-5).
__device__ __forceinline__ float fast_tanh(float x) {
  const float d = 1.0f + __builtin_amdgcn_exp2f(x * 2.885390081777927f);
  return fmaf(__builtin_amdgcn_rcpf(d), -2.0f, 1.0f);
}

// the same on a 16-register tile, two registers per packed instruction (scale, 1 + e, the final FMA; v_exp_f32 / v_rcp_f32
// stay per register)
__device__ __forceinline__ void fast_tanh16(f32x16& o, const f32x16& x) {
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const f32x2 s = f32x2{x[r], x[r + 1]} * (f32x2)(2.885390081777927f);
    const f32x2 d = f32x2{__builtin_amdgcn_exp2f(s.x), __builtin_amdgcn_exp2f(s.y)} + (f32x2)(1.0f);
    const f32x2 rr = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    const f32x2 y = __builtin_elementwise_fma(rr, (f32x2)(-2.0f), (f32x2)(1.0f));
    o[r] = y.x; o[r + 1] = y.y;
  }
}

// a / b with v_rcp_f32 + one Newton step (<= 2 ulp; exact for b == 1): the per-sample divisions of the likelihood
// head and of the input normalisation cost 4 VALU ops instead of the ~12 of the IEEE sequence
__device__ __forceinline__ float fast_div(float a, float b) {
  float r = __builtin_amdgcn_rcpf(b);
  r = r * fmaf(-b, r, 2.0f);
  return a * r;
}

// mask ? a : b on bit patterns (mask = all ones / all zeros per lane)
__device__ __forceinline__ float half_select(uint32_t mask, float a, float b) {
  return __uint_as_float((__float_as_uint(a) & mask) | (__float_as_uint(b) & ~mask));
}

// x[lane] + x[lane ^ 32] in every lane: v_permlane32_swap exchanges the upper half of one copy with the
// lower half of the other (one VALU op, no LDS round trip like ds_bpermute)
__device__ __forceinline__ float half_sum(float p) {
  auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(p), __float_as_uint(p), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}

// every lane: the sum over its 16-lane row, by DPP moves (vector-ALU latency; the same operand pairs, hence the same bits, as
// `v += __shfl_xor(v, 1); ... 2; ... 4; ... 8` -- after each step all lanes of a group hold the group's sum -- without the four
// ~100-cycle trips through the LDS pipe that ds_bpermute costs)
__device__ __forceinline__ float row16_sum(float v) {
  auto dpp = [](float x, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xF, 0xF, true));
  };
  v += dpp(v, std::integral_constant<int, 0xB1>{});       // quad_perm [1,0,3,2]
  v += dpp(v, std::integral_constant<int, 0x4E>{});       // quad_perm [2,3,0,1]
  v += dpp(v, std::integral_constant<int, 0x141>{});      // row_half_mirror
  v += dpp(v, std::integral_constant<int, 0x140>{});      // row_mirror
  return v;
}

// packed fp32 element-wise helpers on 16-register tiles (register pairs -> v_pk_fma_f32 / v_pk_mul_f32)
__device__ __forceinline__ f32x16 pk_1mh2(const f32x16& h) {                      // 1 - h^2
  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const f32x2 hh = {h[r], h[r + 1]};
    const f32x2 ff = __builtin_elementwise_fma(-hh, hh, (f32x2)(1.0f));
    o[r] = ff.x; o[r + 1] = ff.y;
  }
  return o;
}
__device__ __forceinline__ void pk_mul(f32x16& t, const f32x16& f) {              // t *= f
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    f32x2 tt = {t[r], t[r + 1]};
    tt *= f32x2{f[r], f[r + 1]};
    t[r] = tt.x; t[r + 1] = tt.y;
  }
}
__device__ __forceinline__ void pk_mul_1mh2(f32x16& t, const f32x16& h) {         // t *= 1 - h^2
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const f32x2 hh = {h[r], h[r + 1]};
    f32x2 tt = {t[r], t[r + 1]};
    tt *= __builtin_elementwise_fma(-hh, hh, (f32x2)(1.0f));
    t[r] = tt.x; t[r + 1] = tt.y;
  }
}
// The same two as ONE packed FMA per register pair with the negation in the instruction's modifiers: left to the compiler, -h
// becomes a v_xor_b32 per register (32 extra vector-ALU instructions per cached Fisher-vector-product tile) or the pair is split
// into scalar v_fma_f32 / v_mul_f32.  Inline asm is invisible to the compiler's hazard recogniser: NO wait states are inserted
// between an MFMA and an asm instruction that reads its result -- use these only on registers whose producing MFMA retired long
// ago (a whole MFMA phase in between), never directly behind the producer (the non-cached tile body does that: 2 % wrong and
// nondeterministic when it was tried there).
__device__ __forceinline__ f32x2 pk_1mh2_pair_far(f32x2 hh) {
  f32x2 ff;
  asm("v_pk_fma_f32 %0, %1, %1, 1.0 op_sel_hi:[1,1,0] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(ff) : "v"(hh));
  return ff;
}
__device__ __forceinline__ f32x16 pk_1mh2_far(const f32x16& h) {
  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const f32x2 ff = pk_1mh2_pair_far(f32x2{h[r], h[r + 1]});
    o[r] = ff.x; o[r + 1] = ff.y;
  }
  return o;
}
// a fresh MFMA result times 1 - h^2 of values that came from the vector ALU or from LDS: the factor as one packed FMA with
// modifiers (asm: its operands are not MFMA results), the product as a builtin (the compiler sees the MFMA -> VALU hazard)
__device__ __forceinline__ f32x2 mul_1mh2_pair(float a0, float a1, float h0, float h1) {
  const f32x2 ff = pk_1mh2_pair_far(f32x2{h0, h1});
  f32x2 tt = {a0, a1};
  tt *= ff;
  return tt;
}
__device__ __forceinline__ void pk_mul_1mh2_far(f32x16& t, const f32x16& h) {
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    f32x2 tt = {t[r], t[r + 1]};
    const f32x2 ff = pk_1mh2_pair_far(f32x2{h[r], h[r + 1]});
    asm("v_pk_mul_f32 %0, %0, %1" : "+v"(tt) : "v"(ff));
    t[r] = tt.x; t[r + 1] = tt.y;
  }
}

// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{})
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<N, I + 1>(f); }
}

// unit index (within a 32-block) held by accumulator register r of lane-half hi
__device__ __forceinline__ constexpr int unit_of(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

}  // namespace mjx
