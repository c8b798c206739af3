// lw_gemm.h -- the general GEMM kernel of the layer-wise path, k_gemm<BM, BN, NTH>: any operand layout, any edge, ten fused
// epilogues.  What a product is (GemmArgs, EPI_*) and the tile geometry are declared in lw_plan.h, which also decides which
// instance a product goes to; lw_launch.h launches it.  The persistent kernel for the steady-state products is lw_gemm_p.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "mfma_prims.h"
#include "lw_plan.h"

namespace mjx {

#ifdef MJX_PHASE_CLOCK
// timing build (-DMJX_PHASE_CLOCK): every workgroup of a k_gemm launch leaves its entry / first-MFMA / loop-end / exit
// times (s_memrealtime, 100 MHz) and the CU it ran on, in the slot the launcher gave it (lw_launch.h)
#define LW_STAMP(k) do { if (g.clk && tid == 0 && blockIdx.z == 0) { __builtin_amdgcn_sched_barrier(0); \
  g.clk[8 + 8 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) + (k)] = (long long)__builtin_amdgcn_s_memrealtime(); \
  if ((k) == 1 || (k) == 2) g.clk[8 + 8 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) + 5 + (k)] = (long long)__builtin_readcyclecounter(); \
  __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define LW_STAMP(k) do {} while (0)
#endif

// C = sum_p A_p * B_p with v_mfma_f32_32x32x2_f32; 4 waves in a 2x2 grid of 64x64 sub-tiles, K tiles of 32.
// Operand tiles go global -> registers -> LDS in the 16-byte granules they are contiguous in:
//   * a K-contiguous operand (activations, W as "NT") is kept as [row][k] (row stride 36) and its MFMA fragments
//     are read with ONE ds_read_b128 per 32-row block and 4 k-steps;
//   * a row-contiguous operand (W as "NN", the sample-major operands of the weight gradient) is kept as [k][row]
//     (stride 132) and read with ds_read_b32;
//   k-slot `hi` of step (q, t) carries k = 8q + 4hi + t for A and B alike (the permutation trick of the fused kernels).
// Operand tiles are double-buffered in LDS (one barrier per k-tile); tile k + 1 is stored and tile k + 2 requested from
// global memory (register-staged) before the MFMAs of tile k.  blockIdx.z splits the K range of pair 0 (wgrad: K = samples).
// BN = 128: 2x2 waves of 64x64; BN = 32 (narrow outputs: action heads, value heads): 4x1 waves of 32x32, so a
// 17-column product is padded to 32 instead of 128 columns.
// threads per workgroup: 8 waves at BN >= 128 (one workgroup per CU, two waves per SIMD), 4 waves of 32 x 32 at BN = 32.
// Tile shapes (BM x BN, per-wave sub-tile, accumulator registers):
//   128 x 128   32 x 64    32     the round-1 shape: every operand is re-read once per 128 output columns / rows
//   128 x 256   64 x 64    64     sample-major products with >= 256 output columns (hidden layers of 256 / 512 units):
//                                 the activation operand is read ONCE per 256 columns -- these GEMMs sit at the ridge of
//                                 the roofline when their operands stream from HBM, so halving the re-reads
//                                 is worth more than occupancy
//   128 x 128   64 x 64    64     in 256-thread workgroups (4 waves), two workgroups per CU: one workgroup's epilogue
//                                 (activation loads, stores) and pipeline fill run under the other's matrix-core loop
template <int BN> constexpr int gemm_threads() { return BN >= 128 ? 512 : 256; }

template <int BM, int BN, int NTH = gemm_threads<BN>()>
__global__ __launch_bounds__(NTH, 2) void k_gemm(GemmArgs g) {      // (second argument: waves per SIMD; 4 would need <= 128 VGPRs: spills, measured slower)
  constexpr int WN = BN / 64 > 0 ? BN / 64 : 1;   // waves along N
  constexpr int WMc = (NTH / 64) / WN;            // waves along M
  constexpr int TM = BM / WMc, TN = BN / WN;     // per-wave tile
  constexpr int MT = TM / 32, NT = TN / 32;
  // two buffers per operand (dynamic LDS: 72 KB at 128 x 128, 108 KB at 128 x 256, 144 KB at 256 x 256): tile k + 1 is
  // stored while tile k is being multiplied, ONE barrier per k-tile
  constexpr int ASZ = (BM * GLD > GBK * (BM + 4)) ? BM * GLD : GBK * (BM + 4), BSZ = (BN * GLD > GBK * (BN + 4)) ? BN * GLD : GBK * (BN + 4);
  extern __shared__ __attribute__((aligned(16))) float gsm[];
  float* As = gsm;                       // [2][ASZ]
  float* Bs = gsm + 2 * ASZ;             // [2][BSZ]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  LW_STAMP(0);
#ifdef MJX_PHASE_CLOCK
  if (g.clk && tid == 0 && blockIdx.z == 0) {
    long long* q = g.clk + 8 + 8 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
    q[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_ID
    q[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // XCC_ID
    if (blockIdx.x == 0 && blockIdx.y == 0) {
      g.clk[0] = g.M; g.clk[1] = g.N; g.clk[2] = g.K[0]; g.clk[3] = g.npairs > 1 ? g.K[1] : 0; g.clk[4] = g.epi; g.clk[5] = BN;
      g.clk[6] = gridDim.x * gridDim.y; g.clk[7] = gridDim.z;
    }
  }
#endif
  f32x16 acc[MT][NT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = (f32x16)(0.f);

  for (int p = 0; p < g.npairs; ++p) {
    int kbeg = 0, kend = g.K[p];
    if (gridDim.z > 1) {
      int chunk = (g.K[p] + gridDim.z - 1) / gridDim.z;
      chunk = ((chunk + GBK - 1) / GBK) * GBK;
      kbeg = blockIdx.z * chunk;
      kend = min(g.K[p], kbeg + chunk);
    }
    if (kbeg >= kend) continue;
    // one operand tile = 128 rows x 32 k = 1024 float4; 2 (4) per thread.  mode 0: K-contiguous, mode 1: row-contiguous,
    // mode 2: anything else (scalar gather)
    auto mode_of = [](const float* ptr, int64_t rs, int64_t ks) {
      if (ks == 1 && (rs & 3) == 0 && (((uintptr_t)ptr) & 15) == 0) return 0;
      if (rs == 1 && (ks & 3) == 0 && (((uintptr_t)ptr) & 15) == 0) return 1;
      return 2;
    };
    const float* __restrict__ Ap = g.A[p];
    const float* __restrict__ Bp = g.B[p];
    const int64_t ars = g.a_rs[p], aks = g.a_ks[p], bcs = g.b_cs[p], bks = g.b_ks[p];
    const int amode = mode_of(Ap, ars, aks), bmode = mode_of(Bp, bcs, bks);
    constexpr int CA = BM * 8 / NTH, CB = BN * 8 / NTH;        // float4 per thread and operand tile
    f32x4 ra[CA], rb[CB];
    // RT = rows of the tile (128 or 32): 8 float4 per row in the [row][k] image, RT/4 per k-row in the [k][row] image
    auto gload1 = [&](auto rt, auto& r, const float* __restrict__ P, int mode, int64_t rs, int64_t ks, int r0, int R, int k0) {
      constexpr int RT = decltype(rt)::value, NC = RT * 8 / NTH, Q = RT / 4;
      // interior tiles (block-uniform test): unconditional 16-byte loads, nothing else in the way
      if (mode != 2 && r0 + RT <= R && k0 + GBK <= kend) {
        if (mode == 0) {
#pragma unroll
          for (int c = 0; c < NC; ++c) { const int idx = tid + NTH * c; r[c] = *(const f32x4*)(P + (int64_t)(r0 + (idx >> 3)) * rs + k0 + 4 * (idx & 7)); }
        } else {
#pragma unroll
          for (int c = 0; c < NC; ++c) { const int idx = tid + NTH * c; r[c] = *(const f32x4*)(P + (int64_t)(k0 + idx / Q) * ks + r0 + 4 * (idx % Q)); }
        }
        return;
      }
      // edge tiles / unaligned operands: element-wise, clamped address + select (no branches)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int idx = tid + NTH * c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = (mode == 1) ? r0 + 4 * (idx % Q) + e : r0 + (idx >> 3);
          const int k = (mode == 1) ? k0 + idx / Q : k0 + 4 * (idx & 7) + e;
          const bool ok = (row < R) && (k < kend);
          const float v = P[ok ? (int64_t)row * rs + (int64_t)k * ks : 0];
          r[c][e] = ok ? v : 0.f;
        }
      }
    };
    // LDS image: K-contiguous operands as [row][k] (stride GLD), row-contiguous ones as [k][row] (stride RT + 4) --
    // either way the 16-byte granule that was loaded is stored with one conflict-free ds_write_b128
    auto lstore1 = [&](auto rt, float* S, const auto& r, int mode) {
      constexpr int RT = decltype(rt)::value, NC = RT * 8 / NTH, Q = RT / 4;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int idx = tid + NTH * c;
        if (mode == 1) *(f32x4*)&S[(idx / Q) * (RT + 4) + 4 * (idx % Q)] = r[c];
        else *(f32x4*)&S[(idx >> 3) * GLD + 4 * (idx & 7)] = r[c];
      }
    };
    // operand fragment of the 32-row block at row0 for the 4 k-steps of group q: k-slot `hi` of step t carries
    // k = 8q + 4hi + t (one ds_read_b128 from the [row][k] image, four ds_read_b32 from the [k][row] image)
    auto frag = [&](auto rt, const float* S, int mode, int row0, int q) {
      constexpr int RT = decltype(rt)::value;
      if (mode == 1) {
        // (volatile: four single ds_read_b32 with 16-bit byte offsets.  Paired into ds_read2_b32 -- 8-bit offsets, 1 020 bytes of reach
        //  against rows (RT + 4) * 4 = 528 / 1 040 bytes apart -- every k-group re-based with v_add_u32: 16-25 vector-ALU instructions
        //  per k-tile and wave between the MFMAs, which fp32 MFMAs do not hide; LDS instructions they do.)
        const volatile lds_float* p = (const volatile lds_float*)(const lds_float*)&S[(8 * q + 4 * hi) * (RT + 4) + row0 + j];
        return f32x4{p[0], p[RT + 4], p[2 * (RT + 4)], p[3 * (RT + 4)]};
      }
      return *(const f32x4*)&S[(row0 + j) * GLD + 8 * q + 4 * hi];
    };
    constexpr std::integral_constant<int, BM> RA{};
    constexpr std::integral_constant<int, BN> RB{};
    // The K loop is instantiated per LDS image pair (chosen once per operand pair, outside the loop), so that the body
    // is one straight-line block: fragment reads of group q + 1 and the MFMAs of group q schedule together.
    auto kloop = [&](auto ta, auto tb) {
      constexpr int LA = decltype(ta)::value, LB = decltype(tb)::value;     // 1: [k][row] image, 0: [row][k] image
      const int ntile = (kend - kbeg + GBK - 1) / GBK;
      gload1(RA, ra, Ap, amode, ars, aks, m0, g.M, kbeg);
      gload1(RB, rb, Bp, bmode, bcs, bks, n0, g.N, kbeg);
      __syncthreads();                                 // (a previous operand pair is fully consumed)
      lstore1(RA, As, ra, LA);
      lstore1(RB, Bs, rb, LB);
      if (ntile > 1) {
        gload1(RA, ra, Ap, amode, ars, aks, m0, g.M, kbeg + GBK);
        gload1(RB, rb, Bp, bmode, bcs, bks, n0, g.N, kbeg + GBK);
      }
      __syncthreads();
      if (p == 0) LW_STAMP(1);
      for (int kt = 0; kt < ntile; ++kt) {
        const float* Ac = As + (kt & 1) * ASZ;
        const float* Bc = Bs + (kt & 1) * BSZ;
        if (kt + 1 < ntile) {
          // tile kt + 1 goes into the other buffer (its last readers passed the barrier that ended iteration kt - 1), the
          // global loads of tile kt + 2 then fly under this tile's MFMAs
          lstore1(RA, As + ((kt + 1) & 1) * ASZ, ra, LA);
          lstore1(RB, Bs + ((kt + 1) & 1) * BSZ, rb, LB);
          if (kt + 2 < ntile) {
            gload1(RA, ra, Ap, amode, ars, aks, m0, g.M, kbeg + (kt + 2) * GBK);
            gload1(RB, rb, Bp, bmode, bcs, bks, n0, g.N, kbeg + (kt + 2) * GBK);
          }
        }
        f32x4 a4[MT], b4[NT], an[MT], bn[NT];
#pragma unroll
        for (int a = 0; a < MT; ++a) a4[a] = frag(RA, Ac, LA, wm * TM + 32 * a, 0);
#pragma unroll
        for (int b = 0; b < NT; ++b) b4[b] = frag(RB, Bc, LB, wn * TN + 32 * b, 0);
#pragma unroll
        for (int q = 0; q < GBK / 8; ++q) {
          if (q + 1 < GBK / 8) {
#pragma unroll
            for (int a = 0; a < MT; ++a) an[a] = frag(RA, Ac, LA, wm * TM + 32 * a, q + 1);
#pragma unroll
            for (int b = 0; b < NT; ++b) bn[b] = frag(RB, Bc, LB, wn * TN + 32 * b, q + 1);
          }
#ifdef MJX_GEMM_SETPRIO
          __builtin_amdgcn_s_setprio(1);       // (experiment) the wave that is issuing matrix-core work wins arbitration over its SIMD partner's loads / LDS traffic
#endif
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
              for (int b = 0; b < NT; ++b) acc[a][b] = MJX_MFMA(a4[a][t], b4[b][t], acc[a][b]);
#ifdef MJX_GEMM_SETPRIO
          __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
          for (int a = 0; a < MT; ++a) a4[a] = an[a];
#pragma unroll
          for (int b = 0; b < NT; ++b) b4[b] = bn[b];
        }
        __syncthreads();
      }
    };
    // Fast path of the 256-column tiles: every tile of this operand pair is interior (whole 128 x 256 block inside the
    // matrices, K range a multiple of 32, 16-byte granules) -- the steady state of the big products.  Per-thread operand
    // pointers are formed once and bumped by a constant per k-tile, and the LDS stores of tile k + 1 / the global loads of
    // tile k + 2 sit BETWEEN the MFMA groups of tile k instead of in front of them: in the general loop above all eight
    // waves leave the barrier together, do their stores / address arithmetic / load issue together (~700 cycles per
    // k-tile during which no matrix-core instruction runs on the CU) and only then start multiplying.  (Measured before
    // building this: with the activation operand served from cache -- MJX_LW_DEBUG_ALIAS_A -- the big products run 1-3 %
    // faster, so the loop is not waiting for memory; it loses its ~12 % in that phase-locked overhead.)
    auto kloop_fast = [&](auto ta, auto tb) {
      constexpr int LA = decltype(ta)::value, LB = decltype(tb)::value;
      constexpr int QA = BM / 4, QB = BN / 4;
      const int ntile = (kend - kbeg) / GBK;
      const float* pa[CA];
      const float* pb[CB];
#pragma unroll
      for (int c = 0; c < CA; ++c) {
        const int idx = tid + NTH * c;
        pa[c] = LA ? Ap + (int64_t)(kbeg + idx / QA) * aks + m0 + 4 * (idx % QA) : Ap + (int64_t)(m0 + (idx >> 3)) * ars + kbeg + 4 * (idx & 7);
      }
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const int idx = tid + NTH * c;
        pb[c] = LB ? Bp + (int64_t)(kbeg + idx / QB) * bks + n0 + 4 * (idx % QB) : Bp + (int64_t)(n0 + (idx >> 3)) * bcs + kbeg + 4 * (idx & 7);
      }
      const int64_t sa = LA ? (int64_t)GBK * aks : GBK, sb = LB ? (int64_t)GBK * bks : GBK;
      auto gloadf = [&]() {
#pragma unroll
        for (int c = 0; c < CA; ++c) { ra[c] = *(const f32x4*)pa[c]; pa[c] += sa; }
#pragma unroll
        for (int c = 0; c < CB; ++c) { rb[c] = *(const f32x4*)pb[c]; pb[c] += sb; }
      };
      gloadf();
      __syncthreads();                                 // (a previous operand pair is fully consumed)
      lstore1(RA, As, ra, LA);
      lstore1(RB, Bs, rb, LB);
      if (ntile > 1) gloadf();
      __syncthreads();
      if (p == 0) LW_STAMP(1);
      auto body = [&](int kt, auto st_tag, auto ld_tag) {
        constexpr bool ST = decltype(st_tag)::value, LD = decltype(ld_tag)::value;
        const float* Ac = As + (kt & 1) * ASZ;
        const float* Bc = Bs + (kt & 1) * BSZ;
        f32x4 a4[MT], b4[NT], an[MT], bn[NT];
#pragma unroll
        for (int a = 0; a < MT; ++a) a4[a] = frag(RA, Ac, LA, wm * TM + 32 * a, 0);
#pragma unroll
        for (int b = 0; b < NT; ++b) b4[b] = frag(RB, Bc, LB, wn * TN + 32 * b, 0);
#pragma unroll
        for (int q = 0; q < GBK / 8; ++q) {
          if (q + 1 < GBK / 8) {
#pragma unroll
            for (int a = 0; a < MT; ++a) an[a] = frag(RA, Ac, LA, wm * TM + 32 * a, q + 1);
#pragma unroll
            for (int b = 0; b < NT; ++b) bn[b] = frag(RB, Bc, LB, wn * TN + 32 * b, q + 1);
          }
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
              for (int b = 0; b < NT; ++b) acc[a][b] = MJX_MFMA(a4[a][t], b4[b][t], acc[a][b]);
          if (q == 0 && ST) {                            // tile kt + 1 -> the other buffer, under this tile's MFMAs
            lstore1(RA, As + ((kt + 1) & 1) * ASZ, ra, LA);
            lstore1(RB, Bs + ((kt + 1) & 1) * BSZ, rb, LB);
          }
          if (q == 1 && LD) gloadf();                    // tile kt + 2 -> registers
#pragma unroll
          for (int a = 0; a < MT; ++a) a4[a] = an[a];
#pragma unroll
          for (int b = 0; b < NT; ++b) b4[b] = bn[b];
        }
        __syncthreads();
      };
      using T = std::true_type;
      using F = std::false_type;
      int kt = 0;
      for (; kt + 2 < ntile; ++kt) body(kt, T{}, T{});
      if (kt + 1 < ntile) { body(kt, T{}, F{}); ++kt; }
      body(kt, F{}, F{});
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    bool fast = false;
    if (BN == 256 && g.fast && amode != 2 && bmode != 2 && m0 + BM <= g.M && n0 + BN <= g.N && ((kend - kbeg) % GBK) == 0) fast = true;
    if (fast) {
      if constexpr (BN == 256) {
        if (amode == 1) { if (bmode == 1) kloop_fast(I1{}, I1{}); else kloop_fast(I1{}, I0{}); }
        else { if (bmode == 1) kloop_fast(I0{}, I1{}); else kloop_fast(I0{}, I0{}); }
      }
    } else {
      if (amode == 1) { if (bmode == 1) kloop(I1{}, I1{}); else kloop(I1{}, I0{}); }
      else { if (bmode == 1) kloop(I0{}, I1{}); else kloop(I0{}, I0{}); }
    }
  }
  // Epilogue, specialised once per launch (not per element): per-column constants are fetched once per 32-column
  // block, the activation operands of a 32x32 block as one batch of independent loads.
  LW_STAMP(2);
  float* Cz = g.C + (int64_t)blockIdx.z * g.c_zs;
  auto epilogue = [&](auto tag) {
    constexpr int EPI = decltype(tag)::value;
    constexpr bool USE_BIAS = EPI == EPI_BIAS_TANH || EPI == EPI_BIAS_AFFINE || EPI == EPI_TANGENT || EPI == EPI_BIAS || EPI == EPI_BIAS_RELU ||
                              EPI == EPI_FVP_HEAD;
    constexpr bool USE_AUX = EPI == EPI_TANGENT || EPI == EPI_BACK || EPI == EPI_RBACK || EPI == EPI_BACK_RELU;
    constexpr bool CSUM = EPI == EPI_BACK || EPI == EPI_BACK_RELU;      // launches that may carry g.colsum
    const int64_t ccs = g.c_cs ? g.c_cs : 1;
    float csum[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) csum[nt] = 0.f;
    // Interior blocks (the whole BM x BN block inside C, unit column stride): addresses are a wave-uniform base per 32 x 32
    // block (SGPRs) + sixteen 32-bit lane offsets formed once; the element-wise path below pays a 64-bit multiply, bounds
    // tests and selects PER ELEMENT -- measured with the per-workgroup clocks (tools/lw_clock.py) at ~10 us per workgroup,
    // 13-23 % of a 256-wide product and more than half of the K <= 39 ones.  The activation operand of all the wave's blocks
    // is requested as one batch.
    if (m0 + BM <= g.M && n0 + BN <= g.N && ccs == 1 && g.ldc < (1 << 24) && g.ld_aux < (1 << 24)) {
      const int wv = __builtin_amdgcn_readfirstlane(wave);
      const int um = m0 + (wv / WN) * TM, un = n0 + (wv % WN) * TN;        // wave-uniform origin of this wave's sub-tile
      uint32_t offC[16], offA[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        offC[r] = (uint32_t)(4 * hi) * (uint32_t)g.ldc + (uint32_t)j + (uint32_t)((r & 3) + 8 * (r >> 2)) * (uint32_t)g.ldc;
        offA[r] = (uint32_t)(4 * hi) * (uint32_t)g.ld_aux + (uint32_t)j + (uint32_t)((r & 3) + 8 * (r >> 2)) * (uint32_t)g.ld_aux;
      }
      constexpr bool AUX1 = EPI == EPI_TANGENT || EPI == EPI_BACK || EPI == EPI_BACK_RELU;
      float yall[AUX1 ? MT * NT * 16 : 1];
      if (AUX1) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const float* __restrict__ ab = g.aux + (int64_t)(um + mt * 32) * g.ld_aux + (un + nt * 32);
#pragma unroll
            for (int r = 0; r < 16; ++r) yall[(mt * NT + nt) * 16 + r] = ab[offA[r]];
          }
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int col = un + nt * 32 + j;
          const float bias = USE_BIAS ? g.bias[col] : 0.f;
          const float osc = (EPI == EPI_BIAS_AFFINE || EPI == EPI_FVP_HEAD) ? g.osc[col] : 1.f;
          const float osh = (EPI == EPI_BIAS_AFFINE && g.osh) ? g.osh[col] : 0.f;
          float dk = 0.f;
          if (EPI == EPI_FVP_HEAD) { const float sg = expf(g.ls[col]); dk = 2.0f / (2.0f * sg * sg + 1e-8f); }
          float* __restrict__ cb = Cz + (int64_t)(um + mt * 32) * g.ldc + (un + nt * 32);
          float y[16], t2[16], pre[16];
          if (AUX1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) y[r] = yall[(mt * NT + nt) * 16 + r];
          } else if (USE_AUX) {                       // EPI_RBACK: three operands, per block
            const int64_t ao = (int64_t)(um + mt * 32) * g.ld_aux + (un + nt * 32);
#pragma unroll
            for (int r = 0; r < 16; ++r) { y[r] = (g.aux + ao)[offA[r]]; t2[r] = (g.aux2 + ao)[offA[r]]; pre[r] = (g.aux3 + ao)[offA[r]]; }
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = acc[mt][nt][r];
            if (EPI == EPI_BIAS_TANH) v = tanhf(v + bias);
            else if (EPI == EPI_BIAS_AFFINE) v = (v + bias) * osc + osh;
            else if (EPI == EPI_FVP_HEAD) { v = (v + bias) * osc; v = osc * (dk * v * g.inv_N); }
            else if (EPI == EPI_TANGENT) v = (v + bias) * fmaf(-y[r], y[r], 1.0f);
            else if (EPI == EPI_BACK) v = v * fmaf(-y[r], y[r], 1.0f);
            else if (EPI == EPI_RBACK) v = v * fmaf(-y[r], y[r], 1.0f) - 2.0f * y[r] * t2[r] * pre[r];
            else if (EPI == EPI_BIAS) v = v + bias;
            else if (EPI == EPI_BIAS_RELU) v = fmaxf(v + bias, 0.f);
            else if (EPI == EPI_BACK_RELU) v = (y[r] > 0.f) ? v : 0.f;
            cb[offC[r]] = v;
            if (CSUM) csum[nt] += v;
          }
        }
    } else
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + wn * TN + nt * 32 + j;
        const bool cok = col < g.N;
        const int colc = cok ? col : 0;
        const float bias = USE_BIAS ? g.bias[colc] : 0.f;
        const float osc = (EPI == EPI_BIAS_AFFINE || EPI == EPI_FVP_HEAD) ? g.osc[colc] : 1.f;
        const float osh = (EPI == EPI_BIAS_AFFINE && g.osh) ? g.osh[colc] : 0.f;
        float dk = 0.f;                           // EPI_FVP_HEAD: D = 2 / (2 sigma^2 + 1e-8) of the column's action
        if (EPI == EPI_FVP_HEAD) { const float sg = expf(g.ls[colc]); dk = 2.0f / (2.0f * sg * sg + 1e-8f); }
        const int rbase = m0 + wm * TM + mt * 32;
        float y[16], t2[16], pre[16];
        if (USE_AUX) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = rbase + unit_of(r, hi);
            const int64_t o = (row < g.M) ? (int64_t)row * g.ld_aux + colc : 0;
            y[r] = g.aux[o];
            if (EPI == EPI_RBACK) { t2[r] = g.aux2[o]; pre[r] = g.aux3[o]; }
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + unit_of(r, hi);
          float v = acc[mt][nt][r];
          if (EPI == EPI_BIAS_TANH) v = tanhf(v + bias);
          else if (EPI == EPI_BIAS_AFFINE) v = (v + bias) * osc + osh;
          else if (EPI == EPI_FVP_HEAD) { v = (v + bias) * osc; v = osc * (dk * v * g.inv_N); }     // the tangent of mu, then d3 = out_scale D mudot / N
          else if (EPI == EPI_TANGENT) v = (v + bias) * fmaf(-y[r], y[r], 1.0f);
          else if (EPI == EPI_BACK) v = v * fmaf(-y[r], y[r], 1.0f);
          else if (EPI == EPI_RBACK) v = v * fmaf(-y[r], y[r], 1.0f) - 2.0f * y[r] * t2[r] * pre[r];   // Pearlmutter R-backward through tanh
          else if (EPI == EPI_BIAS) v = v + bias;
          else if (EPI == EPI_BIAS_RELU) v = fmaxf(v + bias, 0.f);
          else if (EPI == EPI_BACK_RELU) v = (y[r] > 0.f) ? v : 0.f;
          const bool ok = cok && row < g.M;
          if (ok) Cz[(int64_t)row * g.ldc + (int64_t)col * ccs] = v;
          if (CSUM) csum[nt] += ok ? v : 0.f;
        }
      }
    if (CSUM && g.colsum) {
      // column sums of this block's 128 rows: lane halves (permlane swap), then the waves along M through LDS
      __syncthreads();                              // operand tiles are dead
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float t = half_sum(csum[nt]);
        if (hi == 0) As[wm * BN + wn * TN + nt * 32 + j] = t;
      }
      __syncthreads();
      if (tid < BN && n0 + tid < g.N) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WMc; ++w) t += As[w * BN + tid];
        g.colsum[(int64_t)blockIdx.y * (g.cs_ld ? g.cs_ld : g.N) + n0 + tid] = t;
      }
    }
  };
  switch (g.epi) {
    case EPI_BIAS_TANH: epilogue(std::integral_constant<int, EPI_BIAS_TANH>{}); break;
    case EPI_BIAS_AFFINE: epilogue(std::integral_constant<int, EPI_BIAS_AFFINE>{}); break;
    case EPI_TANGENT: epilogue(std::integral_constant<int, EPI_TANGENT>{}); break;
    case EPI_BACK: epilogue(std::integral_constant<int, EPI_BACK>{}); break;
    case EPI_RBACK: epilogue(std::integral_constant<int, EPI_RBACK>{}); break;
    case EPI_BIAS: epilogue(std::integral_constant<int, EPI_BIAS>{}); break;
    case EPI_BIAS_RELU: epilogue(std::integral_constant<int, EPI_BIAS_RELU>{}); break;
    case EPI_BACK_RELU: epilogue(std::integral_constant<int, EPI_BACK_RELU>{}); break;
    case EPI_FVP_HEAD: epilogue(std::integral_constant<int, EPI_FVP_HEAD>{}); break;
    default: epilogue(std::integral_constant<int, EPI_STORE>{}); break;
  }
  LW_STAMP(3);
}

// out[i] = sum_z part[z][i]   (fp64 accumulate, fixed order)
__global__ void k_reduce_split(const float* __restrict__ part, int Z, int64_t cnt, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
    double a = 0.0;
    for (int z = 0; z < Z; ++z) a += (double)part[(size_t)z * cnt + i];
    out[i] = (float)a;
  }
}

// the same with 16-byte loads and the splits spread over the 4 waves of a workgroup (cnt % 4 == 0): thread (w, c) sums
// slabs w, w + 4, ... of column group c in fp64, the four partial sums are added in a fixed order.  One coalesced 1 KB
// read per wave and slab; Z / 4 independent loads per thread (the scalar kernel above walks all Z slabs with one thread
// and ran at ~130 GB/s: 27 % of a cfg4 Fisher-vector product in round 1).
__global__ __launch_bounds__(256) void k_reduce_split4(const float* __restrict__ part, int Z, int64_t cnt4, float* __restrict__ out) {
  __shared__ double sh[3][64][4];
  const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + c;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (i < cnt4) {
    const f32x4* __restrict__ p = (const f32x4*)part + i;
#pragma unroll 4
    for (int z = w; z < Z; z += 4) {
      const f32x4 v = p[(int64_t)z * cnt4];
      a0 += (double)v[0]; a1 += (double)v[1]; a2 += (double)v[2]; a3 += (double)v[3];
    }
  }
  if (w > 0) { sh[w - 1][c][0] = a0; sh[w - 1][c][1] = a1; sh[w - 1][c][2] = a2; sh[w - 1][c][3] = a3; }
  __syncthreads();
  if (w == 0 && i < cnt4) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { a0 += sh[k][c][0]; a1 += sh[k][c][1]; a2 += sh[k][c][2]; a3 += sh[k][c][3]; }
    ((f32x4*)out)[i] = f32x4{(float)a0, (float)a1, (float)a2, (float)a3};
  }
}

}  // namespace mjx
