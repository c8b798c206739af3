// dfe_tiles.h -- what the kernels that keep a net's activations as LDS tiles and stream its weights from global memory share
// (dyn_fit_ens.h k_dyn_fit_ens, policy_rollout_wide.h k_policy_rollout_wide): the workgroup's shape, the [unit][sample] tile
// conventions and the forward of one layer.
//
// A tile is [unit][sample] fp32 with the sample dimension padded to the MFMA tile (32 or 64) and a row stride of that + 4; a
// hidden layer's tile has its unit rows padded to 32.  Products run on v_mfma_f32_32x32x2_f32 in the chained, operand-swapped form
// of fused_policy.h / mlp_fit.h: the A operand carries the 32 output rows of a tile, the B operand its 32 sample columns, a lane
// half (hi) takes four consecutive k of a group of eight, and accumulator register r of lane (j, hi) is element
// [unit_of(r, hi)][j] of the tile.  A B-operand column only ever reaches its own output column: samples never mix.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dynamics.h"
#include "fused_policy.h"

namespace mjx {

constexpr int DFE_THREADS = 512, DFE_WAVES = DFE_THREADS / 64;

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // four weights of a row (member blocks are 4-byte aligned)
__host__ __device__ constexpr int dfe_pad32(int d) { return (d + 31) & ~31; }      // the unit rows of a hidden layer's LDS tile

// Every phase of a step starts from "fresh" lane coordinates: without this the compiler hoists the address arithmetic of all
// the phases out of the step loop and keeps it in registers for the whole run (256 registers and spills); with it a phase's
// addresses live for that phase only.
__device__ __forceinline__ void dfe_fresh(int& w, int& j, int& hi) { asm volatile("" : "+s"(w), "+v"(j), "+v"(hi)); }

// out[u][s] = act(b[u] + sum_k W[u][k] in[k][s]) over the (ceil(dj / 32) x NS) tiles, a wave per tile.  W: dj x di row-major
// (global); Kp = di rounded up to 8, `in` has Kp rows (zeros beyond di); vec: four weights per load -- di % 8 == 0 (the
// aligned hidden widths), or, RAG, di % 4 == 0 with the groups at and beyond di masked (a group of four lies wholly inside the
// row or wholly beyond it, so no load reaches past the row).  in(k, s) reads the input tile.  Rows u >= dj of the last tile come
// out as zeros.
template <bool RAG, class LdIn>
__device__ __forceinline__ void dfe_forward(const float* __restrict__ W, const float* __restrict__ b, int dj, int di, int Kp, bool vec,
                                            LdIn in, float* out, int ST, int NS, int act, int w, int j, int hi) {
  dfe_fresh(w, j, hi);
  const int MT = (dj + 31) >> 5;
  for (int t = w; t < MT * NS; t += DFE_WAVES) {
    const int mt = t % MT, nt = t / MT;
    const int row = 32 * mt + j;
    const bool rok = row < dj;
    const float* wr = W + (int64_t)(rok ? row : 0) * di;
    f32x16 acc = (f32x16)(0.f);
    // operands of group k0 + 8 are requested before the four MFMAs of group k0 (the last trip re-reads its own group)
    auto lda = [&](int kk, float (&av)[4]) {
      if (vec) {
        const bool ok = RAG ? rok && kk < di : rok;
        const f32x4u a4 = *(const f32x4u*)(wr + (RAG ? (ok ? kk : 0) : kk));
#pragma unroll
        for (int q = 0; q < 4; ++q) av[q] = ok ? a4[q] : 0.f;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool ok = rok && kk + q < di;
          const float x = wr[ok ? kk + q : 0];
          av[q] = ok ? x : 0.f;
        }
      }
    };
    float ac[4], bc[4], an[4], bn[4];
    lda(4 * hi, ac);
#pragma unroll
    for (int q = 0; q < 4; ++q) bc[q] = in(4 * hi + q, 32 * nt + j);
    for (int k0 = 0; k0 < Kp; k0 += 8) {
      const int kk = (k0 + 8 < Kp ? k0 + 8 : k0) + 4 * hi;
      lda(kk, an);
#pragma unroll
      for (int q = 0; q < 4; ++q) bn[q] = in(kk + q, 32 * nt + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = MJX_MFMA(ac[q], bc[q], acc);
#pragma unroll
      for (int q = 0; q < 4; ++q) { ac[q] = an[q]; bc[q] = bn[q]; }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = 32 * mt + unit_of(r, hi);
      float z = 0.f;
      if (u < dj) { z = acc[r] + b[u]; if (act >= 0) z = dyn_act(z, act); }
      out[u * ST + 32 * nt + j] = z;
    }
  }
}

}  // namespace mjx
