// dfe_tiles.h -- what the kernels that keep a net's activations as LDS tiles and stream its weights from global memory share
// (dyn_fit_ens.h k_dyn_fit_ens, policy_rollout_wide.h k_policy_rollout_wide, rows_wide.h k_rollout_disagree_wide and
// k_path_rewards_wide): the workgroup's shape, the [unit][sample] tile conventions and the forward of one layer; for the three
// forward-only kernels also their shape limits, the staging of a member's small vectors, the net as a workgroup reads it (WideNet),
// its forward through two or three layers and the normaliser that fills an input tile; for the two rollout kernels (plan_wide.h,
// policy_rollout_wide.h) the tile-row stride and the thread mapping.
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
#include "mfma_prims.h"

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

// ---- the kernels that only run nets forward (policy_rollout_wide.h, rows_wide.h): two hidden layers up to WIDE_MAXH wide, weights
// streamed from the member's flat torch-layout vector, the small vectors staged into LDS once per workgroup.
constexpr int WIDE_MAXH = 256, WIDE_MAXN = 64, WIDE_MAXM = 64, WIDE_MAXIN = 128;     // hidden widths, n, m, n + m

// the next `count` floats of the staged vectors <- src (EXP: exp(src)); -> their LDS copy
template <bool EXP = false>
__device__ __forceinline__ const float* dfe_stage(float*& cst, const float* __restrict__ src, int count, int tid) {
  float* dst = cst;
  for (int e = tid; e < count; e += DFE_THREADS) dst[e] = EXP ? expf(src[e]) : src[e];
  cst += count;
  return dst;
}
// One net [din, h1, h2, dout] as a workgroup reads it: the weights in global memory, the small vectors staged (LDS).
struct WideNet {
  const float* W1; const float* W2; const float* W3;        // (W3 staged too where the head is no MFMA layer: HEAD)
  const float* b1; const float* b2; const float* b3;
  const float* tail;                                        // exp of what follows b3 in the flat vector (a policy's log_std), if asked for
  const float* tr;                                          // [in_shift din, in_scale din, out_shift dout, out_scale dout]
  int din, h1, h2, dout, act;
};
// P: the flat vector W1 b1 W2 b2 W3 b3 [tail]; staged in the order b1, b2, [W3,] b3, [exp(tail),] tr
template <bool HEAD = false>
__device__ __forceinline__ WideNet dfe_stage_net(float*& cst, const float* __restrict__ P, const float* __restrict__ tr, int din, int h1, int h2,
                                                 int dout, int act, int ntail, int tid) {
  WideNet d;
  d.W1 = P; const float* b1 = d.W1 + (int64_t)h1 * din; d.W2 = b1 + h1; const float* b2 = d.W2 + (int64_t)h2 * h1;
  d.W3 = b2 + h2; const float* b3 = d.W3 + (int64_t)dout * h2;
  d.b1 = dfe_stage(cst, b1, h1, tid); d.b2 = dfe_stage(cst, b2, h2, tid);
  if (HEAD) d.W3 = dfe_stage(cst, d.W3, dout * h2, tid);
  d.b3 = dfe_stage(cst, b3, dout, tid);
  d.tail = dfe_stage<true>(cst, b3 + dout, ntail, tid);
  d.tr = dfe_stage(cst, tr, 2 * din + 2 * dout, tid);
  d.din = din; d.h1 = h1; d.h2 = h2; d.dout = dout; d.act = act;
  return d;
}
// The hidden layers: x (pad8(din) rows, zeros beyond din) -> y1 -> y2, tiles of NS sample tiles of 32 columns, row stride 32 NS + 4;
// a workgroup barrier after each layer.  x and y2 may be one region.  (NS is a template parameter so that the tile readers hold
// the stride as a constant: as a captured run-time value it costs every forward ten registers.)
template <int NS>
__device__ __forceinline__ void dfe_forward2(const WideNet& d, const float* x, float* y1, float* y2, int w, int j, int hi) {
  constexpr int ST = 32 * NS + 4;
  dfe_forward<true>(d.W1, d.b1, d.h1, d.din, pad8(d.din), d.din % 4 == 0, [&](int r, int cc) { return x[r * ST + cc]; }, y1, ST, NS, d.act, w, j, hi);
  __syncthreads();
  dfe_forward<true>(d.W2, d.b2, d.h2, d.h1, pad8(d.h1), d.h1 % 4 == 0, [&](int r, int cc) { return y1[r * ST + cc]; }, y2, ST, NS, d.act, w, j, hi);
  __syncthreads();
}
// ... and the output layer, no activation: y2 -> z (pad32(dout) rows; z and y1 may be one region)
template <int NS>
__device__ __forceinline__ void dfe_forward3(const WideNet& d, const float* x, float* y1, float* y2, float* z, int w, int j, int hi) {
  constexpr int ST = 32 * NS + 4;
  dfe_forward2<NS>(d, x, y1, y2, w, j, hi);
  dfe_forward<true>(d.W3, d.b3, d.dout, d.h2, pad8(d.h2), d.h2 % 4 == 0, [&](int r, int cc) { return y2[r * ST + cc]; }, z, ST, NS, -1, w, j, hi);
  __syncthreads();
}
// Rows into a tile: X[r0 + i][c] = (v - tr[r0 + i]) / (tr[sc + r0 + i] + 1e-8) for the 32 NS columns c and i < width (tr: the
// net's staged transforms, the scales sc floats behind the shifts), v = src(e, c, i) for element e = c width + i (a stored
// row-major block reads src[e]) and 0 for the columns that do not exist (c >= live).
template <int NS, class Src>
__device__ __forceinline__ void dfe_norm_rows(float* X, int r0, int width, int live, const float* tr, int sc, int tid, Src src) {
  constexpr int TILE = 32 * NS, ST = TILE + 4;
  for (int e = tid; e < TILE * width; e += DFE_THREADS) {
    const int c = e / width, i = e - c * width;
    const float v = c < live ? src(e, c, i) : 0.f;
    X[(r0 + i) * ST + c] = (v - tr[r0 + i]) / (tr[sc + r0 + i] + 1e-8f);
  }
}
// ... and zeros in the rows r0 .. r1 - 1 that pad the tile's K dimension
template <int NS>
__device__ __forceinline__ void dfe_zero_rows(float* X, int r0, int r1, int tid) {
  constexpr int TILE = 32 * NS, ST = TILE + 4;
  for (int e = tid; e < (r1 - r0) * TILE; e += DFE_THREADS) X[(r0 + e / TILE) * ST + e % TILE] = 0.f;
}

// ---- the two rollout kernels (plan_wide.h k_plan_rollout_wide, policy_rollout_wide.h k_policy_rollout_wide): a workgroup is ONE
// tile of 32 trajectories of one member through all H steps
constexpr int WR_ST = 32 + 4;                               // floats a tile row
constexpr int WR_UQ = DFE_THREADS / 32;                     // rows between a thread's elements
constexpr int WR_NZ = WIDE_MAXM / WR_UQ;                    // action rows a thread owns (m <= 64): f = u0 + WR_UQ q
// a thread's elements of a [rows][32] block: e = tid + DFE_THREADS q is row e / 32 = u0 + WR_UQ q, sample column c = tid % 32, which
// is trajectory blockIdx.x * 32 + c of the call (valid: it exists; vrow: that row, or row 0 where it does not, for addresses)
struct WideRollMap { int c, u0; bool valid; int64_t vrow; };
__device__ __forceinline__ WideRollMap wr_map(int tid, int64_t N) {
  WideRollMap t;
  t.c = tid & 31; t.u0 = tid >> 5;
  const int64_t row = (int64_t)blockIdx.x * 32 + t.c;
  t.valid = row < N;
  t.vrow = t.valid ? row : 0;
  return t;
}

}  // namespace mjx
