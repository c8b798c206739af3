// rows_wide.h -- the two passes over STORED model rollouts for the nets the register chains of rollout_batch.h and path_reward.h
// do not hold: dynamics nets up to 256 x 256 (the shape of both configs the reference ships), reward nets up to 256 x 256, any
// hidden width 1 .. 256.
//
//   k_rollout_disagree_wide<NS>  k_rollout_disagree's quantity: member k's per-row error mean_c (obs[p][t + 1][c] - f_k(obs[p][t],
//                                act[p][t])[c])^2 over the P x H stored rows, f_k unclamped; all members read the same rows.  The
//                                last row of a path (t = H - 1) is computed and never stored.  k_rd_max (rollout_batch.h) then takes
//                                the maximum over the members in member order.
//   k_path_rewards_wide<NS>      k_path_rewards' quantity: r[k][row] = RewardNet_k(s, a, s') with s' = DynamicsNet_k(s, a)
//                                recomputed and unclamped, s = member k's own observation row, a = member k's action row or the
//                                shared one (act_stride 0).
// Both run rw_next_state, the dynamics half, and are otherwise apart: either can be taken out without touching the other.  The
// shape limits, the staging of a member's small vectors, the net view (WideNet), its forward and the normaliser are dfe_tiles.h's.
//
// The scheme is k_policy_rollout_wide's and k_dyn_fit_ens's (dfe_tiles.h): activations as [unit][sample] LDS tiles, weights
// streamed row-major from global memory, products on v_mfma_f32_32x32x2_f32 through dfe_forward<true>, DFE_THREADS threads.  Stored
// rows have no step-to-step dependence, so a workgroup takes tiles of 32 NS rows (NS = 2: 64 rows, row stride 68 floats, as the
// fit's Bp = 64) and every streamed weight serves 32 NS samples.  Grid (min(tiles, ceil(CUs / K)), K): a workgroup belongs to one
// member, stages that member's small vectors (biases, transforms, head weights) into LDS once and walks its tiles in a grid-stride
// loop, with a workgroup barrier between the phases.
//
// LDS: two ping-pong regions A and B of [unit][sample] rows, ST = 32 NS + 4 floats a row, then the staged vectors.  A phase reads
// one region and writes the other (n <= 64, m <= 64, n + m <= 128, hidden widths <= 256):
//   normalise [s, a]                     global -> XD in B (pad8(n + m) rows, padding rows zero)
//   H1 = act(W1 XD + b1)                 B -> A
//   H2                                   A -> B
//   Z3 = W3 H2 + b3                      B -> A (pad32(n) rows)
//   s' = flags(Z3), unclamped            A -> A (affine 1, mask 2, residual 4; the raw s re-read from global memory)
//   disagreement: the mean               A + the next stored state from global memory -> member means in scratch
//   reward only: XR = normalised [s, a, s'] under the reward transforms (s, a re-read from global memory)
//                                        A, global -> B (pad8(2 n + m) rows, padding rows zero)
//   G1 = act(V1 XR + c1)                 B -> A
//   G2                                   A -> B
//   head                                 B -> partial dots in A (DFE_THREADS / (32 NS) rows) -> r32 / r64
// rows of A = max(pad32(h1), pad32(n), pad32(g1)), rows of B = max(pad8(n + m), pad32(h2), pad8(2 n + m), pad32(g2)); the most a
// served shape takes is 512 x 68 x 4 B = 139 264 B of tiles plus 8 460 B of staged vectors (rows_wide_lds_floats; the kernels have
// no static LDS).
//
// Summation orders (fixed: no atomics, no reductions across lanes, the same bits on every run).  Disagreement: the thread that owns
// a sample column adds d * d (d = next - s' and its square in fp32) for c = 0 .. n - 1 in index order, from 0, in an fp64 sum, divides
// by n and casts to fp32: k_rd_reduce's arithmetic.  (An fp32 fmaf sum in the same order, one thread and 64 terms long, is 4.8e-7 from
// the fp64 oracle at n = 64 even on correctly rounded s' -- over the 3.5e-7 that three times the fp32 torch restatement's own
// distance allows, tests/_rows_wide_cases.py; the fp64 sum is 6.7e-8 and costs a column's thread n additions a tile.)
// Reward head: thread (column, q) adds G2[u] * w3[u] with fmaf for u = q, q + Q, ... (Q = DFE_THREADS / (32 NS)) from 0; the column's
// thread adds the Q partial dots in q order from partial 0, then (dot + b3) * (out_scale + 1e-8) + out_shift.
//
// Padded unit rows of every tile are exact zeros (dfe_forward writes zeros there whatever act(b) would be); padded sample columns
// (row >= rows) start from zeros, are computed and never stored.  A sample column reaches only its own output column, so a NaN
// row stays alone.
//
// Out of scope: more or fewer than two hidden layers, several workgroups per tile, bf16x3 products.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfe_tiles.h"
#include "path_reward.h"
#include "rollout_batch.h"

namespace mjx {

#ifndef MJX_RW_NS
#define MJX_RW_NS 2                                         // (-DMJX_RW_NS=1: the 32-row tile, for A/B builds; tools/bench_rows_wide.py)
#endif
constexpr int RW_NS = MJX_RW_NS;                            // sample tiles of 32 rows a workgroup's tile holds (the shipped instance)
__host__ __device__ constexpr int rw_max(int a, int b) { return a > b ? a : b; }
// rows of the two regions; g1 = g2 = 0: the disagreement kernel, which holds no reward net
__host__ __device__ constexpr int rw_rows_a(int n, int h1, int g1) { return rw_max(rw_max(dfe_pad32(h1), dfe_pad32(n)), dfe_pad32(g1)); }
__host__ __device__ constexpr int rw_rows_b(int n, int m, int h2, int g1, int g2) {
  return rw_max(rw_max(pad8(n + m), dfe_pad32(h2)), g1 > 0 ? rw_max(pad8(2 * n + m), dfe_pad32(g2)) : 0);
}
// floats of the small vectors staged once: the member's b1, b2, b3 and 2 (n + m) + 2 n transforms; with a reward net its c1, c2, w3,
// b3 and 2 (2 n + m) + 2 transforms
__host__ __device__ constexpr int rw_const_floats(int n, int m, int h1, int h2, int g1, int g2) {
  return h1 + h2 + n + (2 * (n + m) + 2 * n) + (g1 > 0 ? g1 + 2 * g2 + 1 + (2 * (2 * n + m) + 2) : 0);
}
__host__ __device__ constexpr size_t rows_wide_lds_floats(int n, int m, int h1, int h2, int g1, int g2, int ns = RW_NS) {
  return (size_t)(rw_rows_a(n, h1, g1) + rw_rows_b(n, m, h2, g1, g2)) * (32 * ns + 4) + rw_const_floats(n, m, h1, h2, g1, g2);
}
// (the count itself, pinned: the largest served shape, the reference's config with and without its reward net, the smallest shape)
static_assert(rows_wide_lds_floats(64, 64, 256, 256, 256, 256, 2) == 68 * 512 + 2115, "rows_wide_lds_floats");
static_assert(rows_wide_lds_floats(11, 2, 256, 256, 100, 100, 2) == 68 * 512 + 922, "rows_wide_lds_floats");
static_assert(rows_wide_lds_floats(11, 2, 256, 256, 0, 0, 2) == 68 * 512 + 571, "rows_wide_lds_floats");
static_assert(rows_wide_lds_floats(17, 6, 160, 96, 33, 130, 2) == 68 * 320 + 729, "rows_wide_lds_floats");
static_assert(rows_wide_lds_floats(1, 1, 1, 1, 0, 0, 1) == 36 * 64 + 9, "rows_wide_lds_floats");

// The dynamics half for one tile: s' of the tile's rows, unclamped, left in A's first n rows (element [c][col]).  so, sa: the
// tile's first stored row of observations and actions (rows are contiguous); live: its rows that exist (1 .. 32 NS).  Starts by
// writing B and ends with a barrier; what the caller last read from B lies behind a barrier of its own.
template <int NS>
__device__ __forceinline__ void rw_next_state(const WideNet& d, int flags, const float* __restrict__ so, const float* __restrict__ sa, int live,
                                              float* A, float* B, int tid, int w, int j, int hi) {
  constexpr int TILE = 32 * NS, ST = TILE + 4;
  const int n = d.dout, din = d.din, m = din - n;
  const float* tr = d.tr;
  dfe_norm_rows<NS>(B, 0, n, live, tr, din, tid, [&](int e, int, int) { return so[e]; });
  dfe_norm_rows<NS>(B, n, m, live, tr, din, tid, [&](int e, int, int) { return sa[e]; });
  dfe_zero_rows<NS>(B, din, pad8(din), tid);
  __syncthreads();
  dfe_forward3<NS>(d, B, A, B, A, w, j, hi);
  const float* osh = tr + 2 * din; const float* osc = osh + n;
  for (int e = tid; e < TILE * n; e += DFE_THREADS) {
    const int c = e / n, i = e - c * n;
    A[i * ST + c] = dyn_out_flags(A[i * ST + c], flags, osh, osc, i, [&] { return c < live ? so[e] : 0.f; });
  }
  __syncthreads();
}

// ---- disagreement.  RollDisArgs as mjx_rollout_disagreement fills them (rollout_batch.h)
template <int NS>
__global__ __launch_bounds__(DFE_THREADS) void k_rollout_disagree_wide(RollDisArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rwl[];
  constexpr int TILE = 32 * NS, ST = TILE + 4;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int n = a.n, m = a.m, H = a.H, k = blockIdx.y;
  float* A = rwl; float* B = A + rw_rows_a(n, a.h1, 0) * ST;
  float* cst = B + rw_rows_b(n, m, a.h2, 0, 0) * ST;
  const WideNet d = dfe_stage_net(cst, a.dP + k * a.dPstride, a.dtr + (int64_t)k * (2 * (n + m) + 2 * n), n + m, a.h1, a.h2, n, a.dact, 0, tid);
  __syncthreads();                                          // (the staged vectors)
  const int64_t tiles = (a.rows + TILE - 1) / TILE, R = (a.rows / H) * (H - 1);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * TILE;
    const int live = a.rows - base < TILE ? (int)(a.rows - base) : TILE;
    rw_next_state<NS>(d, a.flags, a.obs + base * n, a.act + base * m, live, A, B, tid, w, j, hi);
    // the thread that owns a column: its row against the next stored state (the last row of a path has none: never stored)
    if (tid < live) {
      const int64_t row = base + tid, p = row / H;
      const int t = (int)(row - p * H);
      if (t < H - 1) {
        const float* __restrict__ nx = a.obs + (row + 1) * n;
        double acc = 0.0;
        for (int c = 0; c < n; ++c) {
          const float df = nx[c] - A[c * ST + tid];
          acc += (double)(df * df);
        }
        a.mk[(int64_t)k * R + p * (H - 1) + t] = (float)(acc / n);
      }
    }
    // (the next tile writes B, then passes a barrier before it writes A)
  }
}

// ---- learned path rewards.  PathRewArgs as mjx_path_rewards fills them (path_reward.h)
template <int NS>
__global__ __launch_bounds__(DFE_THREADS) void k_path_rewards_wide(PathRewArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rwl[];
  constexpr int TILE = 32 * NS, ST = TILE + 4, Q = DFE_THREADS / TILE;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int n = a.n, m = a.m, din = n + m, rin = din + n, g1 = a.g1, g2 = a.g2, k = blockIdx.y;
  float* A = rwl; float* B = A + rw_rows_a(n, a.h1, g1) * ST;
  float* cst = B + rw_rows_b(n, m, a.h2, g1, g2) * ST;
  const WideNet d = dfe_stage_net(cst, a.dP + k * a.dPstride, a.dtr + (int64_t)k * (2 * din + 2 * n), din, a.h1, a.h2, n, a.dact, 0, tid);
  // the reward net: its head w3 (g2 weights, d_out = 1) is staged with the biases
  const WideNet r = dfe_stage_net<true>(cst, a.rP + k * a.rPstride, a.rtr + (int64_t)k * (2 * rin + 2), rin, g1, g2, 1, a.ract, 0, tid);
  const float* rtr = r.tr;
  __syncthreads();                                          // (the staged vectors)
  const float* __restrict__ obase = a.obs + (int64_t)k * a.rows * n;
  const float* __restrict__ abase = a.actions + k * a.act_stride;
  const int64_t tiles = (a.rows + TILE - 1) / TILE;
  const int col = tid % TILE, q0 = tid / TILE;              // the head: this thread's column and its share of the units
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * TILE;
    const int live = a.rows - base < TILE ? (int)(a.rows - base) : TILE;
    const float* __restrict__ so = obase + base * n;
    const float* __restrict__ sa = abase + base * m;
    rw_next_state<NS>(d, a.flags, so, sa, live, A, B, tid, w, j, hi);
    // ---- XR = [s, a, s'] under the reward net's own shift and scale (s' of every column, as A holds it)
    dfe_norm_rows<NS>(B, 0, n, live, rtr, rin, tid, [&](int e, int, int) { return so[e]; });
    dfe_norm_rows<NS>(B, din, n, TILE, rtr, rin, tid, [&](int, int c, int i) { return A[i * ST + c]; });
    dfe_norm_rows<NS>(B, n, m, live, rtr, rin, tid, [&](int e, int, int) { return sa[e]; });
    dfe_zero_rows<NS>(B, rin, pad8(rin), tid);
    __syncthreads();
    dfe_forward2<NS>(r, B, A, B, w, j, hi);
    // ---- the scalar head (d_out = 1) is no MFMA: Q partial dots per column, then the column's thread adds them in order
    float dot = 0.f;
    for (int u = q0; u < g2; u += Q) dot = fmaf(B[u * ST + col], r.W3[u], dot);
    A[q0 * ST + col] = dot;
    __syncthreads();
    if (tid < live) {
      float sum = A[tid];
#pragma unroll
      for (int q = 1; q < Q; ++q) sum += A[q * ST + tid];
      const float z = (sum + r.b3[0]) * (rtr[2 * rin + 1] + 1e-8f) + rtr[2 * rin];     // out * (out_scale + 1e-8) + out_shift
      const int64_t row = base + tid;
      if (a.r32) a.r32[(int64_t)k * a.rows + row] = z;
      if (a.r64) a.r64[(int64_t)k * a.rows + row] = (double)z;
    }
    // (the next tile writes B, which was last read before the barrier above, then passes a barrier before it writes A)
  }
}

}  // namespace mjx
