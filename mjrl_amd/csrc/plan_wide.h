// plan_wide.h -- k_plan_rollout_wide: k_plan_rollout's job (plan.h: the rollout of GIVEN action sequences (N, H, m), shared by the
// K members, from s0, storing obs (K, N, H, n)) for the nets its register chain does not hold: dynamics nets up to 256 x 256 (the
// shape of both configs the reference ships), any hidden width 1 .. 256, n <= 64, m <= 64, n + m <= 128 (wide_nets_ok).
//
// The scheme, the tile conventions, the thread mapping (dfe_tiles.h wr_map), the padding rules and what is out of scope are
// k_policy_rollout_wide's (policy_rollout_wide.h), and a step has its order and expressions.  What is different here:
//
// No policy half.  The layout is S | XD | H1 | H2 | Z3 and the member's staged vectors; Z3 keeps rows of its own (it could take
// H1's, as rows_wide.h's regions do): the largest served shape (64, 64, 256 x 256) is (768 x 36 + 960) x 4 B = 114 432 B without
// that, and a grid of a few dozen workgroups (the planner's call, K 4, N 250, is 32 on 256 CUs) leaves nothing to gain from a
// smaller footprint.  plan_wide_lds_floats is the only place that sums the layout; the kernel has no static LDS.  There is no
// clamp (trajectory_rollout has none), and the forward after the last stored state is not run.
//
// The actions are known a step ahead.  Thread (u0, c) owns the action rows f = u0 + 16 q of sample column c.  It requests those of
// step t + 1 from global memory into registers BEFORE the forward of step t and writes them into XD AFTER that forward, so the
// load is in flight under the three layers.  Only layer 1 reads XD, and dfe_forward2's barrier after layer 1 stands between every
// wave's last read of XD and this write; the barrier that ends the next step's first phase stands between the write and layer
// 1's next read.  (The policy kernel writes its action rows before the forward: its actions come out of the policy of the same
// step.)  A step is then: store s and the state rows of XD | request the actions of step t + 1 | H1 | H2 | Z3 | flags -> S; the
// action rows of XD for step t + 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfe_tiles.h"
#include "plan.h"

namespace mjx {

// the layout: S | XD | H1 | H2 | Z3 rows, then the staged vectors (b1, b2, b3, transforms)
__host__ __device__ constexpr size_t plan_wide_lds_floats(int n, int m, int h1, int h2) {
  return (size_t)(n + pad8(n + m) + dfe_pad32(h1) + dfe_pad32(h2) + dfe_pad32(n)) * WR_ST + (h1 + h2 + n + 2 * (n + m) + 2 * n);
}
// (the count itself, pinned: the largest served shape, the reference's config, a ragged shape, the smallest shape)
static_assert(plan_wide_lds_floats(64, 64, 256, 256) == 36 * 768 + 960, "plan_wide_lds_floats");
static_assert(plan_wide_lds_floats(64, 64, 256, 256) * sizeof(float) == 114432, "plan_wide_lds_floats");
static_assert(plan_wide_lds_floats(11, 2, 256, 256) == 36 * (11 + 16 + 256 + 256 + 32) + 571, "plan_wide_lds_floats");
static_assert(plan_wide_lds_floats(17, 6, 160, 96) == 36 * (17 + 24 + 160 + 96 + 32) + 353, "plan_wide_lds_floats");
static_assert(plan_wide_lds_floats(1, 1, 1, 1) == 36 * (1 + 8 + 32 + 32 + 32) + 9, "plan_wide_lds_floats");

// PlanArgs as mjx_plan_rollout fills them (plan.h)
__global__ __launch_bounds__(DFE_THREADS) void k_plan_rollout_wide(PlanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float plw[];
  constexpr int ST = WR_ST, UQ = WR_UQ, NZ = WR_NZ;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int n = a.n, m = a.m, din = n + m, h1 = a.h1, h2 = a.h2;
  const int K0 = pad8(din);
  float* S = plw; float* XD = S + n * ST;
  float* H1 = XD + K0 * ST; float* H2 = H1 + dfe_pad32(h1) * ST; float* Z3 = H2 + dfe_pad32(h2) * ST;
  const int k = blockIdx.y;
  // the small vectors of member k go to LDS once (a phase would otherwise wait a round trip to L2 for them)
  float* cst = Z3 + dfe_pad32(n) * ST;
  const WideNet dyn = dfe_stage_net(cst, a.P + k * a.Pstride, a.tr + (int64_t)k * (2 * din + 2 * n), din, h1, h2, n, a.act, 0, tid);
  const float* dtr = dyn.tr;
  const WideRollMap tm = wr_map(tid, a.N);
  const int c = tm.c, u0 = tm.u0;
  const bool valid = tm.valid;
  const int64_t vrow = tm.vrow;
  float* __restrict__ orow = a.obs + ((int64_t)k * a.N + vrow) * a.H * (int64_t)n;
  const float* __restrict__ arow = a.actions + vrow * a.H * (int64_t)m;
  float an[NZ];
#pragma unroll
  for (int q = 0; q < NZ; ++q) { const int f = u0 + UQ * q; an[q] = (valid && f < m) ? arow[f] : 0.f; }
  for (int i = u0; i < n; i += UQ) S[i * ST + c] = valid ? a.s0[vrow * a.s0_stride + i] : 0.f;
  for (int i = din + u0; i < K0; i += UQ) XD[i * ST + c] = 0.f;
  __syncthreads();                                          // (the staged vectors)
#pragma unroll
  for (int q = 0; q < NZ; ++q) {                            // the action rows of step 0
    const int f = u0 + UQ * q;
    if (f < m) XD[(n + f) * ST + c] = (an[q] - dtr[n + f]) / (dtr[din + n + f] + 1e-8f);
  }
  for (int t = 0; t < a.H; ++t) {
    // ---- observations[:, t] is the state BEFORE step t; the state rows of the dynamics input
    for (int i = u0; i < n; i += UQ) {
      const float s = S[i * ST + c];
      if (valid) orow[(int64_t)t * n + i] = s;
      XD[i * ST + c] = (s - dtr[i]) / (dtr[din + i] + 1e-8f);
    }
    if (t + 1 == a.H) break;                                // (uniform: the last stored state needs no successor)
    if (valid) {                                            // the next step's actions: in flight under the forward
#pragma unroll
      for (int q = 0; q < NZ; ++q) { const int f = u0 + UQ * q; if (f < m) an[q] = arow[(int64_t)(t + 1) * m + f]; }
    }
    __syncthreads();
    // ---- the dynamics forward of member k
    dfe_forward3<1>(dyn, XD, H1, H2, Z3, w, j, hi);
    // ---- flags: the next state over S (element (i, c) belongs to the thread that reads it next)
    const float* osh = dtr + 2 * din; const float* osc = osh + n;
    for (int i = u0; i < n; i += UQ) S[i * ST + c] = dyn_out_flags(Z3[i * ST + c], a.flags, osh, osc, i, [&] { return S[i * ST + c]; });
    // ---- the action rows of step t + 1 (layer 1, XD's only reader, lies behind dfe_forward2's first barrier)
#pragma unroll
    for (int q = 0; q < NZ; ++q) {
      const int f = u0 + UQ * q;
      if (f < m) XD[(n + f) * ST + c] = (an[q] - dtr[n + f]) / (dtr[din + n + f] + 1e-8f);
    }
  }
}

}  // namespace mjx
