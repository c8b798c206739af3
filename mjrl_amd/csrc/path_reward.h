// path_reward.h -- learned path rewards for every ensemble member at once (WorldModel.compute_path_rewards / WorldModel.reward,
// nn_dynamics.py:65-77, 149-164 over DynamicsNet.forward :230-245 and RewardNet.forward :313-328):
//
//   k_path_rewards<HB, NB, RB>  r[k][row] = RewardNet_k(s, a, s') with s' = DynamicsNet_k(s, a) recomputed and unclamped, s = member k's
//                               own observation row, a = member k's action row or the shared one (act_stride 0, the planner's case).
//                               Grid (workgroups, K), 256 threads: a workgroup belongs to one member, stages BOTH nets into LDS once and
//                               each of its four waves then walks tiles of 32 rows (a grid-stride loop over tiles).
//   k_pr_gather_sa / k_pr_gather_sp / k_pr_widen
//                               the pieces of the generic route, which runs k_dyn_forward twice: [s, a] and [s, a, s'] rows assembled
//                               in scratch, and the fp64 copy of the result
//
// A register-chained MFMA MLP twice over (mfma_chain.h: the scheme, the dynamics net's LDS image and the pieces of a forward).  One step
// further than the rollout of plan.h: the dynamics net's OUTPUT accumulator -- s' -- is the s' part of the reward net's layer-1 B operand
// as it lies, the s registers that fed the dynamics layer 1 feed the reward layer 1 again (with the reward net's own shift and scale), and
// so do the action slots.  No activation passes through LDS and there is no barrier after the prologue.
//
// The reward net's input features are laid out [s padded to n8 | a padded to m8 | s' padded to n8]; its W1's columns are permuted and
// zero-padded to that layout when they are staged.  Each hidden width is padded to whole 32-blocks, R1 = 32 g1b and R2 = 32 g2b units,
// with zero weights and biases (100 -> 128, 36 -> 64, 72 -> 96): a padded unit is act(0) = 0 for ReLU and tanh and meets zero columns
// downstream and a zero head weight, so the padding adds exact zeros to every sum.  The block counts are run-time values up to the
// instance's RB (2 or 4): the image and the MFMA count follow the net, not the instance, and W2's K dimension is R1, not 32 RB.  The head (d_out = 1) is no MFMA: each lane dots its 16 RB registers of h2
// with the head's weights and the two lane halves are added once.
//
// LDS image (floats): the dynamics image (DynImage, plan_lds_floats), then
//   V1s R1 x (K1r + 4) | V2s R2 x (R1 + 4) | c1 R1 | c2 R2 | w3 R2 | in_shift K1r | in_scale + 1e-8 K1r | b3, out_scale + 1e-8, out_shift, 0
// with K1r = 2 n8 + m8.  (17, 6) at dynamics 64 x 64, reward 100 x 100: 35.8 + 98.0 = 133.7 KiB of the 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_chain.h"

namespace mjx {

struct PathRewArgs {
  const float* obs;                     // K x rows x n
  const float* actions; int64_t act_stride;   // member k reads actions + k * act_stride (0: all members share the rows x m block)
  const float* dP; const float* dtr;    // dynamics: K x dPstride, K x (2 (n + m) + 2 n)
  const float* rP; const float* rtr;    // reward:   K x rPstride, K x (2 (2 n + m) + 2)
  float* r32; double* r64;              // K x rows each; either may be null
  int64_t rows, dPstride, rPstride;
  int n, m, h1, h2, dact, flags;        // dynamics net [n + m, h1, h2, n]
  int g1, g2, ract;                     // reward net   [2 n + m, g1, g2, 1]
};

__host__ __device__ inline size_t path_rew_lds_floats(int g1, int g2, int n, int m) {
  const size_t R1 = 32 * (size_t)((g1 + 31) / 32), R2 = 32 * (size_t)((g2 + 31) / 32), K1r = 2 * (size_t)pad8(n) + pad8(m);
  return R1 * (K1r + 4) + R2 * (R1 + 4) + R1 + 2 * R2 + 2 * K1r + 4;
}

template <int HB, int NB, int RB>
__global__ __launch_bounds__(256, 1) void k_path_rewards(PathRewArgs a) {
  extern __shared__ __attribute__((aligned(16))) float prs[];
  const int n = a.n, m = a.m, g1 = a.g1, g2 = a.g2;
  const int g1b = (g1 + 31) >> 5, g2b = (g2 + 31) >> 5, R1 = 32 * g1b, R2 = 32 * g2b, T2 = R1 + 4;      // blocks in use: g1b, g2b <= RB
  DynImage<HB, NB> im;
  float* V1s = im.carve(prs, n, m);
  const int K1 = im.K1, din = n + m, K1r = K1 + im.n8, T1 = K1r + 4, rin = din + n;
  float* V2s = V1s + R1 * T1; float* c1s = V2s + R2 * T2; float* c2s = c1s + R1; float* w3s = c2s + R2;
  float* rsh = w3s + R2; float* rrs = rsh + K1r; float* hd = rrs + K1r;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const ChainLane L{j, hi};
  const ChainL1 rl1{V1s, T1, rsh, rrs};
  const int k = blockIdx.y;
  const float* __restrict__ Q = a.rP + k * a.rPstride;
  const float* __restrict__ qtr = a.rtr + (int64_t)k * (2 * rin + 2);
  const int64_t qB1 = (int64_t)g1 * rin, qW2 = qB1 + g1, qB2 = qW2 + (int64_t)g2 * g1, qW3 = qB2 + g2, qB3 = qW3 + g2;
  // ---- prologue: the dynamics net as k_plan_rollout stages it ...
  im.stage(a.dP + k * a.dPstride, a.dtr + (int64_t)k * (2 * din + 2 * n), a.h1, a.h2, tid);
  // ... and the reward net, a wave staging whole rows: column c of the padded layout is input feature im.feat(c) of [s, a, s'] or none
  for (int u = tid >> 6; u < R1; u += 4)
    for (int c = lane; c < K1r; c += 64) {
      const int f = im.feat(c);
      V1s[u * T1 + c] = (u < g1 && f >= 0) ? Q[(int64_t)u * rin + f] : 0.f;
    }
  for (int u = tid >> 6; u < R2; u += 4)
    for (int c = lane; c < R1; c += 64) V2s[u * T2 + c] = (u < g2 && c < g1) ? Q[qW2 + (int64_t)u * g1 + c] : 0.f;
  for (int i = tid; i < R1; i += 256) c1s[i] = i < g1 ? Q[qB1 + i] : 0.f;
  for (int i = tid; i < R2; i += 256) {
    c2s[i] = i < g2 ? Q[qB2 + i] : 0.f;
    w3s[i] = i < g2 ? Q[qW3 + i] : 0.f;
  }
  for (int c = tid; c < K1r; c += 256) {
    const int f = im.feat(c);
    rsh[c] = f >= 0 ? qtr[f] : 0.f;
    rrs[c] = f >= 0 ? qtr[rin + f] + 1e-8f : 1.f;
  }
  if (tid == 0) { hd[0] = Q[qB3]; hd[1] = qtr[2 * rin + 1] + 1e-8f; hd[2] = qtr[2 * rin]; hd[3] = 0.f; }
  __syncthreads();
  const int NQS = im.n8 / 8, NQA = im.m8 / 8;
  const float* __restrict__ obase = a.obs + (int64_t)k * a.rows * n;
  const float* __restrict__ abase = a.actions + k * a.act_stride;
  // ---- the tiles of this wave (no barrier from here on)
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile * 32 < a.rows; tile += (int64_t)gridDim.x * 4) {
    const int64_t row = tile * 32 + j;
    const bool valid = row < a.rows;
    const int64_t vrow = valid ? row : 0;
    f32x16 s[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = 32 * b + unit_of(r, hi);
        const float v = obase[vrow * n + (f < n ? f : 0)];
        s[b][r] = (valid && f < n) ? v : 0.f;
      }
    // this lane's action slots: slot (q, tt) is action 8 q + 4 hi + tt
    float an[PLAN_MAX_M8 / 2];
#pragma unroll
    for (int q = 0; q < PLAN_MAX_M8 / 8; ++q)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int f = 8 * q + 4 * hi + tt;
        const float v = abase[vrow * m + ((q < NQA && f < m) ? f : 0)];
        an[4 * q + tt] = (valid && q < NQA && f < m) ? v : 0.f;
      }
    // -- the dynamics net: normalise, layer 1 (the action part, then the state part), the rest -> s' (blocks beyond n stay exactly 0)
    f32x16 h1v[HB];
#pragma unroll
    for (int mb = 0; mb < HB; ++mb) h1v[mb] = (f32x16)(0.f);
    chain_l1_actions(h1v, HB, im.l1(), L, im.n8, an, NQA);
    chain_l1_state(h1v, HB, im.l1(), L, 0, s, NQS);
    f32x16 sp[NB];
    im.tail(L, h1v, s, sp, a.dact, a.flags);
    __builtin_amdgcn_sched_barrier(0);
    // -- reward layer 1 over [s | a | s']: the same registers again, under the reward net's own shift and scale
    f32x16 g1v[RB];
#pragma unroll
    for (int mb = 0; mb < RB; ++mb) g1v[mb] = (f32x16)(0.f);
    chain_l1_actions(g1v, g1b, rl1, L, im.n8, an, NQA);
    chain_l1_state(g1v, g1b, rl1, L, 0, s, NQS);
    chain_l1_state(g1v, g1b, rl1, L, K1, sp, NQS);
    chain_bias_act(g1v, g1b, c1s, L, a.ract);
    __builtin_amdgcn_sched_barrier(0);
    // -- reward layer 2 and the scalar head: a per-lane dot over the h2 registers, then one add across the lane halves
    float dot = 0.f;
#pragma unroll
    for (int ob = 0; ob < RB; ++ob) {
      if (ob < g2b) {
        const f32x16 acc = chain_dense<RB, (RB > 2)>(V2s, T2, ob, L, g1v, g1b);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int u = 32 * ob + unit_of(r, hi);
          dot = fmaf(dyn_act(acc[r] + c2s[u], a.ract), w3s[u], dot);
        }
      }
    }
    dot += __shfl_xor(dot, 32);
    const float z = (dot + hd[0]) * hd[1] + hd[2];     // out * (out_scale + 1e-8) + out_shift (nn_dynamics.py:327)
    if (valid && hi == 0) {
      if (a.r32) a.r32[(int64_t)k * a.rows + row] = z;
      if (a.r64) a.r64[(int64_t)k * a.rows + row] = (double)z;
    }
  }
}

// ---- the generic route's pieces.  X1 (K x rows x (n + m)) = [s, a] and the same columns of X2 (K x rows x (2 n + m)) ...
__global__ void k_pr_gather_sa(const float* __restrict__ obs, const float* __restrict__ actions, int64_t act_stride, int64_t rows, int K, int n,
                               int m, float* __restrict__ X1, float* __restrict__ X2) {
  const int din = n + m, rin = din + n;
  const int64_t total = (int64_t)K * rows * din;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kr = e / din; const int c = (int)(e - kr * din);
    const int64_t k = kr / rows, r = kr - k * rows;
    const float v = c < n ? obs[kr * n + c] : actions[k * act_stride + r * m + (c - n)];
    X1[e] = v;
    X2[kr * rin + c] = v;
  }
}
// ... then s' (K x rows x n, the first k_dyn_forward's output) into X2's last n columns
__global__ void k_pr_gather_sp(const float* __restrict__ sp, int64_t krows, int n, int m, float* __restrict__ X2) {
  const int rin = 2 * n + m;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < krows * n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kr = e / n; const int c = (int)(e - kr * n);
    X2[kr * rin + n + m + c] = sp[e];
  }
}
__global__ void k_pr_widen(const float* __restrict__ r32, int64_t count, double* __restrict__ r64) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) r64[e] = (double)r32[e];
}

}  // namespace mjx
