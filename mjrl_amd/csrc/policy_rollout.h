// policy_rollout.h -- the policy acting inside a learned-model rollout, register-resident (policy_rollout, sampling.py:16-89, for K
// members at once: what ModelAccelNPG.get_refined_action runs once per real environment step):
//
//   k_policy_rollout<HB, NB>  mjx_model_rollout's policy mode.  Grid (ceil(N / 128), K), 256 threads: a workgroup belongs to one
//                             member, stages the member's dynamics net AND the policy into LDS once, and each of its four waves
//                             carries one tile of 32 trajectories through all H steps in registers.
//   k_pol_expand_noise        one H x N x m noise block -> K copies, for the generic route
//
// A register-chained MFMA MLP twice per step (mfma_chain.h: the scheme, the dynamics net's LDS image, the policy's image and the
// pieces of a forward).  The policy's layer 1 reads the state accumulators as k_plan_rollout's dynamics layer 1 does; its OUTPUT
// accumulator holds action 8 q + 4 hi + t in register 4 q + t (unit_of), which is exactly the action slot layout chain_l1_actions
// reads: after the affine, the noise and the clamp the 16 registers ARE the dynamics layer-1 action operand.  The dynamics tail
// writes the next state over the state registers.  Nothing passes through LDS, there is one barrier (after staging) and the kernel
// has no static LDS.  The noise is read by each lane for its own row and its own slots, one step ahead of its use.
//
// Per step, in mjx_model_rollout's order: store the state; policy mean = tanh layers over (s - in_shift) / (in_scale + 1e-8), then
// out * out_scale + out_shift (no 1e-8 on the output side, dynamics.h k_model_rollout); + noise * exp(log_std); clamp; store the
// action; the dynamics forward of member k; clamp.  Padded hidden, action (f >= m) and state units stay exactly 0 throughout: zero
// weights, biases, out_scale, out_shift and sigma, and clamp bounds [0, 0].  Absent bounds are staged as -inf / +inf, which
// dyn_clamp passes every value (NaN included) through unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_chain.h"
#include "plan.h"

namespace mjx {

constexpr int POLR_PB = POL_MAX_PB;   // policy hidden blocks an instance keeps registers for

struct PolRollArgs {
  const float* s0; int64_t s0_stride;   // 0: one state for every trajectory, n: N x n
  const float* noise; int64_t noise_k;  // member k reads steps (k * noise_k + t): H (K x H x N x m) or 0 (one H x N x m block); null: eval mode
  const float* pP; const float* ptr;    // the policy's flat vector [W1, b1, W2, b2, W3, b3, log_std] and [in_shift n, in_scale n, out_shift m, out_scale m]
  const float* P; const float* tr;      // dynamics: K x Pstride, K x (2 (n + m) + 2 n)
  const float* a_lo; const float* a_hi; const float* s_lo; const float* s_hi;   // m / n each, null in pairs
  float* obs; float* act_out;           // K x N x H x n, K x N x H x m
  int64_t N, Pstride;
  int H, n, m, h1, h2, act, flags, p1, p2;
};

template <int HB, int NB>
__global__ __launch_bounds__(256, 1) void k_policy_rollout(PolRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) float prl[];
  const int n = a.n, m = a.m, din = n + m;
  DynImage<HB, NB> im;
  PolImage<NB> pi;
  pi.carve(im.carve(prl, n, m), n, m, a.p1, a.p2);
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const ChainLane L{j, hi};
  const int k = blockIdx.y;
  im.stage(a.P + k * a.Pstride, a.tr + (int64_t)k * (2 * din + 2 * n), a.h1, a.h2, tid);
  pi.stage(a.pP, a.ptr, a.a_lo, a.a_hi, a.s_lo, a.s_hi, tid);
  __syncthreads();
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave, row = tile * 32 + j;
  if (tile * 32 >= a.N) return;                       // (after the only barrier)
  const bool valid = row < a.N;
  const int64_t vrow = valid ? row : 0;
  f32x16 s[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * b + unit_of(r, hi);
      const float v = a.s0[vrow * a.s0_stride + (f < n ? f : 0)];
      s[b][r] = (valid && f < n) ? v : 0.f;
    }
  const int NQS = im.n8 / 8, NQA = im.m8 / 8;
  const bool noisy = a.noise != nullptr;
  // noise of step t for this lane's row: slot r = 4 q + tt is action 8 q + 4 hi + tt = unit_of(r, hi)
  const float* __restrict__ zrow = noisy ? a.noise + ((int64_t)k * a.noise_k * a.N + vrow) * m : nullptr;
  const int64_t zstep = a.N * (int64_t)m;
  float* __restrict__ orow = a.obs + ((int64_t)k * a.N + vrow) * a.H * (int64_t)n;
  float* __restrict__ arow = a.act_out + ((int64_t)k * a.N + vrow) * a.H * (int64_t)m;
  float nz[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int f = unit_of(r, hi);
    nz[r] = (noisy && f < m) ? zrow[f] : 0.f;
  }
  for (int t = 0; t < a.H; ++t) {
    // 1. observations[:, t] is the state BEFORE step t
    if (valid) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const int f = 32 * b + unit_of(r, hi); if (f < n) orow[(int64_t)t * n + f] = s[b][r]; }
    }
    // 2. the policy mean: layer 1 over the state accumulators, layer 2, the output block
    float an[PLAN_MAX_M8 / 2];
    {
      f32x16 p1v[POLR_PB];
#pragma unroll
      for (int mb = 0; mb < POLR_PB; ++mb) p1v[mb] = (f32x16)(0.f);
      chain_l1_state(p1v, pi.p1b, pi.l1(), L, 0, s, NQS);
      chain_bias_act(p1v, pi.p1b, pi.d1, L, DYN_ACT_TANH);
      f32x16 p2v[POLR_PB];
#pragma unroll
      for (int ob = 0; ob < POLR_PB; ++ob) {
        p2v[ob] = (f32x16)(0.f);
        if (ob < pi.p2b) {
          p2v[ob] = chain_dense(pi.Q2s, pi.U2, ob, L, p1v, pi.p1b);
          chain_bias_act(p2v[ob], pi.d2 + 32 * ob, L, DYN_ACT_TANH);
        }
      }
      const f32x16 av = chain_dense(pi.Q3s, pi.U3, 0, L, p2v, pi.p2b);
      // 3, 4. out * out_scale + out_shift, + noise * exp(log_std), clamp: the dynamics layer-1 action operand as it lies
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int u = unit_of(r, hi);
        float v = (av[r] + pi.d3[u]) * pi.osc[u] + pi.osh[u];
        if (noisy) v = v + nz[r] * pi.sig[u];
        an[r] = dyn_clamp(v, pi.alo[u], pi.ahi[u]);
      }
    }
    if (noisy && t + 1 < a.H) {                       // the next step's noise: in flight under the dynamics forward
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = unit_of(r, hi);
        if (f < m) nz[r] = zrow[(int64_t)(t + 1) * zstep + f];
      }
    }
    // 5. actions[:, t]
    if (valid) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { const int f = unit_of(r, hi); if (f < m) arow[(int64_t)t * m + f] = an[r]; }
    }
    // 6. the dynamics forward of member k: the next state over the state registers
    f32x16 h1v[HB];
#pragma unroll
    for (int mb = 0; mb < HB; ++mb) h1v[mb] = (f32x16)(0.f);
    chain_l1_actions(h1v, HB, im.l1(), L, im.n8, an, NQA);
    chain_l1_state(h1v, HB, im.l1(), L, 0, s, NQS);
    im.tail(L, h1v, s, s, a.act, a.flags);
    // 7. clamp the state
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) { const int u = 32 * b + unit_of(r, hi); s[b][r] = dyn_clamp(s[b][r], pi.slo[u], pi.shi[u]); }
  }
}

// out[k] = in for k < K (count elements each)
__global__ void k_pol_expand_noise(const float* __restrict__ in, int64_t count, int K, float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count * K; e += (int64_t)gridDim.x * blockDim.x) out[e] = in[e % count];
}

}  // namespace mjx
