// plan.h -- MPC planning on learned-model ensembles (mjrl/algos/model_accel/model_learning_mpc.py, MPCPolicy.get_action):
//
//   k_plan_rollout<HB, NB>  register-resident rollout of GIVEN action sequences through all K members in one launch
//                           (trajectory_rollout, sampling.py:96-123, called once per member by model_learning_mpc.py:53-56).
//                           Grid (tile groups, K), 256 threads: a workgroup belongs to one member, each of its four waves owns one
//                           tile of 32 trajectories and carries it through all H steps in registers.
//   k_plan_tile_s0          one state -> N rows (np.tile, sampling.py:108-109), for the generic route
//   k_plan_disagree / k_plan_returns / k_plan_softmax / k_plan_sequence
//                           scoring and weighting in fp64 with fixed summation orders (score_trajectory_ensemble
//                           model_learning_mpc.py:85-99, score_trajectory :101-110, the softmax weighting :70-74)
//
// The rollout is a register-chained MFMA MLP (mfma_chain.h: the scheme, the dynamics net's LDS image and the pieces of a forward).
// A rollout adds one observation: the OUTPUT layer's accumulator -- the next state -- is the layer-1 B operand of the NEXT time
// step, so the tail of a forward writes the state registers in place.  The action part of the layer-1 operand is read by each lane
// for its own trajectory and its own four k-slots, one step ahead of its use.  There is no barrier inside the time loop, and the
// kernel has no static LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_chain.h"

namespace mjx {

enum { PLAN_IDX_REFERENCE = 0, PLAN_IDX_TRAJECTORY = 1 };

struct PlanArgs {
  const float* s0; int64_t s0_stride;   // 0: one state for every trajectory, n: N x n
  const float* actions;                 // N x H x m
  const float* P; const float* tr;      // K x Pstride, K x (2 (n + m) + 2 n)
  float* obs;                           // K x N x H x n
  int64_t N, Pstride;
  int H, n, m, h1, h2, act, flags;
};

template <int HB, int NB>
__global__ __launch_bounds__(256, 1) void k_plan_rollout(PlanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pls[];
  const int n = a.n, m = a.m, din = n + m;
  DynImage<HB, NB> im;
  im.carve(pls, n, m);
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const ChainLane L{j, hi};
  const int k = blockIdx.y;
  im.stage(a.P + k * a.Pstride, a.tr + (int64_t)k * (2 * din + 2 * n), a.h1, a.h2, tid);
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
  const float* __restrict__ arow = a.actions + vrow * a.H * (int64_t)m;
  float* __restrict__ orow = a.obs + ((int64_t)k * a.N + vrow) * a.H * (int64_t)n;
  // this lane's action slots of step t: slot (q, tt) is action 8 q + 4 hi + tt
  float an[PLAN_MAX_M8 / 2];
#pragma unroll
  for (int q = 0; q < PLAN_MAX_M8 / 8; ++q)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int f = 8 * q + 4 * hi + tt;
      an[4 * q + tt] = (q < NQA && f < m) ? arow[f] : 0.f;
    }
  for (int t = 0; t < a.H; ++t) {
    // 1. observations[:, t] is the state BEFORE step t
    if (valid) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const int f = 32 * b + unit_of(r, hi); if (f < n) orow[(int64_t)t * n + f] = s[b][r]; }
    }
    // 2, 3. normalise, layer 1: the action part first (its operands were loaded a step ago), then the state part
    f32x16 h1v[HB];
#pragma unroll
    for (int mb = 0; mb < HB; ++mb) h1v[mb] = (f32x16)(0.f);
    chain_l1_actions(h1v, HB, im.l1(), L, im.n8, an, NQA);
    if (t + 1 < a.H) {                                // the next step's actions: in flight under the rest of this step
#pragma unroll
      for (int q = 0; q < PLAN_MAX_M8 / 8; ++q)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int f = 8 * q + 4 * hi + tt;
          if (q < NQA && f < m) an[4 * q + tt] = arow[(int64_t)(t + 1) * m + f];
        }
    }
    chain_l1_state(h1v, HB, im.l1(), L, 0, s, NQS);
    // the rest of the forward and 4.: the result is the next step's layer-1 operand
    im.tail(L, h1v, s, s, a.act, a.flags);
  }
}

__global__ void k_plan_tile_s0(const float* __restrict__ s0, int64_t N, int n, float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N * n; e += (int64_t)gridDim.x * blockDim.x) out[e] = s0[e % n];
}

// ---- scoring.  Every sum has one fixed order: a thread's strided partial sum in index order, then the xor tree over the lanes of
// its wave, then the waves in order.
__device__ __forceinline__ double plan_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double plan_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o); v = w > v ? w : v; }
  return v;
}

// dis[i] = sum over (t, j) of the population standard deviation over the K members of obs[:, i, t, j] (np.std(predictions,
// axis=0) summed over axes (1, 2), model_learning_mpc.py:90-92).  One wave per trajectory; grid = trajectories needed.
__global__ __launch_bounds__(64) void k_plan_disagree(const float* __restrict__ obs, int K, int64_t N, int64_t HN, double* __restrict__ dis) {
  const int64_t i = blockIdx.x;
  double part = 0.0;
  for (int64_t e = threadIdx.x; e < HN; e += 64) {
    double mean = 0.0;
    for (int k = 0; k < K; ++k) mean += (double)obs[((int64_t)k * N + i) * HN + e];
    mean /= (double)K;
    double var = 0.0;
    for (int k = 0; k < K; ++k) { const double d = (double)obs[((int64_t)k * N + i) * HN + e] - mean; var += d * d; }
    part += sqrt(var / (double)K);
  }
  part = plan_wave_sum(part);
  if (threadIdx.x == 0) dis[i] = part;
}

// R[k N + i] = omega * dis[idx] + sum_t gamma^t r[k, i, t] in the reference's order (:93-98): idx = (k N + i) / N = k as the
// reference writes it, or i (PLAN_IDX_TRAJECTORY).  One thread per score.
__global__ void k_plan_returns(const double* __restrict__ rew, const double* __restrict__ dis, int K, int64_t N, int H, double gamma,
                               double omega, int idx_mode, double* __restrict__ R) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * N) return;
  const int64_t k = e / N, i = e - k * N;
  double sc = dis ? omega * dis[idx_mode == PLAN_IDX_TRAJECTORY ? i : k] : 0.0;      // (dis null: score_trajectory)
  for (int t = 0; t < H; ++t) sc += pow(gamma, (double)t) * rew[e * H + t];
  R[e] = sc;
}

// S = exp(kappa (R - max R)) and sum S (:70, :74).  One workgroup of 1024.
__global__ __launch_bounds__(1024) void k_plan_softmax(const double* __restrict__ R, int64_t T, double kappa, double* __restrict__ S,
                                                       double* __restrict__ sumS) {
  __shared__ double red[16];
  __shared__ double bc;
  const int tid = threadIdx.x;
  double mx = -INFINITY;
  for (int64_t e = tid; e < T; e += 1024) { const double v = R[e]; mx = v > mx ? v : mx; }
  mx = plan_wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) { double v = red[0]; for (int w = 1; w < 16; ++w) v = red[w] > v ? red[w] : v; bc = v; }
  __syncthreads();
  mx = bc;
  double part = 0.0;
  for (int64_t e = tid; e < T; e += 1024) { const double v = exp(kappa * (R[e] - mx)); S[e] = v; part += v; }
  part = plan_wave_sum(part);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) { double v = 0.0; for (int w = 0; w < 16; ++w) v += red[w]; sumS[0] = v; }
}

// seq[e] = sum_i (sum_k S[k N + i]) a[i][e] / (sum S + 1e-6) for e < H m (:71-74: the K members share the action sequences).
// One workgroup of 256 per element.
__global__ __launch_bounds__(256) void k_plan_sequence(const double* __restrict__ S, const double* __restrict__ sumS,
                                                       const double* __restrict__ act, int K, int64_t N, int64_t HM, double* __restrict__ seq) {
  __shared__ double red[4];
  const int64_t e = blockIdx.x;
  const int tid = threadIdx.x;
  double part = 0.0;
  for (int64_t i = tid; i < N; i += 256) {
    double w = 0.0;
    for (int k = 0; k < K; ++k) w += S[(int64_t)k * N + i];
    part += w * act[i * HM + e];
  }
  part = plan_wave_sum(part);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) seq[e] = (((red[0] + red[1]) + red[2]) + red[3]) / (sumS[0] + 1e-6);
}

}  // namespace mjx
