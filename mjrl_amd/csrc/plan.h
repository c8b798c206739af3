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
// The rollout uses the scheme of k_mlp_predict128 (baseline.h) and the fused policy kernels: units on the MFMA M / K dimensions,
// the tile's 32 trajectories on N, so the v_mfma_f32_32x32x2_f32 accumulator of layer l is the B operand of layer l + 1 as it
// lies (register r = 4 q + t of lane half `hi` holds unit 8 q + 4 hi + t, unit_of).  A rollout adds one observation: the OUTPUT
// layer's accumulator -- the next state -- is the layer-1 B operand of the NEXT time step.  No activation passes through LDS and
// there is no barrier inside the time loop.
//
// Input features are laid out [state padded to n8 = a multiple of 8 | action padded to m8 = a multiple of 8]; W1's columns are
// permuted and zero-padded to that layout when they are staged.  The state part of the layer-1 operand is the state accumulator
// itself; the action part is read by each lane for its own trajectory and its own four k-slots, one step ahead of its use.
// Hidden widths are padded to HW = 32 HB units with zero weights and biases: a padded unit is act(0) = 0 (ReLU and tanh) and
// meets zero columns downstream.  State blocks beyond n are kept at exactly 0 (zero rows of W_out, zero bias / scale / shift / mask).
//
// LDS image (floats, row strides + 4 as in k_mlp_predict128; the kernel has no static LDS):
//   W1s HW x (K1 + 4) | W2s HW x (HW + 4) | W3s 32 NB x (HW + 4) | b1 HW | b2 HW | b3 32 NB | in_shift K1 | in_scale + 1e-8 K1 |
//   out_scale + 1e-8, out_shift, mask: 32 NB each                 -- 128 x 128 at n = 64, m = 32: 155.4 KiB of the 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dynamics.h"
#include "fused_policy.h"

namespace mjx {

constexpr int PLAN_MAX_M8 = 32;       // action slots a lane keeps one step ahead: 4 k-steps x 4
enum { PLAN_IDX_REFERENCE = 0, PLAN_IDX_TRAJECTORY = 1 };

struct PlanArgs {
  const float* s0; int64_t s0_stride;   // 0: one state for every trajectory, n: N x n
  const float* actions;                 // N x H x m
  const float* P; const float* tr;      // K x Pstride, K x (2 (n + m) + 2 n)
  float* obs;                           // K x N x H x n
  int64_t N, Pstride;
  int H, n, m, h1, h2, act, flags;
};

__host__ __device__ inline int plan_pad8(int v) { return (v + 7) & ~7; }
__host__ __device__ inline size_t plan_lds_floats(int HB, int NB, int n, int m) {
  const size_t HW = 32 * (size_t)HB, K1 = (size_t)plan_pad8(n) + plan_pad8(m);
  return HW * (K1 + 4) + HW * (HW + 4) + 32 * NB * (HW + 4) + 2 * HW + 32 * NB + 2 * K1 + 3 * 32 * NB;
}

template <int HB, int NB>
__global__ __launch_bounds__(256, 1) void k_plan_rollout(PlanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pls[];
  constexpr int HW = 32 * HB, S2 = HW + 4, NS = 32 * NB;
  const int n = a.n, m = a.m, h1 = a.h1, h2 = a.h2, n8 = plan_pad8(n), m8 = plan_pad8(m), K1 = n8 + m8, S1 = K1 + 4, din = n + m;
  float* W1s = pls; float* W2s = W1s + HW * S1; float* W3s = W2s + HW * S2;
  float* b1s = W3s + NS * S2; float* b2s = b1s + HW; float* b3s = b2s + HW;
  float* ish = b3s + NS; float* irs = ish + K1; float* osc = irs + K1; float* osh = osc + NS; float* msk = osh + NS;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = blockIdx.y;
  const float* __restrict__ P = a.P + k * a.Pstride;
  const float* __restrict__ tr = a.tr + (int64_t)k * (2 * din + 2 * n);
  const int64_t oB1 = (int64_t)h1 * din, oW2 = oB1 + h1, oB2 = oW2 + (int64_t)h2 * h1, oW3 = oB2 + h2, oB3 = oW3 + (int64_t)n * h2;
  // ---- prologue: a wave stages whole rows (lanes along the row: coalesced reads, no division)
  for (int u = tid >> 6; u < HW; u += 4) {
    for (int c = lane; c < K1; c += 64) {
      const int f = c < n8 ? (c < n ? c : -1) : (c - n8 < m ? n + c - n8 : -1);
      W1s[u * S1 + c] = (u < h1 && f >= 0) ? P[(int64_t)u * din + f] : 0.f;
    }
    for (int c = lane; c < HW; c += 64) W2s[u * S2 + c] = (u < h2 && c < h1) ? P[oW2 + (int64_t)u * h1 + c] : 0.f;
  }
  for (int u = tid >> 6; u < NS; u += 4)
    for (int c = lane; c < HW; c += 64) W3s[u * S2 + c] = (u < n && c < h2) ? P[oW3 + (int64_t)u * h2 + c] : 0.f;
  for (int i = tid; i < HW; i += 256) { b1s[i] = i < h1 ? P[oB1 + i] : 0.f; b2s[i] = i < h2 ? P[oB2 + i] : 0.f; }
  for (int i = tid; i < NS; i += 256) {
    const float sc = i < n ? tr[2 * din + n + i] : 0.f;
    b3s[i] = i < n ? P[oB3 + i] : 0.f;
    osc[i] = i < n ? sc + 1e-8f : 0.f;
    osh[i] = i < n ? tr[2 * din + i] : 0.f;
    msk[i] = (i < n && sc >= 1e-8f) ? 1.f : 0.f;
  }
  for (int c = tid; c < K1; c += 256) {
    const int f = c < n8 ? (c < n ? c : -1) : (c - n8 < m ? n + c - n8 : -1);
    ish[c] = f >= 0 ? tr[f] : 0.f;
    irs[c] = f >= 0 ? tr[din + f] + 1e-8f : 1.f;
  }
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
  const int NQS = n8 / 8, NQA = m8 / 8;
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
#pragma unroll
    for (int q = 0; q < PLAN_MAX_M8 / 8; ++q) {
      if (q < NQA) {
        const int c0 = n8 + 8 * q + 4 * hi;
        float xb[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) xb[tt] = (an[4 * q + tt] - ish[c0 + tt]) / irs[c0 + tt];
#pragma unroll
        for (int mb = 0; mb < HB; ++mb) {
          const f32x4 a4 = *(const f32x4*)&W1s[(32 * mb + j) * S1 + c0];
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) h1v[mb] = MJX_MFMA(a4[tt], xb[tt], h1v[mb]);
        }
      }
    }
    if (t + 1 < a.H) {                                // the next step's actions: in flight under the rest of this step
#pragma unroll
      for (int q = 0; q < PLAN_MAX_M8 / 8; ++q)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int f = 8 * q + 4 * hi + tt;
          if (q < NQA && f < m) an[4 * q + tt] = arow[(int64_t)(t + 1) * m + f];
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (4 * b + q < NQS) {
          const int c0 = 32 * b + 8 * q + 4 * hi;
          float xb[4];
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) xb[tt] = (s[b][4 * q + tt] - ish[c0 + tt]) / irs[c0 + tt];
#pragma unroll
          for (int mb = 0; mb < HB; ++mb) {
            const f32x4 a4 = *(const f32x4*)&W1s[(32 * mb + j) * S1 + c0];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) h1v[mb] = MJX_MFMA(a4[tt], xb[tt], h1v[mb]);
          }
        }
      }
#pragma unroll
    for (int mb = 0; mb < HB; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) h1v[mb][r] = dyn_act(h1v[mb][r] + b1s[32 * mb + unit_of(r, hi)], a.act);
    // layer 2: register r of h1v[mb] holds unit 32 mb + unit_of(r, hi) -- the B operand of k-step (mb, r) as it lies
    f32x16 h2v[HB];
#pragma unroll
    for (int ob = 0; ob < HB; ++ob) {
      f32x16 acc = (f32x16)(0.f);
      const float* wrow = &W2s[(32 * ob + j) * S2 + 4 * hi];
#pragma unroll
      for (int mb = 0; mb < HB; ++mb)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const f32x4 a4 = *(const f32x4*)(wrow + 32 * mb + 8 * rq);
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) acc = MJX_MFMA(a4[tt], h1v[mb][4 * rq + tt], acc);
        }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = dyn_act(acc[r] + b2s[32 * ob + unit_of(r, hi)], a.act);
      h2v[ob] = acc;
    }
    // output layer and 4.: affine, mask, residual as in dyn_net_tile; the result is the next step's layer-1 operand
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      f32x16 acc = (f32x16)(0.f);
      const float* wrow = &W3s[(32 * b + j) * S2 + 4 * hi];
#pragma unroll
      for (int mb = 0; mb < HB; ++mb)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const f32x4 a4 = *(const f32x4*)(wrow + 32 * mb + 8 * rq);
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) acc = MJX_MFMA(a4[tt], h2v[mb][4 * rq + tt], acc);
        }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int u = 32 * b + unit_of(r, hi);
        float z = acc[r] + b3s[u];
        if (a.flags & DYN_OUT_AFFINE) z = z * osc[u] + osh[u];
        if (a.flags & DYN_MASK) z = z * msk[u];
        if (a.flags & DYN_RESIDUAL) z = z + s[b][r];
        s[b][r] = z;
      }
    }
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
