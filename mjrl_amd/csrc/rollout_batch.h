// rollout_batch.h -- model rollouts that stay on the device between the rollout and ingestion (ModelAccelNPG.train_step's resident
// route, model_accel_npg.py:137-155): the ensemble-disagreement error of STORED rollouts, and the truncated, ragged batch packed
// from them.
//
//   k_rollout_disagree<HB, NB>  member k's per-row error mean_c (obs[p][t + 1][c] - f_k(obs[p][t], act[p][t])[c])^2 over the
//                               P x H stored rows of all members' rollouts back to back, f_k unclamped.  Grid (workgroups, K), 256
//                               threads: a workgroup belongs to one member, stages its net into LDS once and each of its four waves
//                               walks tiles of 32 stored rows (a grid-stride loop over tiles).  The first half of k_path_rewards
//                               (path_reward.h): DynImage staging, chain_l1_actions, chain_l1_state, tail; then s' is left in the
//                               output accumulators, and each lane subtracts its row's next stored state from its units.  The last
//                               row of a path (t = H - 1) is computed and never stored.
//   k_rd_max                    err[i] = max over k, in member order, of the per-member means in scratch; a NaN member makes the row
//                               NaN (np.maximum).  No float atomics: the bits are fixed.
//   k_rd_gather / k_rd_reduce   the generic route: [s, a] rows of t < H - 1 gathered for k_dyn_forward, then k_dyn_pred_err's
//                               arithmetic (fp32 difference and square, fp64 sum over c in index order, / n, cast to fp32)
//   k_rp_first / k_rp_scan / k_rp_rows
//                               the truncation decision per path, the exclusive prefix sum of the kept lengths (one workgroup that
//                               walks the paths 1024 at a time with a carry: any P), and the copy of the kept rows.  Pure data
//                               movement in plain HIP: no atomics, every output exact.
//
// Summation order of route 1's mean: a lane holds the units 32 b + unit_of(r, hi) of its row (b = 0 .. NB - 1, r = 0 .. 15).  It adds
// d * d (fp32, d = next - s') for its units c < n with fmaf, in (b, r) order, from 0; the two lane halves' sums are added once
// (lo + hi); the sum is divided by (float)n.  Padded units (c >= n) take no part.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_chain.h"

namespace mjx {

struct RollDisArgs {
  const float* obs; const float* act;   // P H x n, P H x m: stored rows, path after path
  const float* dP; const float* dtr;    // K x dPstride, K x (2 (n + m) + 2 n)
  float* mk;                            // K x P (H - 1): member k's per-row means
  int64_t rows, dPstride;               // rows = P H
  int H, n, m, h1, h2, dact, flags;
};

template <int HB, int NB>
__global__ __launch_bounds__(256, 1) void k_rollout_disagree(RollDisArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rds[];
  const int n = a.n, m = a.m, din = n + m, H = a.H;
  DynImage<HB, NB> im;
  im.carve(rds, n, m);
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const ChainLane L{j, hi};
  const int k = blockIdx.y;
  im.stage(a.dP + k * a.dPstride, a.dtr + (int64_t)k * (2 * din + 2 * n), a.h1, a.h2, tid);
  __syncthreads();
  const int NQS = im.n8 / 8, NQA = im.m8 / 8;
  const int64_t P = a.rows / H, R = P * (H - 1);
  const float fn = (float)n;
  // ---- the tiles of this wave (no barrier from here on)
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile * 32 < a.rows; tile += (int64_t)gridDim.x * 4) {
    const int64_t row = tile * 32 + j;
    const bool valid = row < a.rows;
    const int64_t vrow = valid ? row : 0;
    const int64_t p = vrow / H; const int t = (int)(vrow - p * H);
    const bool keep = valid && t < H - 1;
    const int64_t nrow = keep ? vrow + 1 : vrow;          // (the last row of a path has no next stored state: never stored)
    f32x16 s[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = 32 * b + unit_of(r, hi);
        const float v = a.obs[vrow * n + (f < n ? f : 0)];
        s[b][r] = (valid && f < n) ? v : 0.f;
      }
    float an[PLAN_MAX_M8 / 2];
#pragma unroll
    for (int q = 0; q < PLAN_MAX_M8 / 8; ++q)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int f = 8 * q + 4 * hi + tt;
        const float v = a.act[vrow * m + ((q < NQA && f < m) ? f : 0)];
        an[4 * q + tt] = (valid && q < NQA && f < m) ? v : 0.f;
      }
    f32x16 h1v[HB];
#pragma unroll
    for (int mb = 0; mb < HB; ++mb) h1v[mb] = (f32x16)(0.f);
    chain_l1_actions(h1v, HB, im.l1(), L, im.n8, an, NQA);
    chain_l1_state(h1v, HB, im.l1(), L, 0, s, NQS);
    f32x16 sp[NB];
    im.tail(L, h1v, s, sp, a.dact, a.flags);
    // -- this lane's units against the next stored state
    float acc = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = 32 * b + unit_of(r, hi);
        const float nx = a.obs[nrow * n + (f < n ? f : 0)];
        const float d = nx - sp[b][r];
        if (f < n) acc = fmaf(d, d, acc);
      }
    acc += __shfl_xor(acc, 32);
    if (keep && hi == 0) a.mk[(int64_t)k * R + p * (H - 1) + t] = acc / fn;
  }
}

// np.maximum over the members in order: a NaN member makes the row NaN (fmaxf would drop it), as k_dyn_pred_err does
__global__ void k_rd_max(const float* __restrict__ mk, int K, int64_t R, float* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R; i += (int64_t)gridDim.x * blockDim.x) {
    float e = 0.f;
    for (int k = 0; k < K; ++k) {
      const float v = mk[(int64_t)k * R + i];
      if (k == 0 || v > e || v != v) e = v;
    }
    err[i] = e;
  }
}

// ---- the generic route's pieces.  X (P (H - 1) x (n + m)) = [s, a] of the rows with a next stored state ...
__global__ void k_rd_gather(const float* __restrict__ obs, const float* __restrict__ act, int64_t R, int H, int n, int m, float* __restrict__ X) {
  const int din = n + m;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < R * din; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / din; const int c = (int)(e - i * din);
    const int64_t p = i / (H - 1), src = p * H + (i - p * (H - 1));
    X[e] = c < n ? obs[src * n + c] : act[src * m + (c - n)];
  }
}
// ... and k_dyn_pred_err's arithmetic on pred (K x R x n) against the next stored states
__global__ void k_rd_reduce(const float* __restrict__ pred, const float* __restrict__ obs, int K, int64_t R, int H, int n, float* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / (H - 1);
    const float* __restrict__ nx = obs + (p * H + (i - p * (H - 1)) + 1) * n;
    float e = 0.f;
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
      for (int c = 0; c < n; ++c) { const float d = nx[c] - pred[((int64_t)k * R + i) * n + c]; s += (double)(d * d); }
      const float v = (float)(s / n);
      if (k == 0 || v > e || v != v) e = v;
    }
    err[i] = e;
  }
}

// ---- truncate and pack.  Per path: v = the first t < H - 1 with (double)err > lim (NaN never counts; no err: none), the kept
// length T = H, or min(H, max(min_len, v + 1)); T goes to off[p + 1], which k_rp_scan then sums in place.
__global__ void k_rp_first(const float* __restrict__ err, int64_t P, int H, double lim, int min_len, int64_t* __restrict__ off,
                           int32_t* __restrict__ first, uint8_t* __restrict__ term) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
    int v = -1;
    if (err)
      for (int t = 0; t < H - 1; ++t)
        if ((double)err[p * (H - 1) + t] > lim) { v = t; break; }
    int T = H;
    if (v >= 0) { T = v + 1 > min_len ? v + 1 : min_len; T = T < H ? T : H; }
    off[p + 1] = T;
    first[p] = v;
    term[p] = (uint8_t)(T != H);
  }
}
// one workgroup of 1024 threads: off[0] = 0, off[p + 1] = sum of the lengths up to p, 1024 paths at a time with a carry
__global__ __launch_bounds__(1024) void k_rp_scan(int64_t P, int64_t* __restrict__ off) {
  __shared__ int64_t buf[2][1024];
  __shared__ int64_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) { carry = 0; off[0] = 0; }
  __syncthreads();
  for (int64_t base = 0; base < P; base += 1024) {
    const int64_t p = base + tid;
    int cur = 0;
    buf[0][tid] = p < P ? off[p + 1] : 0;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      buf[cur ^ 1][tid] = buf[cur][tid] + (tid >= d ? buf[cur][tid - d] : 0);
      cur ^= 1;
      __syncthreads();
    }
    const int64_t c = carry;
    if (p < P) off[p + 1] = c + buf[cur][tid];
    __syncthreads();
    if (tid == 1023) carry = c + buf[cur][1023];
    __syncthreads();
  }
}

struct RollPackArgs {
  const float* obs; const float* act; const float* rew32; const double* rew64;
  const int64_t* off; const int32_t* first;
  float* obs_out; float* act_out; double* rew_out; double* obs64_out; int32_t* tpos_out;
  int64_t P; int H, n, m; double truncate_reward;
};
// element e of the P H x (n + m + 1) grid: column c of stored row (p, t); kept rows go to packed row off[p] + t.  The last column
// carries the reward and the time index.
__global__ void k_rp_rows(RollPackArgs a) {
  const int n = a.n, m = a.m, W = n + m + 1, H = a.H;
  const int64_t total = a.P * H * W;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ph = e / W; const int c = (int)(e - ph * W);
    const int64_t p = ph / H; const int t = (int)(ph - p * H);
    const int64_t o = a.off[p], T = a.off[p + 1] - o;
    if (t >= T) continue;
    const int64_t row = o + t;
    if (c < n) {
      const float v = a.obs[ph * n + c];
      a.obs_out[row * n + c] = v;
      if (a.obs64_out) a.obs64_out[row * n + c] = (double)v;
    } else if (c < n + m) {
      a.act_out[row * m + (c - n)] = a.act[ph * m + (c - n)];
    } else {
      const bool bump = a.first[p] >= 0 && t == T - 1;
      double r;
      if (a.rew32) { r = (double)a.rew32[ph]; if (bump) r = (double)(float)(r + a.truncate_reward); }
      else { r = a.rew64[ph]; if (bump) r = r + a.truncate_reward; }
      a.rew_out[row] = r;
      if (a.tpos_out) a.tpos_out[row] = t;
    }
  }
}

}  // namespace mjx
