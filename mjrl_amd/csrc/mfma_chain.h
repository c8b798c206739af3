// mfma_chain.h -- the shared pieces of the kernels that run a small MLP on v_mfma_f32_32x32x2_f32 with the activations kept in
// registers: k_mlp_predict128 (baseline.h), k_plan_rollout (plan.h) and k_path_rewards (path_reward.h).
//
// The scheme: units on the MFMA M / K dimensions, a tile's 32 rows on N, so the accumulator of layer l is the B operand of layer
// l + 1 as it lies (register r = 4 q + t of lane half `hi` holds unit 8 q + 4 hi + t, unit_of).  Weights come from a padded LDS
// image with row strides + 4, one f32x4 (ds_read_b128) per four k-steps in the k-permuted order (k-slot `hi` of step (q, t) carries
// k = 8 q + 4 hi + t).  No activation passes through LDS.  Hidden widths are padded to whole 32-blocks with zero weights and
// biases: a padded unit is act(0) = 0 (ReLU and tanh) and meets zero columns downstream.
//
// A first layer's input features are laid out in padded columns [s to n8 | a to m8 | s' to n8] (n8, m8 multiples of 8; the dynamics
// net ends after a); W1's columns are permuted and zero-padded to that layout when they are staged (DynImage::feat).  The state
// part of a layer-1 operand is a state accumulator itself; the action part is read by each lane for its own row and k-slots.
//
// Every piece is forceinline and keeps the operation order of the loops it replaced: a kernel's sums are the same fmaf chains.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dynamics.h"
#include "mfma_prims.h"

namespace mjx {

constexpr int PLAN_MAX_M8 = 32;       // action slots a lane keeps: 4 k-steps x 4

struct ChainLane { int j, hi; };      // lane = 32 hi + j: row j of the tile, lane half hi
// a first layer in LDS: W rows x S (S = padded columns + 4); per padded column the input shift and scale + 1e-8 (1 where padded)
struct ChainL1 { const float* W; int S; const float* shift; const float* rscale; };

// ---- 1. one dense 32-unit output block ob of W (rows x S) from register blocks: register r of h[mb] holds unit
// 32 mb + unit_of(r, hi), the B operand of k-step (mb, r) as it lies.  kbs <= KB blocks are in use.  FENCE: weight loads are
// not hoisted further ahead than two quads (registers).
template <int KB, bool FENCE = false>
__device__ __forceinline__ f32x16 chain_dense(const float* W, int S, int ob, ChainLane L, const f32x16 (&h)[KB], int kbs) {
  f32x16 acc = (f32x16)(0.f);
  const float* wrow = &W[(32 * ob + L.j) * S + 4 * L.hi];
#pragma unroll
  for (int mb = 0; mb < KB; ++mb) {
    if (mb < kbs) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const f32x4 a4 = *(const f32x4*)(wrow + 32 * mb + 8 * rq);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc = MJX_MFMA(a4[tt], h[mb][4 * rq + tt], acc);
        if (FENCE && (rq & 1)) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  return acc;
}

// ---- 2. four k-steps of a first layer: inputs x[i0 .. i0 + 3] at padded columns c0 .. c0 + 3 (c0 includes this half's 4 hi),
// normalised, into the mbs blocks in use
template <int MB, class X>
__device__ __forceinline__ void chain_l1_quad(f32x16 (&h)[MB], int mbs, ChainL1 w, ChainLane L, int c0, const X& x, int i0) {
  float xb[4];
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) xb[tt] = (x[i0 + tt] - w.shift[c0 + tt]) / w.rscale[c0 + tt];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if (mb < mbs) {
      const f32x4 a4 = *(const f32x4*)&w.W[(32 * mb + L.j) * w.S + c0];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) h[mb] = MJX_MFMA(a4[tt], xb[tt], h[mb]);
    }
  }
}
// ... over a lane's action slots (slot (q, tt) is action 8 q + 4 hi + tt), the action part starting at column c_a
template <int MB>
__device__ __forceinline__ void chain_l1_actions(f32x16 (&h)[MB], int mbs, ChainL1 w, ChainLane L, int c_a, const float (&an)[PLAN_MAX_M8 / 2], int NQA) {
#pragma unroll
  for (int q = 0; q < PLAN_MAX_M8 / 8; ++q)
    if (q < NQA) chain_l1_quad(h, mbs, w, L, c_a + 8 * q + 4 * L.hi, an, 4 * q);
}
// ... and over state accumulators, the state part starting at column c_s
template <int MB, int NB>
__device__ __forceinline__ void chain_l1_state(f32x16 (&h)[MB], int mbs, ChainL1 w, ChainLane L, int c_s, const f32x16 (&s)[NB], int NQS) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (4 * b + q < NQS) chain_l1_quad(h, mbs, w, L, c_s + 32 * b + 8 * q + 4 * L.hi, s[b], 4 * q);
}

// ---- 3. bias + activation: one block (bias points at its 32 units), and the mbs blocks in use (a block beyond stays exactly 0
// and is never read)
__device__ __forceinline__ void chain_bias_act(f32x16& v, const float* bias, ChainLane L, int act) {
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = dyn_act(v[r] + bias[unit_of(r, L.hi)], act);
}
template <int MB>
__device__ __forceinline__ void chain_bias_act(f32x16 (&h)[MB], int mbs, const float* bias, ChainLane L, int act) {
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
    if (mb < mbs) chain_bias_act(h[mb], bias + 32 * mb, L, act);
}

// ---- 4. the dynamics net [n + m, h1, h2, n] of one ensemble member in LDS, hidden widths padded to HW = 32 HB, the output to
// NS = 32 NB (state blocks beyond n are kept at exactly 0: zero rows of W_out, zero bias / scale / shift / mask).  In floats:
//   W1s HW x (K1 + 4) | W2s HW x (HW + 4) | W3s NS x (HW + 4) | b1 HW | b2 HW | b3 NS | in_shift K1 | in_scale + 1e-8 K1 |
//   out_scale + 1e-8, out_shift, mask: NS each                    -- 128 x 128 at n = 64, m = 32: 155.4 KiB of the 160 KiB.
// plan_lds_floats sums these terms in carve()'s order: carve(base) - base == plan_lds_floats for the same (HB, NB, n, m).
__host__ __device__ inline size_t plan_lds_floats(int HB, int NB, int n, int m) {
  const size_t HW = 32 * (size_t)HB, K1 = (size_t)pad8(n) + pad8(m);
  return HW * (K1 + 4) + HW * (HW + 4) + 32 * NB * (HW + 4) + 2 * HW + 32 * NB + 2 * K1 + 3 * 32 * NB;
}

template <int HB, int NB>
struct DynImage {
  static constexpr int HW = 32 * HB, S2 = HW + 4, NS = 32 * NB;
  float *W1s, *W2s, *W3s, *b1s, *b2s, *b3s, *ish, *irs, *osc, *osh, *msk;
  int n, m, n8, m8, K1, S1, din;

  __device__ __forceinline__ float* carve(float* base, int n_, int m_) {      // returns the end: where a second image may follow
    n = n_; m = m_; n8 = pad8(n); m8 = pad8(m); K1 = n8 + m8; S1 = K1 + 4; din = n + m;
    W1s = base; W2s = W1s + HW * S1; W3s = W2s + HW * S2;
    b1s = W3s + NS * S2; b2s = b1s + HW; b3s = b2s + HW;
    ish = b3s + NS; irs = ish + K1; osc = irs + K1; osh = osc + NS; msk = osh + NS;
    return msk + NS;
  }
  __device__ __forceinline__ ChainL1 l1() const { return ChainL1{W1s, S1, ish, irs}; }
  // padded column c of [s | a | s'] -> input feature of [s, a, s'], or -1 for padding
  __device__ __forceinline__ int feat(int c) const {
    return c < n8 ? (c < n ? c : -1) : c < K1 ? (c - n8 < m ? n + c - n8 : -1) : (c - K1 < n ? din + c - K1 : -1);
  }
  // all 256 threads, before the barrier: a wave stages whole rows (lanes along the row: coalesced reads, no division).
  // P = the member's parameters, tr = its transforms (2 (n + m) + 2 n)
  __device__ __forceinline__ void stage(const float* __restrict__ P, const float* __restrict__ tr, int h1, int h2, int tid) const {
    const int lane = tid & 63;
    const int64_t oB1 = (int64_t)h1 * din, oW2 = oB1 + h1, oB2 = oW2 + (int64_t)h2 * h1, oW3 = oB2 + h2, oB3 = oW3 + (int64_t)n * h2;
    for (int u = tid >> 6; u < HW; u += 4) {
      for (int c = lane; c < K1; c += 64) {
        const int f = feat(c);
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
      const int f = feat(c);
      ish[c] = f >= 0 ? tr[f] : 0.f;
      irs[c] = f >= 0 ? tr[din + f] + 1e-8f : 1.f;
    }
  }
  // ---- 5. the rest of a forward after layer 1's MFMAs: bias + activation, layer 2, and the output layer with affine, mask and
  // residual as in dyn_net_tile.  Block b reads s[b][r] before it writes out[b][r], so out may be s (the rollout's next state).
  __device__ __forceinline__ void tail(ChainLane L, f32x16 (&h1v)[HB], const f32x16 (&s)[NB], f32x16 (&out)[NB], int act, int flags) const {
    chain_bias_act(h1v, HB, b1s, L, act);
    f32x16 h2v[HB];
#pragma unroll
    for (int ob = 0; ob < HB; ++ob) {
      h2v[ob] = chain_dense(W2s, S2, ob, L, h1v, HB);
      chain_bias_act(h2v[ob], b2s + 32 * ob, L, act);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const f32x16 acc = chain_dense(W3s, S2, b, L, h2v, HB);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int u = 32 * b + unit_of(r, L.hi);
        float z = acc[r] + b3s[u];
        if (flags & DYN_OUT_AFFINE) z = z * osc[u] + osh[u];
        if (flags & DYN_MASK) z = z * msk[u];
        if (flags & DYN_RESIDUAL) z = z + s[b][r];
        out[b][r] = z;
      }
    }
  }
};

// ---- 6. a tanh policy [n, p1, p2, m] (FCNetwork with its transforms and log_std) in LDS, for a kernel that lets it act on state
// accumulators (policy_rollout.h).  Hidden widths padded to P1 = 32 p1b and P2 = 32 p2b (run-time block counts, 1 .. POL_MAX_PB),
// the output to one block of 32 action units in the action slot layout (unit f of the block is action f).  In floats:
//   Q1s P1 x (n8 + 4) | Q2s P2 x (P1 + 4) | Q3s 32 x (P2 + 4) | d1 P1 | d2 P2 | d3 32 | in_shift n8 | in_scale + 1e-8 n8 (1 where
//   padded) | out_scale, out_shift, exp(log_std), a_lo, a_hi: 32 each | s_lo, s_hi: NS = 32 NB each
// pol_lds_floats sums these terms in carve()'s order: carve(base) - base == pol_lds_floats for the same (p1, p2, n, NB).
// Padded action units have zero rows of Q3s and zero d3 / out_scale / out_shift / sigma, padded units of either kind the bounds
// [0, 0]; absent bounds are -inf / +inf.
constexpr int POL_MAX_PB = 2;
__host__ __device__ inline size_t pol_lds_floats(int p1, int p2, int n, int NB) {
  const size_t P1 = 32 * (size_t)((p1 + 31) / 32), P2 = 32 * (size_t)((p2 + 31) / 32), n8 = (size_t)pad8(n);
  return P1 * (n8 + 4) + P2 * (P1 + 4) + 32 * (P2 + 4) + P1 + P2 + 32 + 2 * n8 + 5 * 32 + 2 * 32 * (size_t)NB;
}

template <int NB>
struct PolImage {
  static constexpr int NS = 32 * NB;
  float *Q1s, *Q2s, *Q3s, *d1, *d2, *d3, *ish, *irs, *osc, *osh, *sig, *alo, *ahi, *slo, *shi;
  int n, m, n8, p1, p2, p1b, p2b, P1, P2, U1, U2, U3;

  __device__ __forceinline__ float* carve(float* base, int n_, int m_, int p1_, int p2_) {
    n = n_; m = m_; n8 = pad8(n); p1 = p1_; p2 = p2_;
    p1b = (p1 + 31) >> 5; p2b = (p2 + 31) >> 5; P1 = 32 * p1b; P2 = 32 * p2b; U1 = n8 + 4; U2 = P1 + 4; U3 = P2 + 4;
    Q1s = base; Q2s = Q1s + P1 * U1; Q3s = Q2s + P2 * U2;
    d1 = Q3s + 32 * U3; d2 = d1 + P1; d3 = d2 + P2;
    ish = d3 + 32; irs = ish + n8;
    osc = irs + n8; osh = osc + 32; sig = osh + 32; alo = sig + 32; ahi = alo + 32;
    slo = ahi + 32; shi = slo + NS;
    return shi + NS;
  }
  __device__ __forceinline__ ChainL1 l1() const { return ChainL1{Q1s, U1, ish, irs}; }
  // all 256 threads, before the barrier.  P = the policy's flat vector with log_std behind the output bias, tr = [in_shift n,
  // in_scale n, out_shift m, out_scale m]; the bounds are m / n floats each or null in pairs
  __device__ __forceinline__ void stage(const float* __restrict__ P, const float* __restrict__ tr, const float* __restrict__ a_lo,
                                        const float* __restrict__ a_hi, const float* __restrict__ s_lo, const float* __restrict__ s_hi,
                                        int tid) const {
    const int lane = tid & 63;
    const int64_t oB1 = (int64_t)p1 * n, oW2 = oB1 + p1, oB2 = oW2 + (int64_t)p2 * p1, oW3 = oB2 + p2, oB3 = oW3 + (int64_t)m * p2, oLS = oB3 + m;
    for (int u = tid >> 6; u < P1; u += 4)
      for (int c = lane; c < n8; c += 64) Q1s[u * U1 + c] = (u < p1 && c < n) ? P[(int64_t)u * n + c] : 0.f;
    for (int u = tid >> 6; u < P2; u += 4)
      for (int c = lane; c < P1; c += 64) Q2s[u * U2 + c] = (u < p2 && c < p1) ? P[oW2 + (int64_t)u * p1 + c] : 0.f;
    for (int u = tid >> 6; u < 32; u += 4)
      for (int c = lane; c < P2; c += 64) Q3s[u * U3 + c] = (u < m && c < p2) ? P[oW3 + (int64_t)u * p2 + c] : 0.f;
    for (int i = tid; i < P1; i += 256) d1[i] = i < p1 ? P[oB1 + i] : 0.f;
    for (int i = tid; i < P2; i += 256) d2[i] = i < p2 ? P[oB2 + i] : 0.f;
    for (int i = tid; i < 32; i += 256) {
      const bool on = i < m;
      d3[i] = on ? P[oB3 + i] : 0.f;
      osh[i] = on ? tr[2 * n + i] : 0.f;
      osc[i] = on ? tr[2 * n + m + i] : 0.f;
      sig[i] = on ? expf(P[oLS + i]) : 0.f;
      alo[i] = on ? (a_lo ? a_lo[i] : -INFINITY) : 0.f;
      ahi[i] = on ? (a_hi ? a_hi[i] : INFINITY) : 0.f;
    }
    for (int i = tid; i < NS; i += 256) {
      const bool on = i < n;
      slo[i] = on ? (s_lo ? s_lo[i] : -INFINITY) : 0.f;
      shi[i] = on ? (s_hi ? s_hi[i] : INFINITY) : 0.f;
    }
    for (int c = tid; c < n8; c += 256) {
      ish[c] = c < n ? tr[c] : 0.f;
      irs[c] = c < n ? tr[n + c] + 1e-8f : 1.f;
    }
  }
};

}  // namespace mjx
