// dyn_fit_ens.h -- k_dyn_fit_ens: the minibatch-Adam fit of a whole ensemble of dynamics nets, or of its reward nets, in ONE
// persistent launch.
//
// The reference's driver fits its K models one after the other, every outer iteration (run_model_accel_npg.py:168-177:
// `for model in ensemble: model.fit_dynamics(...)`), at hidden_size (256, 256) in both configs it ships -- the shape that
// mjx_dyn_fit_adam serves with ten launches per Adam step (dynamics.h k_dl_*).  Here workgroup k of a K-workgroup grid runs every
// step of member k by itself: gather -> forward -> MSE head -> backward -> torch.optim.Adam, the arithmetic of k_dyn_fit.  The
// workgroups never meet: no grid barrier, no flag, no shared word; parameters, moments, indices, losses and scratch are per member.
//
// Products run on v_mfma_f32_32x32x2_f32 in the chained, operand-swapped form of fused_policy.h / mlp_fit.h: the A operand
// carries the 32 output rows of a tile, the B operand its 32 columns, a lane half (hi) takes four consecutive k of a group of
// eight, and accumulator register r of lane (j, hi) is element [unit_of(r, hi)][j] of the tile.
//
// Where things live (two hidden layers h1, h2 <= 256, d_in <= 128, d_out <= 64, minibatch B <= 64):
//   weights, Adam moments   global memory (one member's 256 x 256 net is 280 KiB of weights and 560 KiB of moments: neither
//                           160 KiB of LDS nor the 512 KiB register file holds W2 beside anything else).  A workgroup stays on one
//                           CU, so its weights come back from that CU's L1 / the XCD's L2.
//   activations             LDS, as [unit][sample] tiles with the sample dimension padded to the MFMA tile (Bp = 32 or 64, row
//                           stride Bp + 4): H1, H2 (unit rows padded to 32: nothing for the aligned widths), the output block Z3
//                           (rows padded to 32) and the gathered inputs X (rows padded to 8).  (256 + 256 + 64) x 68 x 4 B = 153 KiB is the most H1 + H2 + Z3 take; when X no longer
//                           fits beside them (B > 32 with d_in + h1 + h2 + d_out near the limits) X goes to a per-member global
//                           scratch tile instead, the only operand it changes.
//   deltas                  in place: dMSE/dz3 over Z3; delta2 and delta1 are formed in registers (two 32 x 32 tiles a wave),
//                           held there while the weight gradient that still needs the activations runs, then written over H2 / H1.
// Padded sample columns (>= B) carry x = 0 forward and delta = 0 backward (the head writes exact zeros there), so they add
// exactly 0 to every gradient sum; padded rows of Z3 and X are zeros, and weight rows beyond a layer's width are never read.
//
// Two instances.  k_dyn_fit_ens<false>: the dynamics nets -- hidden widths multiples of 32, targets as k_dyn_prep forms them
// (modes 1 / 2), plain MSE head; its arithmetic is the kernel's from before the second instance existed, bit for bit.
// k_dyn_fit_ens<true> (RAG): any two hidden widths 1 .. 256 and the affine head of target mode 0, the RewardNet fit
// (mjx_reward_fit_ensemble; the reference's reward nets are (100, 100)).  What it adds:
//   ragged widths   the padded unit rows of H1 / H2 hold exact zeros forward (dfe_forward writes zeros for rows >= dj).  Backward
//                   dfe_delta covers the partial last tile, reads the weight columns >= di as zeros AND sets the padded rows of
//                   its result to zero outright -- tanh'(0) = 1, so the activation derivative would pass a stray product on --
//                   and dfe_delta_store writes those zeros over the padded rows.  They then add exactly 0 to every later
//                   delta, weight gradient and bias sum (the bias sums run over the real units only).  The four-weight loads
//                   of dfe_forward serve di % 4 == 0 with the groups at and beyond di masked (no load reaches past its row);
//                   other widths take the scalar arm.
//   affine head     c = out_scale + 1e-8: yhat = z c + out_shift, err = yhat - y_raw, loss = mean(err^2) over B x d_out,
//                   delta3 = (2 / (B d_out)) err c (dyn_loss_head's expressions); the per-member out_tr travels in the arguments.
//
// A step, with a workgroup barrier between the phases (8 waves = 2 a SIMD: fp32 MFMAs run at the vector ALU's rate and the
// two exclude each other, so the second wave is there to cover LDS / L2 latency, not to overlap VALU with MFMA):
//   gather X | H1 = act(W1 X + b1) | H2 | Z3 | head: loss, delta3 | delta2 (registers) | grad W3, b3 + Adam | delta2 -> H2,
//   delta1 (registers) | grad W2, b2 + Adam | delta1 -> H1 | grad W1, b1 + Adam
// Every delta is formed before the layer it reads is updated.  A weight-gradient tile (32 x 32, 16 accumulator registers) goes
// straight from the MFMA chain into the Adam update of the 16 weights the lane holds: gradients never touch memory.
//
// Out of scope: teams of several workgroups per member, bf16x3 products and more than two hidden layers: mjx_dyn_fit_route /
// mjx_reward_fit_route send them to mjx_dyn_fit_adam member by member.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfe_tiles.h"
#include "dynamics.h"
#include "mfma_prims.h"
#include "launch_state.h"
#include "vecops.h"

namespace mjx {

// (the workgroup's shape, dfe_pad32, dfe_fresh and dfe_forward: dfe_tiles.h, shared with k_policy_rollout_wide)
constexpr int DFE_MAXH = 256, DFE_MAXIN = 128, DFE_MAXOUT = 64, DFE_MAXB = 64;
constexpr int DFE_CHUNK = 64;                                // members per launch (their step counts travel as kernel arguments)
constexpr size_t DFE_STATIC_LDS = 8 * sizeof(double) + 64 * sizeof(int);

struct DfeLayout {
  int Bp, ST, K0, ZR;
  size_t tiles, xtile;                                      // floats of H1 + H2 + Z3; of X
  bool x_in_lds;
  __host__ DfeLayout(const DynNet& net, int batch) {
    Bp = batch > 32 ? 64 : 32; ST = Bp + 4;
    K0 = (net.din() + 7) & ~7; ZR = (net.dout() + 31) & ~31;
    tiles = (size_t)(dfe_pad32(net.sz[1]) + dfe_pad32(net.sz[2]) + ZR) * ST; xtile = (size_t)K0 * ST;
    x_in_lds = (tiles + xtile) * sizeof(float) + DFE_STATIC_LDS <= LDS_MAX;
  }
  __host__ size_t lds_bytes() const { return (tiles + (x_in_lds ? xtile : 0)) * sizeof(float); }
};

struct DynFitEnsArgs {
  int din, h1, h2, dout, B, act;
  int64_t P, N, steps;
  const float* xn; const float* tg;     // K x N x d_in normalised inputs, K x N x d_out targets (k_dyn_prep, per member)
  const int32_t* idx;                   // K x steps x B row indices
  float* W; float* m; float* v;         // K x P parameters and Adam moments, updated in place
  float* loss;                          // K x steps minibatch losses
  float* xscr;                          // null: the X tile is in LDS; else K x (K0 x ST) floats of scratch
  const float* otr;                     // the affine head (RAG instance): K x [out_shift (d_out), out_scale (d_out)]; else unused
  float lr, wd;
  int k0;                               // member of workgroup 0
  int64_t step0[DFE_CHUNK];             // Adam steps taken before this call, members k0 ..
};

// torch.optim.Adam as dyn_adam, in the v_rcp_f32 + Newton form (vecops.h: AdamRcp) with torch's constants: 1 - beta rounded
// once (0.1f, 0.001f).  `1.0f - 0.999f` is 0.0009999871, 1.3e-5 low: a bias of the same sign in every second moment, which alone
// moved a weight of the [13, 256, 256, 11] batch-16 test case by 2e-2 lr from the fp64 chain in ten steps.
__device__ __forceinline__ void dfe_adam_math(float& p, float& m, float& v, float g, float lr_bc1, float inv_bc2s, float wd) {
  p = AdamRcp<AdamTorch>{wd, lr_bc1, inv_bc2s}.one(p, g, m, v);
}
__device__ __forceinline__ void dfe_adam(float* p, float* m, float* v, int64_t i, float g, float lr_bc1, float inv_bc2s, float wd) {
  float p_ = p[i], m_ = m[i], v_ = v[i];
  dfe_adam_math(p_, m_, v_, g, lr_bc1, inv_bc2s, wd);
  p[i] = p_; m[i] = m_; v[i] = v_;
}

// dreg[q] = (sum_{jj < dj} W[jj][u] D[jj][s]) * act'(H[u][s]) for the wave's tiles q = 0, 1 of the MT x NS tiles of H
// (MT = di / 32; RAG: ceil(di / 32), where the columns u >= di of W read as zeros and the unit rows u >= di of the last tile
// come out as exact zeros whatever act'(0) is: tanh' (0) = 1 would pass a stray product on).  D: the [dj rounded up to
// 8][sample] delta tile, zeros beyond dj.
template <bool RAG>
__device__ __forceinline__ void dfe_delta(const float* __restrict__ W, int dj, int di, const float* D, const float* H, int ST, int NS,
                                          int act, int w, int j, int hi, f32x16 (&dreg)[2]) {
  dfe_fresh(w, j, hi);
  const int MT = RAG ? (di + 31) >> 5 : di >> 5, Kp = (dj + 7) & ~7;
#pragma unroll
  for (int q2 = 0; q2 < 2; ++q2) {
    const int t = w + DFE_WAVES * q2;
    if (t < MT * NS) {
      const int mt = t % MT, nt = t / MT;
      const bool cok = !RAG || 32 * mt + j < di;
      const float* wc = W + (cok ? 32 * mt + j : 0);
      f32x16 acc = (f32x16)(0.f);
      auto ld = [&](int kk, float (&av)[4], float (&bv)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool ok = kk + q < dj && cok;
          const float x = wc[(int64_t)(ok ? kk + q : 0) * di];
          av[q] = ok ? x : 0.f;
          bv[q] = D[(kk + q) * ST + 32 * nt + j];
        }
      };
      float ac[4], bc[4], an[4], bn[4];
      ld(4 * hi, ac, bc);
      for (int k0 = 0; k0 < Kp; k0 += 8) {
        ld((k0 + 8 < Kp ? k0 + 8 : k0) + 4 * hi, an, bn);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = MJX_MFMA(ac[q], bc[q], acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) { ac[q] = an[q]; bc[q] = bn[q]; }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[r] *= dyn_dact(H[(32 * mt + unit_of(r, hi)) * ST + 32 * nt + j], act);
        if (RAG && 32 * mt + unit_of(r, hi) >= di) acc[r] = 0.f;
      }
      dreg[q2] = acc;
    }
  }
}

template <bool RAG>
__device__ __forceinline__ void dfe_delta_store(const f32x16 (&dreg)[2], int di, float* H, int ST, int NS, int w, int j, int hi) {
  const int MT = RAG ? (di + 31) >> 5 : di >> 5;
#pragma unroll
  for (int q2 = 0; q2 < 2; ++q2) {
    const int t = w + DFE_WAVES * q2;
    if (t < MT * NS) {
      const int mt = t % MT, nt = t / MT;
#pragma unroll
      for (int r = 0; r < 16; ++r) H[(32 * mt + unit_of(r, hi)) * ST + 32 * nt + j] = dreg[q2][r];
    }
  }
}

// g[jj][i] = sum_s D[jj][s] In[i][s] tile by tile (32 x 32, a wave per tile), each tile straight into the Adam update of the
// weights W[jj][i] (jj < dj, i < di) its lanes hold; then the bias: g[jj] = sum_s D[jj][s], a thread per unit.  D: [dj rounded
// up to 32][sample]; in4(i, s) reads In[i][s .. s + 3] (zeros for a row the tile does not have).
template <class LdIn4>
__device__ __forceinline__ void dfe_grad_adam(const float* D, int dj, int di, LdIn4 in4, int Bp, int ST, float* __restrict__ P,
                                              float* __restrict__ Pm, float* __restrict__ Pv, int64_t oW, int64_t ob, float lr_bc1,
                                              float inv_bc2s, float wd, int tid, int w, int j, int hi) {
  dfe_fresh(w, j, hi);
  asm volatile("" : "+v"(tid));
  const int RT = (dj + 31) >> 5, CT = (di + 31) >> 5;
  for (int t = w; t < RT * CT; t += DFE_WAVES) {
    const int mt = t / CT, nt = t % CT;
    f32x16 acc = (f32x16)(0.f);
    f32x4 ac = *(const f32x4*)&D[(32 * mt + j) * ST + 4 * hi], bc = in4(32 * nt + j, 4 * hi);
    for (int s0 = 0; s0 < Bp; s0 += 8) {
      const int sn = (s0 + 8 < Bp ? s0 + 8 : s0) + 4 * hi;
      const f32x4 an = *(const f32x4*)&D[(32 * mt + j) * ST + sn], bn = in4(32 * nt + j, sn);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = MJX_MFMA(ac[q], bc[q], acc);
      ac = an; bc = bn;
    }
    // the 16 weights of this lane: row 32 mt + unit_of(r, hi), column 32 nt + j, eight at a time: all three blocks of the eight
    // are requested before the first update.  Offsets are 32-bit from the member's (uniform) base, so a row costs one register
    // for the three blocks; a lane outside the matrix reads the layer's first entry and stores nothing.
    const int col = 32 * nt + j;
    const unsigned e0 = (unsigned)oW + (unsigned)((32 * mt + 4 * hi) * di + col);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float pw[8], pm[8], pv[8];
#pragma unroll
      for (int r = 8 * h; r < 8 * h + 8; ++r) {
        const bool ok = 32 * mt + unit_of(r, hi) < dj && col < di;
        const unsigned e = ok ? e0 + (unsigned)(unit_of(r, 0) * di) : (unsigned)oW;
        pw[r & 7] = P[e]; pm[r & 7] = Pm[e]; pv[r & 7] = Pv[e];
      }
#pragma unroll
      for (int r = 8 * h; r < 8 * h + 8; ++r) {
        const bool ok = 32 * mt + unit_of(r, hi) < dj && col < di;
        const unsigned e = e0 + (unsigned)(unit_of(r, 0) * di);
        dfe_adam_math(pw[r & 7], pm[r & 7], pv[r & 7], acc[r], lr_bc1, inv_bc2s, wd);
        if (ok) { P[e] = pw[r & 7]; Pm[e] = pm[r & 7]; Pv[e] = pv[r & 7]; }
      }
    }
  }
  for (int u = tid; u < dj; u += DFE_THREADS) {
    float g = 0.f;
    for (int s = 0; s < Bp; ++s) g += D[u * ST + s];
    dfe_adam(P, Pm, Pv, ob + u, g, lr_bc1, inv_bc2s, wd);
  }
}

// RAG = false: the instance of the dynamics ensembles (hidden widths multiples of 32, targets formed by k_dyn_prep, plain MSE).
// RAG = true: any hidden width 1 .. 256 (tiles padded to 32 unit rows) and the affine head of target mode 0 (RewardNet).
template <bool RAG>
__global__ __launch_bounds__(DFE_THREADS) void k_dyn_fit_ens(DynFitEnsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float els[];
  __shared__ double red[DFE_WAVES];
  __shared__ int sIx[DFE_MAXB];
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int k = a.k0 + (int)blockIdx.x;
  const int din = a.din, h1 = a.h1, h2 = a.h2, dout = a.dout, B = a.B, act = a.act;
  const int Bp = B > 32 ? 64 : 32, NS = Bp >> 5, ST = Bp + 4;
  const int K0 = (din + 7) & ~7, ZR = (dout + 31) & ~31;
  const int h1p = RAG ? dfe_pad32(h1) : h1, h2p = RAG ? dfe_pad32(h2) : h2;
  float* H1 = els; float* H2 = H1 + h1p * ST; float* Z3 = H2 + h2p * ST; float* XL = Z3 + ZR * ST;
  const bool xg = a.xscr != nullptr;
  float* XG = xg ? a.xscr + (int64_t)k * K0 * ST : nullptr;
  const int64_t oW1 = 0, ob1 = (int64_t)h1 * din, oW2 = ob1 + h1, ob2 = oW2 + (int64_t)h2 * h1, oW3 = ob2 + h2, ob3 = oW3 + (int64_t)dout * h2;
  float* P = a.W + k * a.P; float* Pm = a.m + k * a.P; float* Pv = a.v + k * a.P;
  const float* xn = a.xn + (int64_t)k * a.N * din;
  const float* tg = a.tg + (int64_t)k * a.N * dout;
  const float* otr = RAG ? a.otr + (int64_t)k * 2 * dout : nullptr;
  const int32_t* idx = a.idx + (int64_t)k * a.steps * B;
  float* loss = a.loss + (int64_t)k * a.steps;
  const int64_t step0 = a.step0[blockIdx.x];
  auto ldx = [&](int r, int s) -> float { return xg ? XG[r * ST + s] : XL[r * ST + s]; };
  auto ldx4 = [&](int r, int s) -> f32x4 {
    const int rr = r < K0 ? r : 0;
    f32x4 q = xg ? *(const f32x4*)&XG[rr * ST + s] : *(const f32x4*)&XL[rr * ST + s];
    return r < K0 ? q : (f32x4)(0.f);
  };

  for (int64_t s = 0; s < a.steps; ++s) {
    // ---- gather: X[f][r] = xn[ix[r]][f], zeros in the padded rows and columns
    const int32_t* ix = idx + s * B;
    if (tid < DFE_MAXB) sIx[tid] = tid < B ? ix[tid] : 0;
    for (int e = tid; e < K0 * Bp; e += DFE_THREADS) {
      const int r = e / K0, f = e - r * K0;
      const float x = (r < B && f < din) ? xn[(int64_t)ix[r] * din + f] : 0.f;
      if (xg) XG[f * ST + r] = x; else XL[f * ST + r] = x;
    }
    __syncthreads();
    // ---- forward
    dfe_forward<RAG>(P + oW1, P + ob1, h1, din, K0, false, ldx, H1, ST, NS, act, w, j, hi);
    __syncthreads();
    dfe_forward<RAG>(P + oW2, P + ob2, h2, h1, RAG ? (h1 + 7) & ~7 : h1, RAG ? h1 % 4 == 0 : true, [&](int r, int c) { return H1[r * ST + c]; }, H2, ST, NS, act, w, j, hi);
    __syncthreads();
    dfe_forward<RAG>(P + oW3, P + ob3, dout, h2, RAG ? (h2 + 7) & ~7 : h2, RAG ? h2 % 4 == 0 : true, [&](int r, int c) { return H2[r * ST + c]; }, Z3, ST, NS, -1, w, j, hi);
    __syncthreads();
    // ---- MSE head: delta3 over Z3 (exact zeros in the padding), the step's loss
    double part = 0.0;
    const float dscale = 2.0f / (float)(B * dout);
    for (int e = tid; e < ZR * Bp; e += DFE_THREADS) {
      const int u = e / Bp, r = e - u * Bp;
      float d = 0.f;
      if (u < dout && r < B) {
        float z = Z3[u * ST + r], c = 1.f;
        if (RAG) { c = otr[dout + u] + 1e-8f; z = z * c + otr[u]; }                  // yhat = z c + out_shift, on raw y
        const float err = z - tg[(int64_t)sIx[r] * dout + u];
        d = dscale * err;
        if (RAG) d *= c;
        part += (double)err * (double)err;
      }
      Z3[u * ST + r] = d;
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) red[w] = part;
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      for (int q = 0; q < DFE_WAVES; ++q) tot += red[q];
      loss[s] = (float)(tot / (double)(B * dout));
    }
    float lr_bc1, bc2s;
    dyn_bias_corr(step0 + s + 1, a.lr, lr_bc1, bc2s);
    const float inv_bc2s = 1.0f / bc2s;
    // ---- layer 3: delta2 with W3 as it is, then W3's own update
    f32x16 dreg[2];
    dfe_delta<RAG>(P + oW3, dout, h2, Z3, H2, ST, NS, act, w, j, hi, dreg);
    __syncthreads();
    dfe_grad_adam(Z3, dout, h2, [&](int r, int c) { return *(const f32x4*)&H2[r * ST + c]; }, Bp, ST, P, Pm, Pv, oW3, ob3, lr_bc1,
                  inv_bc2s, a.wd, tid, w, j, hi);
    __syncthreads();
    dfe_delta_store<RAG>(dreg, h2, H2, ST, NS, w, j, hi);
    __syncthreads();
    // ---- layer 2
    dfe_delta<RAG>(P + oW2, h2, h1, H2, H1, ST, NS, act, w, j, hi, dreg);
    __syncthreads();
    dfe_grad_adam(H2, h2, h1, [&](int r, int c) { return *(const f32x4*)&H1[r * ST + c]; }, Bp, ST, P, Pm, Pv, oW2, ob2, lr_bc1,
                  inv_bc2s, a.wd, tid, w, j, hi);
    __syncthreads();
    dfe_delta_store<RAG>(dreg, h1, H1, ST, NS, w, j, hi);
    __syncthreads();
    // ---- layer 1
    dfe_grad_adam(H1, h1, din, ldx4, Bp, ST, P, Pm, Pv, oW1, ob1, lr_bc1, inv_bc2s, a.wd, tid, w, j, hi);
    __syncthreads();
  }
}

}  // namespace mjx
