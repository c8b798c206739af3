// policy_rollout_wide.h -- k_policy_rollout_wide: the policy acting inside a learned-model rollout for the nets the register chain of
// policy_rollout.h does not hold: dynamics nets up to 256 x 256 (the shape of both configs the reference ships), policies up to
// 256 x 256, any hidden width 1 .. 256.
//
// The scheme is k_dyn_fit_ens's forward half (dfe_tiles.h): activations as [unit][sample] LDS tiles, weights streamed row-major from
// global memory (one member's block: 1 MiB for K = 4 at 256 x 256, so L2 and the CU's L1 serve them), products on
// v_mfma_f32_32x32x2_f32, a wave per output tile of 32 units -- at 256 wide one tile per wave per layer.  Grid (ceil(N / 32), K),
// DFE_THREADS threads: a workgroup is ONE tile of 32 trajectories of one member through all H steps.  A forward requests the
// weights of the next group of eight k ahead of the four MFMAs of this one, as the fit does (four groups ahead measured 0.4 ms
// slower over 50 steps at 256 x 256).
//
// Where things live (n <= 64, m <= 64, n + m <= 128, hidden widths <= 256; ST = 32 + 4 floats a row):
//   S    n rows            the raw state of the tile, kept between steps
//   XD   pad8(n + m) rows  the normalised dynamics input [s, a]; its padding rows are zeroed once (nothing else writes them)
//   U    max(pad32(h1) + pad32(h2) + pad32(n), pad8(n) + pad32(p1) + pad32(p2) + pad32(m)) rows, used twice a step:
//          by the policy:    XP (normalised state, padding rows rewritten every step) | P1 | P2 | PZ (the output block)
//          by the dynamics:  H1 | H2 | Z3 -- written only after the action phase has read PZ, read for the last time before the
//                            next step's policy writes XP
//   C    the small vectors, staged once: the policy's b1, b2, b3, exp(log_std) and its 2 n + 2 m transforms, the member's b1, b2,
//        b3 and its 2 (n + m) + 2 n transforms (prw_const_floats).  Read from global memory where they are used, each would cost
//        its phase a round trip to L2, nine a step.  The bounds, where given, are read from global memory.
// The most a served shape takes is ((64 + 128 + 640) x 36 + 1 856) x 4 B = 127 232 B (wide_roll_lds_floats; the kernel has no
// static LDS).
//
// A step, with a workgroup barrier between the phases, in k_model_rollout's order and with its expressions (dynamics.h):
//   store s; XP = (s - in_shift) / (in_scale + 1e-8); the state rows of XD likewise | P1 = tanh(..) | P2 = tanh(..) | PZ |
//   a = clamp(PZ * out_scale + out_shift + noise * exp(log_std)) (PZ carries b3; no 1e-8 on the policy's output side); store a;
//   the action rows of XD; request the next step's noise | H1 | H2 | Z3 | flags (1 affine, 2 mask, 4 residual), clamp -> S
// The last phase and the next step's first one give an element of S to the same thread, so no barrier stands between them.  The
// dynamics forward after the last stored action is not run.
//
// Padded unit rows of every tile are exact zeros (dfe_forward writes zeros there whatever act(b) would be); padded sample columns
// (row >= N) start from a zero state with zero noise, are computed and never stored.  A sample column reaches only its own
// output column, so a NaN trajectory stays alone.  No atomics and no reductions across lanes: the bits are the same every run.
//
// Out of scope: more or fewer than two hidden layers, several workgroups per tile, bf16x3 products, a 64-row tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfe_tiles.h"
#include "policy_rollout.h"

namespace mjx {

// rows of the region the policy and the dynamics forward take in turn
__host__ __device__ constexpr int prw_shared_rows(int n, int m, int h1, int h2, int p1, int p2) {
  return dfe_pad32(h1) + dfe_pad32(h2) + dfe_pad32(n) > pad8(n) + dfe_pad32(p1) + dfe_pad32(p2) + dfe_pad32(m)
             ? dfe_pad32(h1) + dfe_pad32(h2) + dfe_pad32(n)
             : pad8(n) + dfe_pad32(p1) + dfe_pad32(p2) + dfe_pad32(m);
}
// floats of the small vectors staged once: the policy's b1, b2, b3, exp(log_std) and transforms, the member's b1, b2, b3 and transforms
__host__ __device__ constexpr int prw_const_floats(int n, int m, int h1, int h2, int p1, int p2) {
  return p1 + p2 + 2 * m + (2 * n + 2 * m) + h1 + h2 + n + (2 * (n + m) + 2 * n);
}
__host__ __device__ constexpr size_t wide_roll_lds_floats(int n, int m, int h1, int h2, int p1, int p2) {
  return (size_t)(n + pad8(n + m) + prw_shared_rows(n, m, h1, h2, p1, p2)) * WR_ST + prw_const_floats(n, m, h1, h2, p1, p2);
}

// PolRollArgs as mjx_policy_rollout fills them (policy_rollout.h)
__global__ __launch_bounds__(DFE_THREADS) void k_policy_rollout_wide(PolRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) float prw[];
  constexpr int ST = WR_ST, UQ = WR_UQ, NZ = WR_NZ;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int n = a.n, m = a.m, din = n + m, h1 = a.h1, h2 = a.h2, p1 = a.p1, p2 = a.p2;
  const int n8 = pad8(n), K0 = pad8(din);
  float* S = prw; float* XD = S + n * ST; float* U = XD + K0 * ST;
  float* XP = U; float* P1 = XP + n8 * ST; float* P2 = P1 + dfe_pad32(p1) * ST; float* PZ = P2 + dfe_pad32(p2) * ST;
  float* H1 = U; float* H2 = H1 + dfe_pad32(h1) * ST; float* Z3 = H2 + dfe_pad32(h2) * ST;
  const int k = blockIdx.y;
  // the small vectors of the policy and of member k go to LDS once (a phase would otherwise wait a round trip to L2 for them,
  // nine times a step); pol.tail is exp(log_std)
  float* cst = U + prw_shared_rows(n, m, h1, h2, p1, p2) * ST;
  const WideNet pol = dfe_stage_net(cst, a.pP, a.ptr, n, p1, p2, m, DYN_ACT_TANH, m, tid);
  const WideNet dyn = dfe_stage_net(cst, a.P + k * a.Pstride, a.tr + (int64_t)k * (2 * din + 2 * n), din, h1, h2, n, a.act, 0, tid);
  const float* ptr = pol.tr; const float* sig = pol.tail; const float* dtr = dyn.tr;
  const WideRollMap tm = wr_map(tid, a.N);
  const int c = tm.c, u0 = tm.u0;
  const bool valid = tm.valid;
  const int64_t vrow = tm.vrow;
  float* __restrict__ orow = a.obs + ((int64_t)k * a.N + vrow) * a.H * (int64_t)n;
  float* __restrict__ arow = a.act_out + ((int64_t)k * a.N + vrow) * a.H * (int64_t)m;
  const bool noisy = a.noise != nullptr;
  const float* __restrict__ zrow = noisy ? a.noise + ((int64_t)k * a.noise_k * a.N + vrow) * m : nullptr;
  const int64_t zstep = a.N * (int64_t)m;
  float nz[NZ];
#pragma unroll
  for (int q = 0; q < NZ; ++q) { const int f = u0 + UQ * q; nz[q] = (noisy && valid && f < m) ? zrow[f] : 0.f; }
  for (int i = u0; i < n; i += UQ) S[i * ST + c] = valid ? a.s0[vrow * a.s0_stride + i] : 0.f;
  for (int i = din + u0; i < K0; i += UQ) XD[i * ST + c] = 0.f;
  __syncthreads();                                          // (the staged vectors)
  for (int t = 0; t < a.H; ++t) {
    // ---- observations[:, t] is the state BEFORE step t; the policy's input and the state rows of the dynamics input
    for (int i = u0; i < n8; i += UQ) {
      float xp = 0.f;
      if (i < n) {
        const float s = S[i * ST + c];
        if (valid) orow[(int64_t)t * n + i] = s;
        xp = (s - ptr[i]) / (ptr[n + i] + 1e-8f);
        XD[i * ST + c] = (s - dtr[i]) / (dtr[din + i] + 1e-8f);
      }
      XP[i * ST + c] = xp;
    }
    __syncthreads();
    // ---- the policy mean
    dfe_forward3<1>(pol, XP, P1, P2, PZ, w, j, hi);
    // ---- actions[:, t]: out * out_scale + out_shift, + noise * exp(log_std), clamp; the action rows of the dynamics input
#pragma unroll
    for (int q = 0; q < NZ; ++q) {
      const int f = u0 + UQ * q;
      if (f < m) {
        float v = PZ[f * ST + c] * ptr[2 * n + m + f] + ptr[2 * n + f];
        if (noisy) v = v + nz[q] * sig[f];
        if (a.a_lo) v = dyn_clamp(v, a.a_lo[f], a.a_hi[f]);
        if (valid) arow[(int64_t)t * m + f] = v;
        XD[(n + f) * ST + c] = (v - dtr[n + f]) / (dtr[din + n + f] + 1e-8f);
      }
    }
    if (t + 1 == a.H) break;                                // (uniform: the last stored action needs no next state)
    if (noisy && valid) {                                   // the next step's noise: in flight under the dynamics forward
#pragma unroll
      for (int q = 0; q < NZ; ++q) { const int f = u0 + UQ * q; if (f < m) nz[q] = zrow[(int64_t)(t + 1) * zstep + f]; }
    }
    __syncthreads();
    // ---- the dynamics forward of member k
    dfe_forward3<1>(dyn, XD, H1, H2, Z3, w, j, hi);
    // ---- flags and the state clamp: the next state over S (element (i, c) belongs to the thread that reads it next)
    const float* osh = dtr + 2 * din; const float* osc = osh + n;
    for (int i = u0; i < n; i += UQ) {
      float z = dyn_out_flags(Z3[i * ST + c], a.flags, osh, osc, i, [&] { return S[i * ST + c]; });
      if (a.s_lo) z = dyn_clamp(z, a.s_lo[i], a.s_hi[i]);
      S[i * ST + c] = z;
    }
  }
}

}  // namespace mjx
