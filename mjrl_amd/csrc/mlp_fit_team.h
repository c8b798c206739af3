// mlp_fit_team.h -- the MLP-baseline trainer for minibatches of 128 .. 512 rows (d_in -> 128 -> 128 -> 1, ReLU): a TEAM of
// G = B / 64 workgroups, one per CU, launched as one grid, shares every Adam step.
//
// mlp_fit.h's trainers serve batch 64; every other batch size used to fall to ~14 launches per step (the reference's own model-based
// driver builds MLPBaseline(batch_size=256)).  One workgroup walking 2 B / 64 halves in sequence would fix the launch count and
// leave a step that grows linearly with B -- a larger minibatch is exactly where a step has parallel work to give away.  So:
//   * workgroup g takes rows [64 g, 64 g + 64) of every minibatch as two 32-sample halves -- the half body of k_mlp_fit (gather
//     with the two-stage prefetch, three chained MFMA layers, MSE head with 2 err / B, delta2, grad W3 / b3 / b2, grad W2 from
//     registers x h1^T, delta1, grad W1 / b1) -- on its own copy of the weight image in LDS;
//   * ONE exchange per step, after the second half: a thread publishes the gradient registers it holds (gW2[4], gW1[NF1], gb2,
//     gw3, gb3 and, on one lane, the workgroup's sum of squared errors) in slot [parity][g] of an uncached exchange block, laid
//     out [quad][thread] of f32x4 (a wave moves 1 KB per quad, coalesced); s_waitcnt vmcnt(0), workgroup barrier, one arrival on
//     the grid counter, the wait, workgroup barrier; then EVERY workgroup reads all G slots -- its own through memory as well --
//     and sums them from zero in workgroup order;
//   * every workgroup then holds the same bits, and the Adam update runs REPLICATED: identical data, identical instructions, so
//     the G weight images and the register-resident moments (the team trainer is register-moments only, as k_mlp_fit1p is) stay
//     bit-identical and no second exchange is needed.  Workgroup 0 alone writes parameters, moments and epoch losses back.
// Slots are double-buffered by step parity: a workgroup is at most one step ahead of another (it cannot pass barrier s + 1
// before all have read step s).  The grid barrier is the wide trainer's (k_mlp_fit<.., MULTI>): relaxed agent-scope atomics on the
// arrival counter, target G (phase + 1), s_sleep in the wait, give-up after ~2 s through the OR-ed word behind the counter,
// k_mlp_fit_verdict behind the trainer turning that word into NaN epoch losses, which MLPBaseline._settle rejects.
// The step body is written here, not as a flag of k_mlp_fit: sharing more structure cost the default instances registers and
// scratch (mlp_fit.h says where).
#pragma once
#include "mlp_fit.h"

namespace mjx {

constexpr int MLPFIT_TEAM_GMAX = 8;                // workgroups of a team: minibatches up to 512 rows
// f32x4 quads a thread publishes per step: gW2 (4 tiles x 4), gW1 (NF1 tiles x 4), {gb2, gw3, gb3, sum of squared errors}
__host__ __device__ constexpr int mlp_fit_team_quads(int nf1) { return 16 + 4 * nf1 + 1; }
// the exchange block [2 parities][G][quads][256 threads] of f32x4, sized for the largest team
constexpr size_t MLPFIT_TEAM_XBYTES = (size_t)2 * MLPFIT_TEAM_GMAX * mlp_fit_team_quads(2) * 256 * 16;

// acc[c] += slot g's quad (q0 + c), g = 0 .. G - 1 in order: CQ x 4 loads in flight, surplus slots neither read nor added
template <int CQ>
__device__ __forceinline__ void mlp_fit_team_sum(const f32x4* xi, int q0, size_t slot, int G, f32x4 (&acc)[CQ]) {
#pragma unroll
  for (int c = 0; c < CQ; ++c) acc[c] = (f32x4)(0.f);
  for (int g0 = 0; g0 < G; g0 += 4) {
    f32x4 t[4][CQ];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (g0 + u < G) {
#pragma unroll
        for (int c = 0; c < CQ; ++c) t[u][c] = xi[(size_t)(g0 + u) * slot + (size_t)(q0 + c) * 256];
      }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (g0 + u < G) {
#pragma unroll
        for (int c = 0; c < CQ; ++c) acc[c] += t[u][c];
      }
  }
}

// (no-packed-fp32-ops: the f32x2 / f32x4 arithmetic of this kernel -- adam.pairp, the slot sums -- is issued element by element,
// the same roundings as the packed forms.  flatten: a callee compiled with other target features -- __syncthreads, the lambdas, the
// layout's constructor -- is otherwise left as a CALL, with its captures in scratch)
template <int NF1>
__global__ __launch_bounds__(256, 1) __attribute__((target("no-packed-fp32-ops"), flatten)) void k_mlp_fit_team(MlpFitArgs A) {
  constexpr int H = 128;
  using LT = MlpFitLayout<H>;
  constexpr int ST = LT::ST, S2 = LT::S2, NT = H / 32, NQ = mlp_fit_team_quads(NF1);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int g_id = (int)blockIdx.x, G = A.G, BS = A.batch;
  const int d_in = A.d_in;
  const LT L(d_in, NF1 > 1);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int K1 = L.K1, S1 = L.S1;
  unsigned phase = 0;                                                 // grid barriers passed = steps taken in this call
  bool timed_out = false;
  float* sW1 = lds + L.oW1; float* sW2 = lds + L.oW2; float* sW3 = lds + L.oW3; float* sB2 = lds + L.oB2;
  float* sB3 = sB2 + H;
  float* xs = lds + L.oXS; float* xT = lds + L.oXT; float* h1T = lds + L.oH1; float* h2T = lds + L.oH2; float* d2T = lds + L.oD2;
  float* sY = lds + L.oY; float* sPart = lds + L.oPART; float* sDY = lds + L.oDY;
  const MlpFitBlock<H> B(d_in, 0, d_in, true);

  // ---- every workgroup: the whole parameter block into its LDS, the moments into its own copy of the interleaved workspace
  mlp_fit_load_params<H>(A, B, L, lds, tid);
  if (tid < 32) { if (NF1 == 1) xs[tid * S1 + d_in] = 1.0f; xT[d_in * ST + tid] = 1.0f; }
  float* const mvbase = A.mv + (int64_t)g_id * 2 * B.P;
  mlp_fit_load_moments<H>(A, B, mvbase, tid);
  __syncthreads();

  double pw1 = pow((double)ADAM32_B1, (double)A.step0), pw2 = pow((double)ADAM32_B2, (double)A.step0);
  constexpr int GL = (32 * 32 * NF1 + 255) / 256;   // gather elements per thread (d_in <= 32 NF1 - 1)
  float gx[GL];
  float gy = 0.f;
  // two-stage prefetch as in k_mlp_fit: row indices one half-step before the rows they address, the rows one half-step before
  // they are staged.  Row s of half hb of workgroup g: perm[ep N + mb B + 64 g + 32 hb + s]
  int gidx[GL];
  int gyi = 0;
  int gs[GL], gf[GL];
#pragma unroll
  for (int c = 0; c < GL; ++c) {
    const int e = c * 256 + tid;
    gs[c] = (e < 32 * d_in) ? e / d_in : -1;
    gf[c] = e - (e / d_in) * d_in;
  }
  auto index_load = [&](int ep, int64_t mb, int hb) {
    const int32_t* idx = A.perm + (int64_t)ep * A.N + mb * BS + 64 * g_id + 32 * hb;
#pragma unroll
    for (int c = 0; c < GL; ++c) gidx[c] = idx[gs[c] >= 0 ? gs[c] : 0];
    gyi = idx[tid & 31];
  };
  auto gather_load = [&]() {
#pragma unroll
    for (int c = 0; c < GL; ++c) gx[c] = A.feat[gs[c] >= 0 ? (int64_t)gidx[c] * d_in + gf[c] : 0];
    gy = A.y[gyi];
  };
  auto gather_store = [&]() {
#pragma unroll
    for (int c = 0; c < GL; ++c)
      if (gs[c] >= 0) { if (NF1 == 1) xs[gs[c] * S1 + gf[c]] = gx[c]; xT[gf[c] * ST + gs[c]] = gx[c]; }
    if (tid < 32) sY[tid] = gy;
  };

  // ---- the weights this thread applies Adam to (k_mlp_fit's ownership), their moments in registers for the whole run,
  // re-paired for packed math: entry r (even) = the first moments of weights r, r + 1, entry r + 1 = their second moments
  f32x2* __restrict__ MV = (f32x2*)mvbase;
  f32x2* __restrict__ mvW2 = MV + B.oW2 + (int64_t)(32 * w + 4 * hi) * H + j;
  float* pW2 = sW2 + (32 * w + 4 * hi) * S2 + j;
  bool own1[NF1];
  int stg[NF1];
  f32x2* mvW1[NF1];
  float* pW1[NF1];
#pragma unroll
  for (int fb = 0; fb < NF1; ++fb) {
    const int f = 32 * fb + j;
    const bool isw = f < d_in;
    own1[fb] = isw || f == d_in;
    stg[fb] = isw ? d_in : 1;
    const int64_t gbase1 = isw ? B.oW1 + (int64_t)(32 * w + 4 * hi) * d_in + f : B.oB1 + 32 * w + 4 * hi;
    mvW1[fb] = MV + (own1[fb] ? gbase1 : 0);
    pW1[fb] = sW1 + (32 * w + 4 * hi) * S1 + (isw ? f : d_in);
  }
  const bool ownb2 = hi == 0, ownw3 = tid < H, ownb3 = tid == 0;
  const int64_t gb2i = B.oB2 + 32 * w + j, gw3i = B.oW3 + (ownw3 ? tid : 0), gb3i = B.oB3;
  f32x2 q2[NT][16], q1[NF1][16], qb2, qw3, qb3;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const f32x2 a = mvW2[unit_of(r, 0) * H + 32 * nt], b = mvW2[unit_of(r + 1, 0) * H + 32 * nt];
      q2[nt][r] = f32x2{a.x, b.x}; q2[nt][r + 1] = f32x2{a.y, b.y};
    }
#pragma unroll
  for (int fb = 0; fb < NF1; ++fb)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const f32x2 a = mvW1[fb][own1[fb] ? unit_of(r, 0) * stg[fb] : 0], b = mvW1[fb][own1[fb] ? unit_of(r + 1, 0) * stg[fb] : 0];
      q1[fb][r] = f32x2{a.x, b.x}; q1[fb][r + 1] = f32x2{a.y, b.y};
    }
  qb2 = MV[gb2i]; qw3 = MV[gw3i]; qb3 = MV[gb3i];

  const size_t slot = (size_t)NQ * 256;             // f32x4 entries of one workgroup's slot

  for (int ep = 0; ep < A.epochs; ++ep) {
    double ep_loss = 0.0;
    if (A.steps > 0) { index_load(ep, 0, 0); gather_load(); index_load(ep, 0, 1); }
#pragma unroll 1
    for (int64_t mb = 0; mb < A.steps; ++mb) {
      f32x16 gW2[NT], gW1[NF1];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) gW2[nt] = (f32x16)(0.f);
#pragma unroll
      for (int fb = 0; fb < NF1; ++fb) gW1[fb] = (f32x16)(0.f);
      float gb2 = 0.f, gw3 = 0.f, gb3 = 0.f, sse = 0.f;
      float w3v[16];                                // this lane's 16 output-layer weights, fetched once per step
#pragma unroll
      for (int r = 0; r < 16; ++r) w3v[r] = sW3[32 * w + unit_of(r, hi)];
#pragma unroll 1
      for (int hb = 0; hb < 2; ++hb) {
        // this lane's windows on the tiles, re-made every half (FitLane: pinned bases, base + immediate at every use)
        const FitLane<true> h1w(h1T, (32 * w + 4 * hi) * ST + j), d2w(d2T, (32 * w + 4 * hi) * ST + j);   // row group 32 w + 4 hi, sample j
        const FitLane<true> h2w(h2T, (32 * w + 4 * hi) * ST + j);
        const FitLane<true> h1c(h1T, (4 * hi) * ST + j), d2c(d2T, (4 * hi) * ST + j);                     // rows k (+ const), sample j
        const FitLane<true> h1r(h1T, (32 * w + j) * ST + 4 * hi), d2r(d2T, (32 * w + j) * ST + 4 * hi);   // row = this lane's unit, 4 samples per read
        const FitLane<true> h1n(h1T, j * ST + 4 * hi);                                                    // rows 32 nt + j
        const FitLane<true> w2r(sW2, (32 * w + j) * S2 + 4 * hi), w2c(sW2, (4 * hi) * S2 + 32 * w + j);
        gather_store();
        __syncthreads();
        // prefetch the next half's rows while this half computes
        if (hb == 0) { gather_load(); if (mb + 1 < A.steps) index_load(ep, mb + 1, 0); }       // rows of half 1; indices of the next step
        else if (mb + 1 < A.steps) { gather_load(); index_load(ep, mb + 1, 1); }
        // ---- layer 1: z1[unit 32w+., sample] = W1a x~a ; h1 = relu
        f32x16 z1 = (f32x16)(0.f);
        for (int q = 0; q < K1 / 4; ++q) {
          const int f0 = 4 * q + 2 * hi;
          f32x2 a = *(const f32x2*)&sW1[(32 * w + j) * S1 + f0];
          f32x2 b;
          if (NF1 == 1) b = *(const f32x2*)&xs[j * S1 + f0];
          else b = f32x2{xT[f0 * ST + j], xT[(f0 + 1) * ST + j]};
          z1 = MJX_MFMA(a.x, b.x, z1);
          z1 = MJX_MFMA(a.y, b.y, z1);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) h1w.st(unit_of(r, 0) * ST, fmaxf(z1[r], 0.f));         // row 32 w + unit_of(r, hi)
        __syncthreads();
        // ---- layer 2: K = all 128 h1 units (B operand from the shared h1^T tile)
        f32x16 z2;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 b = *(const f32x4*)&sB2[32 * w + 8 * q + 4 * hi];
          z2[4 * q] = b.x; z2[4 * q + 1] = b.y; z2[4 * q + 2] = b.z; z2[4 * q + 3] = b.w;
        }
        __builtin_amdgcn_sched_barrier(0);
        {
          f32x4 ac, an;
          float bc[4], bn[4];
          ac = w2r.ld4(0);                                                  // W2[32 w + j][4 hi ..]
#pragma unroll
          for (int t = 0; t < 4; ++t) bc[t] = h1c.ld1(t * ST);
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            if (g + 1 < 16) {
              const int k1c = 32 * ((g + 1) >> 2) + 8 * ((g + 1) & 3);          // (+ 4 hi: in the windows)
              an = w2r.ld4(k1c);
#pragma unroll
              for (int t = 0; t < 4; ++t) bn[t] = h1c.ld1((k1c + t) * ST);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) z2 = MJX_MFMA(ac[t], bc[t], z2);
            ac = an;
#pragma unroll
            for (int t = 0; t < 4; ++t) bc[t] = bn[t];
          }
          // in-order single wave: keep group g+1's five LDS fetches ahead of group g's four MFMAs
          __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            if (g + 1 < 16) __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float hv = fmaxf(z2[r], 0.f);
          z2[r] = hv;
          h2w.st(unit_of(r, 0) * ST, hv);
          part = fmaf(w3v[r], hv, part);
        }
        part = half_sum(part);
        if (hi == 0) sPart[w * 32 + j] = part;
        __syncthreads();
        // ---- output + MSE gradient (every wave redundantly, lane j = sample): MSELoss(mean) over the B-row minibatch
        const float yhat = (sPart[j] + sPart[32 + j]) + (sPart[64 + j] + sPart[96 + j]) + sB3[0];
        const float err = yhat - sY[j];
        const float dy = 2.0f * err / (float)BS;
        if (w == 0 && hi == 0) {
          sDY[j] = dy;
          const float e2 = sum32_lane0(err * err);
          if (j == 0) sse += e2;                            // (this workgroup's 64 rows; the team's sum is formed after the exchange)
        }
        // delta2 (lane = sample) -> d2T [unit][sample]
#pragma unroll
        for (int r = 0; r < 16; ++r) d2w.st(unit_of(r, 0) * ST, (z2[r] > 0.f) ? w3v[r] * dy : 0.f);
        __syncthreads();
        // ---- grad W3 / b3 (thread = unit), grad b2, delta2 in lane = unit layout straight from d2T
        if (tid < H) {
          float a = 0.f;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            f32x4 hv = *(const f32x4*)&h2T[tid * ST + 4 * q];
            f32x4 dv = *(const f32x4*)&sDY[4 * q];
            a += hv.x * dv.x + hv.y * dv.y + hv.z * dv.z + hv.w * dv.w;
          }
          gw3 += a;
        }
        if (tid == 0) { float a = 0.f; for (int s = 0; s < 32; ++s) a += sDY[s]; gb3 += a; }
        f32x16 d2u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 t4 = d2r.ld4(8 * q);
          d2u[4 * q] = t4.x; d2u[4 * q + 1] = t4.y; d2u[4 * q + 2] = t4.z; d2u[4 * q + 3] = t4.w;
        }
        {
          float s2 = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) s2 += d2u[r];
          gb2 += half_sum(s2);
        }
        // grad W2 rows of this wave: A = delta2u (registers), B = h1^T tiles
        {
          f32x4 bc[NT], bn[NT];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) bc[nt] = h1n.ld4(32 * nt * ST);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (q + 1 < 4) {
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) bn[nt] = h1n.ld4(32 * nt * ST + 8 * (q + 1));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) gW2[nt] = MJX_MFMA(d2u[4 * q + t], bc[nt][t], gW2[nt]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bc[nt] = bn[nt];
          }
        }
        // delta1 (lane = h1 unit of this wave's tile): A = delta2 [sample][k] from d2T, B = W2[k][unit]
        f32x16 d1u = (f32x16)(0.f);
        __builtin_amdgcn_sched_barrier(0);
        {
          float ac[4], an[4], bc[4], bn[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) { ac[t] = d2c.ld1(t * ST); bc[t] = w2c.ld1(t * S2); }
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            if (g + 1 < 16) {
              const int k1c = 32 * ((g + 1) >> 2) + 8 * ((g + 1) & 3);
#pragma unroll
              for (int t = 0; t < 4; ++t) { an[t] = d2c.ld1((k1c + t) * ST); bn[t] = w2c.ld1((k1c + t) * S2); }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) d1u = MJX_MFMA(ac[t], bc[t], d1u);
#pragma unroll
            for (int t = 0; t < 4; ++t) { ac[t] = an[t]; bc[t] = bn[t]; }
          }
          __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            if (g + 1 < 16) __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {                       // relu'(z1) mask from h1^T (same layout)
          const f32x4 hv = h1r.ld4(8 * q);
          d1u[4 * q] = hv.x > 0.f ? d1u[4 * q] : 0.f; d1u[4 * q + 1] = hv.y > 0.f ? d1u[4 * q + 1] : 0.f;
          d1u[4 * q + 2] = hv.z > 0.f ? d1u[4 * q + 2] : 0.f; d1u[4 * q + 3] = hv.w > 0.f ? d1u[4 * q + 3] : 0.f;
        }
        // grad W1a rows of this wave (column d_in = grad b1)
#pragma unroll
        for (int fb = 0; fb < NF1; ++fb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int f = 32 * fb + j;
            f32x4 b4 = *(const f32x4*)&xT[(f < K1 ? f : 0) * ST + 8 * q + 4 * hi];
            if (f >= K1) b4 = (f32x4)(0.f);
#pragma unroll
            for (int t = 0; t < 4; ++t) gW1[fb] = MJX_MFMA(d1u[4 * q + t], b4[t], gW1[fb]);
          }
        __syncthreads();                                    // tiles are rewritten by the next half
      }

      // ---- the exchange: this workgroup's partial gradients -> slot [parity][g_id], quad q of thread tid at [q][tid]
      {
        f32x4* xo = (f32x4*)A.xch + ((size_t)(phase & 1u) * (size_t)G + (size_t)g_id) * slot + tid;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int q = 0; q < 4; ++q) xo[(size_t)(4 * nt + q) * 256] = f32x4{gW2[nt][4 * q], gW2[nt][4 * q + 1], gW2[nt][4 * q + 2], gW2[nt][4 * q + 3]};
#pragma unroll
        for (int fb = 0; fb < NF1; ++fb)
#pragma unroll
          for (int q = 0; q < 4; ++q) xo[(size_t)(16 + 4 * fb + q) * 256] = f32x4{gW1[fb][4 * q], gW1[fb][4 * q + 1], gW1[fb][4 * q + 2], gW1[fb][4 * q + 3]};
        xo[(size_t)(NQ - 1) * 256] = f32x4{gb2, gw3, gb3, sse};
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // uncached stores: acknowledged by memory, nothing holds them back
      __syncthreads();
      if (tid == 0) timed_out = mlp_fit_grid_barrier(A.bar, G, phase, timed_out);
      __syncthreads();
      // ---- every workgroup: the sum of all G slots from zero, in workgroup order (its own slot through memory as well: its
      // registers are dead after the publish, the sum needs no second copy) -- the same bits on every workgroup
      {
        const f32x4* xi = (const f32x4*)A.xch + (size_t)(phase & 1u) * (size_t)G * slot + tid;
        asm volatile("" : "+v"(xi) :: "memory");                      // (a fresh look at memory every step: nothing cached in registers)
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          mlp_fit_team_sum<4>(xi, 4 * nt, slot, G, acc);
#pragma unroll
          for (int q = 0; q < 4; ++q) { gW2[nt][4 * q] = acc[q].x; gW2[nt][4 * q + 1] = acc[q].y; gW2[nt][4 * q + 2] = acc[q].z; gW2[nt][4 * q + 3] = acc[q].w; }
        }
#pragma unroll
        for (int fb = 0; fb < NF1; ++fb) {
          mlp_fit_team_sum<4>(xi, 16 + 4 * fb, slot, G, acc);
#pragma unroll
          for (int q = 0; q < 4; ++q) { gW1[fb][4 * q] = acc[q].x; gW1[fb][4 * q + 1] = acc[q].y; gW1[fb][4 * q + 2] = acc[q].z; gW1[fb][4 * q + 3] = acc[q].w; }
        }
        // the scalar quad: all G of them in flight at once; the squared errors sum in double
        f32x4 t[MLPFIT_TEAM_GMAX];
#pragma unroll
        for (int g = 0; g < MLPFIT_TEAM_GMAX; ++g) t[g] = xi[(size_t)(g < G ? g : 0) * slot + (size_t)(NQ - 1) * 256];
        gb2 = 0.f; gw3 = 0.f; gb3 = 0.f;
        double ss = 0.0;
#pragma unroll
        for (int g = 0; g < MLPFIT_TEAM_GMAX; ++g)
          if (g < G) { gb2 += t[g].x; gw3 += t[g].y; gb3 += t[g].z; ss += (double)t[g].w; }
        ep_loss += ss / (double)BS;                         // (thread 0's lane holds the workgroups' sums; the others add zeros)
        ++phase;
      }

      // ---- Adam, replicated (torch.optim.Adam: L2 weight decay folded into the gradient, bias-corrected)
      const MlpFitAdam adam = mlp_fit_adam_step(pw1, pw2, A.lr, A.wd);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const int l0 = unit_of(r, 0) * S2 + 32 * nt, l1 = unit_of(r + 1, 0) * S2 + 32 * nt;
          const f32x2 pn = adam.pairp(f32x2{pW2[l0], pW2[l1]}, f32x2{gW2[nt][r], gW2[nt][r + 1]}, q2[nt][r], q2[nt][r + 1]);
          pW2[l0] = pn.x; pW2[l1] = pn.y;
        }
#pragma unroll
      for (int fb = 0; fb < NF1; ++fb)
        if (own1[fb]) {
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const int l0 = unit_of(r, 0) * S1, l1 = unit_of(r + 1, 0) * S1;
            const f32x2 pn = adam.pairp(f32x2{pW1[fb][l0], pW1[fb][l1]}, f32x2{gW1[fb][r], gW1[fb][r + 1]}, q1[fb][r], q1[fb][r + 1]);
            pW1[fb][l0] = pn.x; pW1[fb][l1] = pn.y;
          }
        }
      if (ownb2) sB2[32 * w + j] = adam.one(sB2[32 * w + j], gb2, qb2);
      if (ownw3) sW3[tid] = adam.one(sW3[tid], gw3, qw3);
      if (ownb3) sB3[0] = adam.one(sB3[0], gb3, qb3);
      __syncthreads();
    }
    if (tid == 0 && g_id == 0) A.epoch_loss[ep] = ep_loss;
    if (tid == 0 && timed_out) A.epoch_loss[ep] = (double)__builtin_nanf("");      // (any workgroup that gave up says so; the verdict kernel decides)
  }
  // ---- workgroup 0 alone writes the trained parameters and the moments back (the others hold the same bits)
  if (g_id != 0) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      mvW2[unit_of(r, 0) * H + 32 * nt] = f32x2{q2[nt][r].x, q2[nt][r + 1].x};
      mvW2[unit_of(r + 1, 0) * H + 32 * nt] = f32x2{q2[nt][r].y, q2[nt][r + 1].y};
    }
#pragma unroll
  for (int fb = 0; fb < NF1; ++fb)
    if (own1[fb]) {
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        mvW1[fb][unit_of(r, 0) * stg[fb]] = f32x2{q1[fb][r].x, q1[fb][r + 1].x};
        mvW1[fb][unit_of(r + 1, 0) * stg[fb]] = f32x2{q1[fb][r].y, q1[fb][r + 1].y};
      }
    }
  if (ownb2) MV[gb2i] = qb2;
  if (ownw3) MV[gw3i] = qw3;
  if (ownb3) MV[gb3i] = qb3;
  __syncthreads();
  mlp_fit_store_moments<H, false>(A, B, mvbase, 0, tid);
  mlp_fit_store_params<H, false>(A, B, L, lds, 0, tid);
}

}  // namespace mjx
