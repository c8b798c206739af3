// dyn_fit_ens_team.h -- k_dyn_fit_ens_team: the minibatch-Adam fit of an ensemble of dynamics nets with a TEAM of G workgroups
// per member, one per CU, all teams in one persistent launch.
//
// k_dyn_fit_ens (dyn_fit_ens.h) gives a member one workgroup, so an ensemble of K = 4 keeps four CUs busy, and the steps of one
// member are a dependent chain: the parallelism left is inside a step.  Here a grid of K x G workgroups runs the same step,
// workgroups [k G, k G + G) being member k's team.  The team splits the HIDDEN UNITS of both layers: workgroup g owns units
// [g h1 / G, (g + 1) h1 / G) of layer 1 and [g h2 / G, (g + 1) h2 / G) of layer 2, i.e. the W1 rows, the W2 rows and the W3
// columns of its slices, their biases (b3: workgroup 0) and their Adam moments.  It alone reads and writes them (in global
// memory, cached in its CU's L1 / its XCD's L2, as k_dyn_fit_ens keeps them): no weight is replicated, no Adam update runs
// twice, and no cached word is read by a workgroup that does not own it.  Teams of different members never meet.
//
// Activations are LDS tiles in dfe_tiles.h's [unit][sample] layout (Bp = 32 or 64, row stride Bp + 4): the FULL H1, the
// workgroup's own H2 slice, Z3 and the gathered X.  The products are dyn_fit_ens.h's chained, operand-swapped fp32 MFMAs; the
// forward of layers 1 and 2 and the weight gradients of W2 and W1 ARE its functions on the slice's rows.
//
// One Adam step has three team barriers, each with one exchange through an UNCACHED global block (its own region per barrier,
// double-buffered by step parity):
//   gather X (every workgroup, redundantly) | H1 slice -> published | A | all of H1 into LDS | H2 slice | the partial output
//   W3[:, slice] H2[slice] (d_out x B, no bias) -> published, b3 beside workgroup 0's | B | Z3 = the G partials summed from zero
//   in workgroup order, + b3, and with the same bits on every team-mate the MSE head replicated: loss (workgroup 0 writes it),
//   delta3 | delta2[slice] from the W3 columns (registers) | grad W3 columns (+ b3: workgroup 0) + Adam | delta2 -> H2 |
//   the partial delta1_g = W2[slice, :]^T delta2[slice] over ALL h1 units (registers) -> published | grad W2 rows, b2 + Adam
//   (from the full H1) | C | delta1[slice] = (the G partials summed in workgroup order) act'(H1[slice]) over the H1 slice |
//   grad W1 rows, b1 + Adam
// Every delta is formed before the layer it reads is updated, and a weight-gradient tile goes from the accumulator straight into
// Adam, as in k_dyn_fit_ens.  The targets (modes 1 / 2), dfe_adam with torch's constants, the head's 2 err / (B d_out) and the
// zeros in padded sample columns and padded Z3 / X rows are dyn_fit_ens.h's expressions.  (b3 travels through the exchange
// because workgroup 0 updates it: a team-mate on another XCD would read a stale cached copy.)
//
// The barrier is mlp_fit.h's mlp_fit_grid_barrier with one counter word and one give-up word PER MEMBER (uncached, zeroed per
// call): relaxed agent-scope arrivals, target G (phase + 1), s_sleep in the wait.  A workgroup whose wait times out marks the
// member's give-up word and leaves at once -- it writes no parameter or moment after that; its team-mates give up at their next
// barrier -- and k_dfe_team_verdict, launched behind the trainer, turns the member's losses into NaN.  The host launches at most
// floor(CUs / G) members at a time and sizes the workgroup's LDS so that two never share a CU (fit_host.h dfe_team_run).
#pragma once
#include "dyn_fit_ens.h"
#include "mlp_fit.h"

namespace mjx {

constexpr size_t DFET_STATIC_LDS = DFE_STATIC_LDS + 16;     // k_dyn_fit_ens's red / sIx and the give-up flag
constexpr size_t DFET_MIN_LDS = LDS_MAX / 2 + 1024;         // dynamic LDS of a workgroup at least: two cannot share a CU

// The team of a net with two hidden layers as dfe_serves takes them: G = 4 where both widths are multiples of 128, G = 2 where
// both are multiples of 64, else none (G = 0); the LDS tiles of a workgroup (full H1, own H2 slice, Z3, X) and the floats of the
// three exchange regions of one parity
struct DfeTeamLayout {
  int G, Bp, ST, K0, ZR;
  size_t tiles, xa, xb, xc;
  __host__ DfeTeamLayout(const DynNet& net, int batch) {
    const int h1 = net.sz[1], h2 = net.sz[2];
    G = (h1 % 128 == 0 && h2 % 128 == 0) ? 4 : (h1 % 64 == 0 && h2 % 64 == 0) ? 2 : 0;
    Bp = batch > 32 ? 64 : 32; ST = Bp + 4;
    K0 = (net.din() + 7) & ~7; ZR = (net.dout() + 31) & ~31;
    tiles = (size_t)(h1 + (G ? h2 / G : h2) + ZR + K0) * ST;
    xa = (size_t)h1 * Bp; xb = (size_t)(G * Bp + 1) * ZR; xc = (size_t)G * h1 * Bp;
  }
  __host__ bool fits() const { return G > 0 && tiles * sizeof(float) + DFET_STATIC_LDS <= LDS_MAX; }
  __host__ size_t lds_bytes() const { return tiles * sizeof(float) > DFET_MIN_LDS ? tiles * sizeof(float) : DFET_MIN_LDS; }
  __host__ size_t slot_floats() const { return 2 * (xa + xb + xc); }       // one member's exchange block, both parities
};

struct DynFitTeamArgs {
  DynFitEnsArgs e;                      // k_dyn_fit_ens's arguments (xscr, otr unused); e.k0: the member of team 0
  int G;                                // workgroups a team
  float* xch;                           // UNCACHED: one slot of `xslot` floats per team of the launch
  unsigned* bar;                        // UNCACHED, zeroed per call: [arrival counter, give-up word] per member of the CALL
  int64_t xslot;
};

// out[u][s] = sum_{k < nk} W[u][k] in[k][s] for u < dj (zeros for the rows up to the tile's 32), no bias and no activation: the
// partial output of one slice.  W: rows of ldw floats (the slice's columns start at W), nk a multiple of 8; out: [.][Bp] in
// the exchange block, written from the accumulators (a lane's 16 stores lie in 16 rows; a wave's in 128-byte runs).
template <class LdIn>
__device__ __forceinline__ void dfet_out_partial(const float* __restrict__ W, int ldw, int dj, int nk, LdIn in, float* out, int Bp, int NS,
                                                 int w, int j, int hi) {
  dfe_fresh(w, j, hi);
  const int MT = (dj + 31) >> 5;
  for (int t = w; t < MT * NS; t += DFE_WAVES) {
    const int mt = t % MT, nt = t / MT;
    const int row = 32 * mt + j;
    const bool rok = row < dj;
    const float* wr = W + (int64_t)(rok ? row : 0) * ldw;
    f32x16 acc = (f32x16)(0.f);
    auto lda = [&](int kk, float (&av)[4]) {
      const f32x4u a4 = *(const f32x4u*)(wr + kk);
#pragma unroll
      for (int q = 0; q < 4; ++q) av[q] = rok ? a4[q] : 0.f;
    };
    float ac[4], bc[4], an[4], bn[4];
    lda(4 * hi, ac);
#pragma unroll
    for (int q = 0; q < 4; ++q) bc[q] = in(4 * hi + q, 32 * nt + j);
    for (int k0 = 0; k0 < nk; k0 += 8) {
      const int kk = (k0 + 8 < nk ? k0 + 8 : k0) + 4 * hi;
      lda(kk, an);
#pragma unroll
      for (int q = 0; q < 4; ++q) bn[q] = in(kk + q, 32 * nt + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = MJX_MFMA(ac[q], bc[q], acc);
#pragma unroll
      for (int q = 0; q < 4; ++q) { ac[q] = an[q]; bc[q] = bn[q]; }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(32 * mt + unit_of(r, hi)) * Bp + 32 * nt + j] = acc[r];
  }
}

// dfe_delta for a slice: dreg[q] = sum_{jj < dj} W[jj][u] D[jj][s] for the wave's tiles q = 0, 1 of the (nu / 32) x NS tiles
// (nu a multiple of 32, at most 16 tiles), times act'(H[u][s]) where ACT.  W: dj rows of ldw floats, unit u at column u of W;
// D: the [dj rounded up to 8][sample] delta tile, zeros beyond dj.
template <bool ACT>
__device__ __forceinline__ void dfet_delta(const float* __restrict__ W, int ldw, int dj, int nu, const float* D, const float* H, int ST, int NS,
                                           int act, int w, int j, int hi, f32x16 (&dreg)[2]) {
  dfe_fresh(w, j, hi);
  const int MT = nu >> 5, Kp = (dj + 7) & ~7;
#pragma unroll
  for (int q2 = 0; q2 < 2; ++q2) {
    const int t = w + DFE_WAVES * q2;
    if (t < MT * NS) {
      const int mt = t % MT, nt = t / MT;
      const float* wc = W + 32 * mt + j;
      f32x16 acc = (f32x16)(0.f);
      auto ld = [&](int kk, float (&av)[4], float (&bv)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool ok = kk + q < dj;
          const float x = wc[(int64_t)(ok ? kk + q : 0) * ldw];
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
      if (ACT) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= dyn_dact(H[(32 * mt + unit_of(r, hi)) * ST + 32 * nt + j], act);
      }
      dreg[q2] = acc;
    }
  }
}

// the partial delta1 of a workgroup from the registers dfet_delta left into its [nu][Bp] block of the exchange
__device__ __forceinline__ void dfet_delta_publish(const f32x16 (&dreg)[2], int nu, float* out, int Bp, int NS, int w, int j, int hi) {
  const int MT = nu >> 5;
#pragma unroll
  for (int q2 = 0; q2 < 2; ++q2) {
    const int t = w + DFE_WAVES * q2;
    if (t < MT * NS) {
      const int mt = t % MT, nt = t / MT;
#pragma unroll
      for (int r = 0; r < 16; ++r) out[(32 * mt + unit_of(r, hi)) * Bp + 32 * nt + j] = dreg[q2][r];
    }
  }
}

// dfe_grad_adam for COLUMNS of a layer: g[jj][i] = sum_s D[jj][s] In[i][s] for jj < dj and the di columns (a multiple of 32) that
// start at offset oW of the member's block, rows ldw floats apart, each 32 x 32 tile straight into the Adam update of its
// weights; then, where `bias`, the layer's bias at ob from the row sums of D.  in4(i, s) reads In[i][s .. s + 3].
template <class LdIn4>
__device__ __forceinline__ void dfet_grad_adam_cols(const float* D, int dj, int di, int ldw, LdIn4 in4, int Bp, int ST, float* __restrict__ P,
                                                    float* __restrict__ Pm, float* __restrict__ Pv, int64_t oW, int64_t ob, bool bias,
                                                    float lr_bc1, float inv_bc2s, float wd, int tid, int w, int j, int hi) {
  dfe_fresh(w, j, hi);
  asm volatile("" : "+v"(tid));
  const int RT = (dj + 31) >> 5, CT = di >> 5;
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
    // (dfe_grad_adam's walk over the lane's 16 weights, eight at a time; a lane outside the rows reads the slice's first entry)
    const int col = 32 * nt + j;
    const unsigned e0 = (unsigned)oW + (unsigned)((32 * mt + 4 * hi) * ldw + col);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float pw[8], pm[8], pv[8];
#pragma unroll
      for (int r = 8 * h; r < 8 * h + 8; ++r) {
        const bool ok = 32 * mt + unit_of(r, hi) < dj;
        const unsigned e = ok ? e0 + (unsigned)(unit_of(r, 0) * ldw) : (unsigned)oW;
        pw[r & 7] = P[e]; pm[r & 7] = Pm[e]; pv[r & 7] = Pv[e];
      }
#pragma unroll
      for (int r = 8 * h; r < 8 * h + 8; ++r) {
        const bool ok = 32 * mt + unit_of(r, hi) < dj;
        const unsigned e = e0 + (unsigned)(unit_of(r, 0) * ldw);
        dfe_adam_math(pw[r & 7], pm[r & 7], pv[r & 7], acc[r], lr_bc1, inv_bc2s, wd);
        if (ok) { P[e] = pw[r & 7]; Pm[e] = pm[r & 7]; Pv[e] = pv[r & 7]; }
      }
    }
  }
  if (bias)
    for (int u = tid; u < dj; u += DFE_THREADS) {
      float g = 0.f;
      for (int s = 0; s < Bp; ++s) g += D[u * ST + s];
      dfe_adam(P, Pm, Pv, ob + u, g, lr_bc1, inv_bc2s, wd);
    }
}

// (no-packed-fp32-ops: the element-wise float arithmetic of this kernel -- act' over an accumulator, Adam over a lane's weights --
// is issued element by element, the same roundings as the packed forms.  flatten: a callee compiled with other target features is
// otherwise left as a CALL, with its captures in scratch; mlp_fit_team.h does the same)
__global__ __launch_bounds__(DFE_THREADS) __attribute__((target("no-packed-fp32-ops"), flatten)) void k_dyn_fit_ens_team(DynFitTeamArgs t) {
  const DynFitEnsArgs& a = t.e;
  extern __shared__ __attribute__((aligned(16))) float els[];
  __shared__ double red[DFE_WAVES];
  __shared__ int sIx[DFE_MAXB];
  __shared__ int sGaveUp;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 31, hi = lane >> 5;
  const int G = t.G, team = (int)blockIdx.x / G, g = (int)blockIdx.x - team * G;
  const int k = a.k0 + team;
  const int din = a.din, h1 = a.h1, h2 = a.h2, dout = a.dout, B = a.B, act = a.act;
  const int Bp = B > 32 ? 64 : 32, NS = Bp >> 5, ST = Bp + 4, B4 = Bp >> 2;
  const int K0 = (din + 7) & ~7, ZR = (dout + 31) & ~31;
  const int s1 = h1 / G, s2 = h2 / G, o1 = g * s1, o2 = g * s2;         // this workgroup's units of layer 1 and of layer 2
  float* H1 = els; float* H2 = H1 + h1 * ST; float* Z3 = H2 + s2 * ST; float* XL = Z3 + ZR * ST;     // H2: the slice's rows only
  float* H1s = H1 + o1 * ST;
  const int64_t oW1 = 0, ob1 = (int64_t)h1 * din, oW2 = ob1 + h1, ob2 = oW2 + (int64_t)h2 * h1, oW3 = ob2 + h2, ob3 = oW3 + (int64_t)dout * h2;
  float* P = a.W + k * a.P; float* Pm = a.m + k * a.P; float* Pv = a.v + k * a.P;
  const float* xn = a.xn + (int64_t)k * a.N * din;
  const float* tg = a.tg + (int64_t)k * a.N * dout;
  const int32_t* idx = a.idx + (int64_t)k * a.steps * B;
  float* loss = a.loss + (int64_t)k * a.steps;
  const int64_t step0 = a.step0[team];
  // the exchange: per parity [H1: h1 x Bp | G partial outputs ZR x Bp, then b3 | G partial delta1 h1 x Bp]
  const int64_t nA = (int64_t)h1 * Bp, nB = (int64_t)(G * Bp + 1) * ZR, nC = (int64_t)G * h1 * Bp;
  float* const xch = t.xch + (int64_t)team * t.xslot;
  unsigned* const bar = t.bar + 2 * (int64_t)k;
  unsigned phase = 0;                                                   // team barriers passed in this call
  auto ldx = [&](int r, int s) -> float { return XL[r * ST + s]; };
  auto ldx4 = [&](int r, int s) -> f32x4 {
    const int rr = r < K0 ? r : 0;
    const f32x4 q = *(const f32x4*)&XL[rr * ST + s];
    return r < K0 ? q : (f32x4)(0.f);
  };
  // everything this workgroup published is in memory (uncached stores are acknowledged by memory), then one arrival and the
  // wait; -> a wait timed out: the workgroup leaves.  What the team-mates published is read after it, never from a register.
  auto team_barrier = [&]() -> bool {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) sGaveUp = mlp_fit_grid_barrier(bar, G, phase, false) ? 1 : 0;
    __syncthreads();
    asm volatile("" ::: "memory");
    ++phase;
    return sGaveUp != 0;
  };

  for (int64_t s = 0; s < a.steps; ++s) {
    float* XA = xch + (s & 1) * (nA + nB + nC); float* XB = XA + nA; float* XC = XB + nB;
    // ---- gather: X[f][r] = xn[ix[r]][f], zeros in the padded rows and columns (every workgroup of the team: no exchange)
    const int32_t* ix = idx + s * B;
    if (tid < DFE_MAXB) sIx[tid] = tid < B ? ix[tid] : 0;
    for (int e = tid; e < K0 * Bp; e += DFE_THREADS) {
      const int r = e / K0, f = e - r * K0;
      XL[f * ST + r] = (r < B && f < din) ? xn[(int64_t)ix[r] * din + f] : 0.f;
    }
    __syncthreads();
    // ---- layer 1: the slice's rows of H1, published; A; the team-mates' rows into LDS
    dfe_forward<false>(P + oW1 + (int64_t)o1 * din, P + ob1 + o1, s1, din, K0, false, ldx, H1s, ST, NS, act, w, j, hi);
    __syncthreads();
    for (int e = tid; e < s1 * B4; e += DFE_THREADS) {
      const int u = o1 + e / B4, c = 4 * (e % B4);
      *(f32x4*)&XA[u * Bp + c] = *(const f32x4*)&H1[u * ST + c];
    }
    if (team_barrier()) break;
    for (int e = tid; e < (h1 - s1) * B4; e += DFE_THREADS) {
      const int uu = e / B4, u = uu < o1 ? uu : uu + s1, c = 4 * (e % B4);
      *(f32x4*)&H1[u * ST + c] = *(const f32x4*)&XA[u * Bp + c];
    }
    __syncthreads();
    // ---- layer 2: the slice's rows of H2 from all of H1; the partial output W3[:, slice] H2[slice], published (+ b3); B
    dfe_forward<false>(P + oW2 + (int64_t)o2 * h1, P + ob2 + o2, s2, h1, h1, true, [&](int r, int c) { return H1[r * ST + c]; }, H2, ST, NS, act, w, j, hi);
    __syncthreads();
    dfet_out_partial(P + oW3 + o2, h2, dout, s2, [&](int r, int c) { return H2[r * ST + c]; }, XB + (int64_t)g * ZR * Bp, Bp, NS, w, j, hi);
    if (g == 0 && tid < dout) XB[(int64_t)G * ZR * Bp + tid] = P[ob3 + tid];
    if (team_barrier()) break;
    // ---- Z3 = the partials summed from zero in workgroup order, + b3; MSE head: delta3 over Z3 (exact zeros in the padding), the loss
    double part = 0.0;
    const float dscale = 2.0f / (float)(B * dout);
    for (int e = tid; e < ZR * Bp; e += DFE_THREADS) {
      const int u = e / Bp, r = e - u * Bp;
      float d = 0.f;
      if (u < dout && r < B) {
        float z = 0.f;
        for (int q = 0; q < G; ++q) z += XB[((int64_t)q * ZR + u) * Bp + r];
        z += XB[(int64_t)G * ZR * Bp + u];
        const float err = z - tg[(int64_t)sIx[r] * dout + u];
        d = dscale * err;
        part += (double)err * (double)err;
      }
      Z3[u * ST + r] = d;
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) red[w] = part;
    __syncthreads();
    if (tid == 0 && g == 0) {
      double tot = 0.0;
      for (int q = 0; q < DFE_WAVES; ++q) tot += red[q];
      loss[s] = (float)(tot / (double)(B * dout));
    }
    float lr_bc1, bc2s;
    dyn_bias_corr(step0 + s + 1, a.lr, lr_bc1, bc2s);
    const float inv_bc2s = 1.0f / bc2s;
    // ---- layer 3: delta2[slice] with the W3 columns as they are, then their own update (b3: workgroup 0)
    f32x16 dreg[2];
    dfet_delta<true>(P + oW3 + o2, h2, dout, s2, Z3, H2, ST, NS, act, w, j, hi, dreg);
    __syncthreads();
    dfet_grad_adam_cols(Z3, dout, s2, h2, [&](int r, int c) { return *(const f32x4*)&H2[r * ST + c]; }, Bp, ST, P, Pm, Pv, oW3 + o2, ob3, g == 0,
                        lr_bc1, inv_bc2s, a.wd, tid, w, j, hi);
    __syncthreads();
    dfe_delta_store<false>(dreg, s2, H2, ST, NS, w, j, hi);
    __syncthreads();
    // ---- layer 2: the partial delta1 over all h1 units with the W2 rows as they are, published; the rows' own update; C
    dfet_delta<false>(P + oW2 + (int64_t)o2 * h1, h1, s2, h1, H2, nullptr, ST, NS, act, w, j, hi, dreg);
    dfet_delta_publish(dreg, h1, XC + (int64_t)g * h1 * Bp, Bp, NS, w, j, hi);
    __syncthreads();
    dfe_grad_adam(H2, s2, h1, [&](int r, int c) { return *(const f32x4*)&H1[r * ST + c]; }, Bp, ST, P, Pm, Pv, oW2 + (int64_t)o2 * h1, ob2 + o2,
                  lr_bc1, inv_bc2s, a.wd, tid, w, j, hi);
    if (team_barrier()) break;
    // ---- layer 1: delta1[slice] = (the partials summed from zero in workgroup order) act'(H1[slice]), over the H1 slice
    for (int e = tid; e < s1 * Bp; e += DFE_THREADS) {
      const int u = o1 + e / Bp, c = e % Bp;
      float d = 0.f;
      for (int q = 0; q < G; ++q) d += XC[((int64_t)q * h1 + u) * Bp + c];
      H1[u * ST + c] = d * dyn_dact(H1[u * ST + c], act);
    }
    __syncthreads();
    dfe_grad_adam(H1s, s1, din, ldx4, Bp, ST, P, Pm, Pv, oW1 + (int64_t)o1 * din, ob1 + o1, lr_bc1, inv_bc2s, a.wd, tid, w, j, hi);
    __syncthreads();
  }
}

// behind the trainer, a workgroup per member of the call: a team that gave up on a barrier left a mark in the member's give-up
// word -> every loss of that member becomes NaN, whatever its workgroup 0 wrote (k_mlp_fit_verdict's rule)
__global__ void k_dfe_team_verdict(const unsigned* __restrict__ bar, float* __restrict__ loss, int64_t steps) {
  const int64_t k = blockIdx.x;
  if (__hip_atomic_load(bar + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
  for (int64_t e = threadIdx.x; e < steps; e += blockDim.x) loss[k * steps + e] = __builtin_nanf("");
}
// the counters and give-up words of a call, cleared on its stream
__global__ void k_dfe_team_clear(unsigned* __restrict__ bar, int64_t words) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < words; e += (int64_t)gridDim.x * blockDim.x) bar[e] = 0u;
}

}  // namespace mjx
