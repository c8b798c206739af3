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
// workgroup's own H2 slice, Z3 and the gathered X.  The products are dyn_fit_ens.h's functions, called on the slice: the tile
// dimensions (dfe_dims), the forward of layers 1 and 2 (dfe_forward on the slice's rows), the deltas (dfe_delta with W's
// leading dimension: the W3 columns of the slice; the W2 rows without act'), their stores (dfe_delta_store, into LDS or into
// the exchange), the weight gradients with Adam (dfe_grad_adam: the W3 columns with the row stride h2 and b3 on workgroup 0
// only, the W2 and W1 rows whole) and dfe_bias_corr.  Its own: dfet_out_partial, the slice's share of the output layer, and
// the lines of the gather, the head and the member's pointers, which k_dyn_fit_ens has too (see there).
//
// One Adam step has three team barriers, each with one exchange through an UNCACHED global block (its own region per barrier,
// dfe_team_xch, double-buffered by step parity):
//   gather X (every workgroup, redundantly) | H1 slice -> published | A | all of H1 into LDS | H2 slice | the partial output
//   W3[:, slice] H2[slice] (d_out x B, no bias) -> published, b3 beside workgroup 0's | B | Z3 = the G partials summed from zero
//   in workgroup order, + b3, and with the same bits on every team-mate the MSE head replicated: loss (workgroup 0 writes it),
//   delta3 | delta2[slice] from the W3 columns (registers) | grad W3 columns (+ b3: workgroup 0) + Adam | delta2 -> H2 |
//   the partial delta1_g = W2[slice, :]^T delta2[slice] over ALL h1 units (registers) -> published | grad W2 rows, b2 + Adam
//   (from the full H1) | C | delta1[slice] = (the G partials summed in workgroup order) act'(H1[slice]) over the H1 slice |
//   grad W1 rows, b1 + Adam
// Every delta is formed before the layer it reads is updated, and a weight-gradient tile goes from the accumulator straight into
// Adam, as in k_dyn_fit_ens.  (b3 travels through the exchange because workgroup 0 updates it: a team-mate on another XCD would
// read a stale cached copy.)
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

// The floats of a team's three exchange regions of one parity, for the host's block and for the kernel's pointers:
// [H1: h1 x Bp | G partial outputs ZR x Bp, then b3 | G partial delta1 h1 x Bp]
struct DfeTeamXch { int64_t nA, nB, nC; };
__host__ __device__ __forceinline__ DfeTeamXch dfe_team_xch(int G, int h1, int Bp, int ZR) {
  return {(int64_t)h1 * Bp, (int64_t)(G * Bp + 1) * ZR, (int64_t)G * h1 * Bp};
}
// The team of a net with two hidden layers as dfe_serves takes them: G = 4 where both widths are multiples of 128, G = 2 where
// both are multiples of 64, else none (G = 0); the LDS tiles of a workgroup (full H1, own H2 slice, Z3, X) and the floats of one
// member's exchange block (the three regions, both parities)
struct DfeTeamLayout : DfeDims {
  int G;
  size_t tiles, slot;
  __host__ DfeTeamLayout(const DynNet& net, int batch) : DfeDims(dfe_dims(batch, net.din(), net.dout())) {
    const int h1 = net.sz[1], h2 = net.sz[2];
    G = (h1 % 128 == 0 && h2 % 128 == 0) ? 4 : (h1 % 64 == 0 && h2 % 64 == 0) ? 2 : 0;
    tiles = (size_t)(h1 + (G ? h2 / G : h2) + ZR + K0) * ST;
    const DfeTeamXch x = dfe_team_xch(G, h1, Bp, ZR);
    slot = (size_t)(2 * (x.nA + x.nB + x.nC));
  }
  __host__ bool fits() const { return G > 0 && tiles * sizeof(float) + DFET_STATIC_LDS <= LDS_MAX; }
  __host__ size_t lds_bytes() const { return tiles * sizeof(float) > DFET_MIN_LDS ? tiles * sizeof(float) : DFET_MIN_LDS; }
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
// (dfe_forward with a leading dimension, no bias and the output's own stride: kept apart, dfe_forward is the forward of four
// more kernels.)
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
  const DfeDims T = dfe_dims(B, din, dout);
  const int Bp = T.Bp, NS = T.NS, ST = T.ST, K0 = T.K0, ZR = T.ZR, B4 = Bp >> 2;
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
  const DfeTeamXch X = dfe_team_xch(G, h1, Bp, ZR);
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
    float* XA = xch + (s & 1) * (X.nA + X.nB + X.nC); float* XB = XA + X.nA; float* XC = XB + X.nB;
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
    float lr_bc1, inv_bc2s;
    dfe_bias_corr(step0 + s + 1, a.lr, lr_bc1, inv_bc2s);
    // ---- layer 3: delta2[slice] with the W3 columns as they are, then their own update (b3: workgroup 0)
    f32x16 dreg[2];
    dfe_delta<false>(P + oW3 + o2, h2, dout, s2, Z3, H2, ST, NS, act, true, w, j, hi, dreg);
    __syncthreads();
    dfe_grad_adam(Z3, dout, s2, h2, [&](int r, int c) { return *(const f32x4*)&H2[r * ST + c]; }, Bp, ST, P, Pm, Pv, oW3 + o2, ob3, g == 0,
                  lr_bc1, inv_bc2s, a.wd, tid, w, j, hi);
    __syncthreads();
    dfe_delta_store<false>(dreg, s2, H2, ST, NS, w, j, hi);
    __syncthreads();
    // ---- layer 2: the partial delta1 over all h1 units with the W2 rows as they are, published; the rows' own update; C
    dfe_delta<false>(P + oW2 + (int64_t)o2 * h1, h1, s2, h1, H2, nullptr, ST, NS, act, false, w, j, hi, dreg);
    dfe_delta_store<false>(dreg, h1, XC + (int64_t)g * h1 * Bp, Bp, NS, w, j, hi);
    __syncthreads();
    dfe_grad_adam(H2, s2, h1, h1, [&](int r, int c) { return *(const f32x4*)&H1[r * ST + c]; }, Bp, ST, P, Pm, Pv, oW2 + (int64_t)o2 * h1, ob2 + o2,
                  true, lr_bc1, inv_bc2s, a.wd, tid, w, j, hi);
    if (team_barrier()) break;
    // ---- layer 1: delta1[slice] = (the partials summed from zero in workgroup order) act'(H1[slice]), over the H1 slice
    for (int e = tid; e < s1 * Bp; e += DFE_THREADS) {
      const int u = o1 + e / Bp, c = e % Bp;
      float d = 0.f;
      for (int q = 0; q < G; ++q) d += XC[((int64_t)q * h1 + u) * Bp + c];
      H1[u * ST + c] = d * dyn_dact(H1[u * ST + c], act);
    }
    __syncthreads();
    dfe_grad_adam(H1s, s1, din, din, ldx4, Bp, ST, P, Pm, Pv, oW1 + (int64_t)o1 * din, ob1 + o1, true, lr_bc1, inv_bc2s, a.wd, tid, w, j, hi);
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
