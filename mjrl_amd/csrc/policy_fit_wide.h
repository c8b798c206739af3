// policy_fit_wide.h -- persistent single-workgroup minibatch-Adam trainer for the manipulation-sized tanh-MLP policies: two hidden
// layers of equal width H in {32, 64}, up to 64 observations, up to 32 actions, minibatches of up to 64 rows (the hand_dapg class:
// 39 .. 46 observations, 24 .. 30 actions).  Same contract as k_policy_fit (policy_fit.h), whose shape-free pieces it uses as they
// are -- mma_tiles, fit_layer, fit_back, fresh and the two-deep minibatch prefetch --, but a layout and a step of its own:
//
//   * NO gradient image.  The weight-gradient product leaves every gradient element in a register of exactly one lane; that lane owns
//     the element's two Adam moments (registers, for the whole launch) and updates the weight in LDS right there, in the product's
//     epilogue.  Each of the three products has at most 16 output tiles (H / 16 x ceil(n / 16), (H / 16)^2, ceil(m / 16) x H / 16),
//     one per wave, so a lane owns 4 elements per product: 24 moment registers.  A bias or log_std entry u is owned by thread 16 u,
//     the lane that ends up with its sixteen-partial row sum: 8 more registers.
//   * Phase order.  Updating W_l in place is only safe once nothing reads the old W_l: fit_back of layer l reads W_l, so BOTH cotangent
//     products run first (two phases), then the three weight-gradient products, which no longer depend on each other, as ONE phase
//     (W3's tiles start at the far end of the waves, so that a wave has two tiles where the three products have at most 32).
//     Workgroup barriers per step: minibatch 1, forward 3 (+ 3 for PPO's fixed old network), loss head 1, backward 3 = 8 (11).
//   * Loss head: one (row, action) per lane, a row on 32 lanes, 32 rows per pass of the 1024 threads; the row totals are row16_sum
//     plus the neighbouring 16-lane row (v_permlane16_swap).  Lanes with a >= m and rows >= B contribute exact zeros.
//   * LDS.  The per-action blocks have a row stride of 36 and are updated in place by the lane that read them: dLoss/dmean over the
//     means, the per-row log_std term over the actions.  The old network's inputs have a block of their own at the observation
//     stride; its hidden activations pass through D2 / D1, which are free until the backward pass.  In floats, with Bp = B rounded
//     up to 16, S1 = n rounded up to 16 + 4, S2 = H + 4:  P (+ P) + Bp (S1 (+ S1) + 4 S2 + 2 x 36 (+ 36) + 4) + 552.
//
// The summation order inside a step depends on the shape alone (tiles, partial sums and butterflies are fixed), so a call continued
// with step0 and the carried moments repeats the bits of one longer call.
#pragma once
#include "policy_fit.h"

namespace mjx {

constexpr int PFW_MS = 36;               // row stride of the per-action blocks: 32 (two contraction blocks) + 4
constexpr int PFW_MISC = 8 + 416 + 128;  // step scalars, transform table ([4][64] in, [4][32] out, [32] old log_std), row ids [2][64]

template <int H>
struct PolicyFitWideLayout {
  int n, m, S1, S2, M16;            // S1: row stride of W1 and of the observation blocks, S2: of W2 / W3 and the hidden blocks
  int oW1, ob1, oW2, ob2, oW3, ob3, oS, P;
  __host__ __device__ PolicyFitWideLayout(int n_, int m_) {
    n = n_; m = m_;
    S1 = ((n + 15) & ~15) + 4; S2 = H + 4; M16 = (m + 15) & ~15;
    // W3 has M16 rows (zero rows behind the m real ones: fit_back's column operand walks whole blocks of 16 units)
    oW1 = 0; ob1 = oW1 + H * S1; oW2 = ob1 + H; ob2 = oW2 + H * S2; oW3 = ob2 + H; ob3 = oW3 + M16 * S2;
    oS = ob3 + M16; P = oS + M16;
  }
  __host__ __device__ int pad_of(int i) const {      // flat reference order [W1, b1, W2, b2, W3, b3, log_std] -> padded offset
    int k = i;
    if (k < H * n) return oW1 + (k / n) * S1 + k % n;
    k -= H * n; if (k < H) return ob1 + k;
    k -= H; if (k < H * H) return oW2 + (k / H) * S2 + k % H;
    k -= H * H; if (k < H) return ob2 + k;
    k -= H; if (k < m * H) return oW3 + (k / H) * S2 + k % H;
    k -= m * H; if (k < m) return ob3 + k;
    k -= m; return oS + k;
  }
  __host__ __device__ int d() const { return H * n + H + H * H + H + m * H + m + m; }
  __host__ __device__ size_t lds_floats(int B, bool old_net) const {
    const size_t Bp = (size_t)((B + 15) & ~15), o = old_net ? 1 : 0;
    return (size_t)P * (1 + o) + Bp * ((size_t)S1 * (1 + o) + 4 * (size_t)S2 + (size_t)PFW_MS * (2 + o) + 4) + PFW_MISC;
  }
};

// x[lane] + x[lane ^ 16] in every lane: v_permlane16_swap exchanges the odd 16-lane rows of one copy with the even rows of the other
__device__ __forceinline__ float pair16_sum(float p) {
  auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(p), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}
__device__ __forceinline__ float row32_sum(float v) { return pair16_sum(row16_sum(v)); }

// one torch.optim.Adam step on a parameter in LDS whose two moments the calling lane keeps in registers
__device__ __forceinline__ void pfw_adam(float* w, float g, float& am, float& av, float inv_bc2s, float step_size) {
  const float mi = am + (g - am) * ADAM_C1;
  const float vi = av * ADAM_B2 + g * g * ADAM_C2;
  am = mi; av = vi;
  const float denom = fmaf(__builtin_amdgcn_sqrtf(vi), inv_bc2s, ADAM_EPS);
  *w = fmaf(-step_size, fast_div(mi, denom), *w);
}

// W[u][k] -= Adam(sum_s delta[s][u] in[s][k]) for u < OUT, k < K, in place.  At most 16 tiles: the tile of wave (tid >> 6) is
// (r, c) = (wave % TR, wave / TR), and lane (q, r16) of it holds rows 16 r + 4 q .. + 3 of column 16 c + r16 -- pfw_owned() below is
// the same map for the prologue and the write-back.  (delta's rows s >= B are zero.)
__device__ __forceinline__ void pfw_wgrad_adam(const float* __restrict__ delta, int DS, const float* __restrict__ in, int IS, int B, int OUT,
                                               int K, float* __restrict__ Wl, int WS, float (&am)[4], float (&av)[4], float inv_bc2s,
                                               float step_size, int tid) {
  const int lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  mma_tiles<true, true>(tid, delta, DS, in, IS, (OUT + 15) >> 4, (K + 15) >> 4, (B + 15) >> 4, [&](int r, int c, f32x4 acc) {
    const int u0 = 16 * r + 4 * q, k = 16 * c + r16;
    float* w = Wl + u0 * WS + k;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) if (k < K && u0 + rr < OUT) pfw_adam(w + rr * WS, acc[rr], am[rr], av[rr], inv_bc2s, step_size);
  });
}
// flat index (within the layer's weight block of OUT x K) of element rr of the calling lane's tile, or -1
__device__ __forceinline__ int pfw_owned(int tid, int OUT, int K, int rr) {
  const int wave = tid >> 6, lane = tid & 63, TR = (OUT + 15) >> 4, TC = (K + 15) >> 4;
  if (wave >= TR * TC) return -1;
  const int c = wave / TR, r = wave - c * TR, u = 16 * r + 4 * (lane >> 4) + rr, k = 16 * c + (lane & 15);
  return (u < OUT && k < K) ? u * K + k : -1;
}
// b[u] -= Adam(sum_s delta[s][u]) for u < OUT <= 64: sixteen partial sums per unit, combined inside 16 neighbouring lanes; thread
// 16 u applies the step and owns the moments
__device__ __forceinline__ void pfw_bias_adam(const float* __restrict__ delta, int DS, int B, int OUT, float* __restrict__ b, float& am,
                                              float& av, float inv_bc2s, float step_size, int tid) {
  const int u = tid >> 4, part = tid & 15;
  float g = 0.f;
  if (u < OUT) for (int sr = part; sr < B; sr += 16) g += delta[sr * DS + u];
  g = row16_sum(g);
  if (part == 0 && u < OUT) pfw_adam(b + u, g, am, av, inv_bc2s, step_size);
}

template <int H>
__global__ __launch_bounds__(PFIT_THREADS) void k_policy_fit_wide(PolicyFitArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const PolicyFitWideLayout<H> L(A.n, A.m);
  const int tid = threadIdx.x, n = A.n, m = A.m, B = A.B, d = L.d();
  constexpr int MS = PFW_MS;
  const int S1 = L.S1, S2 = L.S2, M16 = L.M16;
  const bool old_net = (A.loss == 2) && !A.old_tracks_new;
  const int Bp = (B + 15) & ~15;            // rows of every sample block (rows >= B stay zero)
  float* W = lds;                           // parameters (padded layout), updated in place
  float* Wo = W + L.P;                      // old parameters (PPO with a fixed old policy)
  float* X = Wo + (old_net ? L.P : 0);      // [Bp][S1] normalised observations
  float* Xo = X + Bp * S1;                  // ... by the old network's transforms
  float* H1 = Xo + (old_net ? Bp * S1 : 0); // [Bp][S2]
  float* H2 = H1 + Bp * S2;
  float* D1 = H2 + Bp * S2;
  float* D2 = D1 + Bp * S2;
  float* MU = D2 + Bp * S2;                 // [Bp][MS] means, then dLoss/dmean in place (D3)
  float* ACT = MU + Bp * MS;                // [Bp][MS] this step's actions, then the per-row log_std terms in place
  float* MUo = ACT + Bp * MS;               // [Bp][MS] the old network's means
  float* ROW = MUo + (old_net ? Bp * MS : 0);     // [Bp][4]: adv, loss term, -, -
  float* sh = ROW + Bp * 4;                 // [8] this step's bias corrections
  float* TR = sh + 8;                       // [4][64] in-transforms, [4][32] out-transforms, [32] old log_std
  int* IDXL = (int*)(TR + 416);             // [2][64] row ids of the next two steps
  float* D3 = MU;
  float* DLS = ACT;

  for (int i = tid; i < A.lds_floats; i += PFIT_THREADS) lds[i] = 0.f;      // incl. the zero pads every operand read relies on
  __syncthreads();
  // parameters through a rolled loop (policy_fit.h: unrolled global accesses keep their addresses alive across the step loop)
#pragma nounroll
  for (int i = tid; i < d; i += PFIT_THREADS) {
    const int po = L.pad_of(i);
    W[po] = A.theta[i];
    if (old_net) Wo[po] = A.theta_old[i];
  }
  for (int f = tid; f < n; f += PFIT_THREADS) { TR[f] = A.tr[f]; TR[64 + f] = A.tr[n + f]; TR[128 + f] = A.tr_old[f]; TR[192 + f] = A.tr_old[n + f]; }
  for (int a = tid; a < m; a += PFIT_THREADS) {
    TR[256 + a] = A.tr[2 * n + a]; TR[288 + a] = A.tr[2 * n + m + a];
    TR[320 + a] = A.tr_old[2 * n + a]; TR[352 + a] = A.tr_old[2 * n + m + a];
    TR[384 + a] = (A.loss == 2) ? A.theta_old[d - m + a] : 0.f;
  }
  // the moments this lane owns: 4 elements of its tile of W1, W2 and W3 (W3's tiles sit on the last waves), and for thread 16 u
  // entry u of b1, b2, b3 and log_std
  const int T3 = ((m + 15) >> 4) * (H >> 4);
  const int fW1 = 0, fb1 = H * n, fW2 = fb1 + H, fb2 = fW2 + H * H, fW3 = fb2 + H, fb3 = fW3 + m * H, fS = fb3 + m;
  float m1[4], v1[4], m2[4], v2[4], m3[4], v3[4], mb[4], vb[4];
  {
    const int t3 = (tid + 64 * T3) & (PFIT_THREADS - 1);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int i1 = pfw_owned(tid, H, n, rr), i2 = pfw_owned(tid, H, H, rr), i3 = pfw_owned(t3, m, H, rr);
      m1[rr] = i1 >= 0 ? A.adam_m[fW1 + i1] : 0.f; v1[rr] = i1 >= 0 ? A.adam_v[fW1 + i1] : 0.f;
      m2[rr] = i2 >= 0 ? A.adam_m[fW2 + i2] : 0.f; v2[rr] = i2 >= 0 ? A.adam_v[fW2 + i2] : 0.f;
      m3[rr] = i3 >= 0 ? A.adam_m[fW3 + i3] : 0.f; v3[rr] = i3 >= 0 ? A.adam_v[fW3 + i3] : 0.f;
    }
    const int u = tid >> 4; const bool own = (tid & 15) == 0;
    const int ib[4] = {own && u < H ? fb1 + u : -1, own && u < H ? fb2 + u : -1, own && u < m ? fb3 + u : -1, own && u < m ? fS + u : -1};
#pragma unroll
    for (int e = 0; e < 4; ++e) { mb[e] = ib[e] >= 0 ? A.adam_m[ib[e]] : 0.f; vb[e] = ib[e] >= 0 ? A.adam_v[ib[e]] : 0.f; }
  }
  __syncthreads();

  double pw1 = pow(ADAM_B1D, (double)A.step0), pw2 = pow(ADAM_B2D, (double)A.step0);
  const float invB = 1.0f / (float)B;
  const float llc = 0.5f * (float)m * 1.8378770664093453f;

  // the minibatch pipeline of policy_fit.h, two stages deep: row ids of step s + 2 at the top of step s, rows of step s + 1 right after
  // this step's rows have left the registers
  constexpr int XR = 4, AR = 2;            // B n <= 64 * 64 and B m <= 64 * 32 elements over 1024 threads
  float xraw[XR], araw[AR], advraw = 0.f;
  int xsf[XR], asf[AR];                    // (row | column << 8) of the elements this thread moves, -1: none
#pragma unroll
  for (int c = 0; c < XR; ++c) { const int e = tid + PFIT_THREADS * c, r = e / n; xsf[c] = (e < B * n) ? (r | ((e - r * n) << 8)) : -1; }
#pragma unroll
  for (int c = 0; c < AR; ++c) { const int e = tid + PFIT_THREADS * c, r = e / m; asf[c] = (e < B * m) ? (r | ((e - r * m) << 8)) : -1; }
  auto fetch = [&](int64_t st) {
    const int* rows = IDXL + 64 * (int)(st & 1);
#pragma unroll
    for (int c = 0; c < XR; ++c) { if (PFIT_THREADS * c >= B * n) break; if (xsf[c] >= 0) xraw[c] = A.obs[(int64_t)rows[xsf[c] & 255] * n + (xsf[c] >> 8)]; }
#pragma unroll
    for (int c = 0; c < AR; ++c) { if (PFIT_THREADS * c >= B * m) break; if (asf[c] >= 0) araw[c] = A.act[(int64_t)rows[asf[c] & 255] * m + (asf[c] >> 8)]; }
    if (tid < B && A.loss == 2) advraw = A.adv[rows[tid]];
  };
  if (tid < B) {
    if (A.steps > 0) IDXL[tid] = A.idx[tid];
    if (A.steps > 1) IDXL[64 + tid] = A.idx[B + tid];
  }
  __syncthreads();
  if (A.steps > 0) fetch(0);
  for (int64_t step = 0; step < A.steps; ++step) {
    int next_row = 0;
    if (tid == 0) {                                        // this step's bias corrections, in double like torch's Python scalars
      pw1 *= ADAM_B1D; pw2 *= ADAM_B2D;
      sh[0] = 1.0f / (float)sqrt(1.0 - pw2);
      sh[1] = A.lr / (float)(1.0 - pw1);
    }
    if (tid < B && step + 2 < A.steps) next_row = A.idx[(step + 2) * B + tid];
    // ---- 1. the minibatch from the prefetched registers ----
#pragma unroll
    for (int c = 0; c < XR; ++c) {
      if (PFIT_THREADS * c >= B * n) break;                // (uniform)
      if (xsf[c] >= 0) {
        const int r = xsf[c] & 255, f = xsf[c] >> 8;
        X[r * S1 + f] = fast_div(xraw[c] - TR[f], TR[64 + f] + 1e-8f);
        if (old_net) Xo[r * S1 + f] = fast_div(xraw[c] - TR[128 + f], TR[192 + f] + 1e-8f);
      }
    }
#pragma unroll
    for (int c = 0; c < AR; ++c) { if (PFIT_THREADS * c >= B * m) break; if (asf[c] >= 0) ACT[(asf[c] & 255) * MS + (asf[c] >> 8)] = araw[c]; }
    if (tid < B) ROW[tid * 4] = advraw;
    if (step + 1 < A.steps) fetch(step + 1);
    __syncthreads();
    // ---- 2. forward: the new parameters, then (PPO with a fixed old policy) the old ones: Xo -> D2 -> D1 -> MUo ----
    const int K16 = (n + 15) & ~15;
#pragma nounroll
    for (int pass = 0; pass < (old_net ? 2 : 1); ++pass) {
      const float* Wp = pass ? Wo : W;
#pragma nounroll
      for (int l = 0; l < 3; ++l) {
        const float* in = l == 0 ? (pass ? Xo : X) : l == 1 ? (pass ? D2 : H1) : (pass ? D1 : H2);
        float* out = l == 0 ? (pass ? D2 : H1) : l == 1 ? (pass ? D1 : H2) : (pass ? MUo : MU);
        fit_layer(in, l == 0 ? S1 : S2, Wp + (l == 0 ? L.oW1 : l == 1 ? L.oW2 : L.oW3), l == 0 ? S1 : S2,
                  Wp + (l == 0 ? L.ob1 : l == 1 ? L.ob2 : L.ob3), B, l == 2 ? m : H, l == 0 ? K16 : H, out, l == 2 ? MS : S2, l != 2,
                  fresh(tid));
        __syncthreads();
      }
      if (pass == 0 && tid < B && step + 2 < A.steps) IDXL[64 * (int)(step & 1) + tid] = next_row;   // last read by fetch(step), a step ago
    }
    // ---- 3. loss head: one thread per (row, action), a row on 32 lanes, 32 rows a pass ----
#pragma nounroll
    for (int s0 = 0; s0 < B; s0 += 32) {
      const int ft = fresh(tid), s = s0 + (ft >> 5), a = ft & 31;
      float rloss = 0.f;                                  // this row's loss term (all 32 lanes of the row agree)
      const bool on = s < B && a < m;
      const int am = a < m ? a : 0, sm = s < B ? s : 0;
      const float x = ACT[sm * MS + am];
      const float mu = MU[sm * MS + am] * TR[288 + am] + TR[256 + am];
      if (A.loss == 0) {
        const float e = mu - x;
        if (on) D3[s * MS + a] = TR[288 + a] * (2.0f * e * invB / (float)m);
        rloss = row32_sum(on ? e * e : 0.f);
      } else {
        const float ls = W[L.oS + am], sg = expf(ls);
        const float zn = on ? (x - mu) / sg : 0.f;
        const float lln = row32_sum(-0.5f * zn * zn) - row32_sum(on ? ls : 0.f) - llc;
        float wrow;
        if (A.loss == 1) { wrow = -invB; rloss = lln; }
        else {
          const float lso = TR[384 + am];
          const float muo = old_net ? MUo[sm * MS + am] * TR[352 + am] + TR[320 + am] : mu;
          const float zo = on ? (x - muo) / expf(lso) : 0.f;
          const float llo = row32_sum(-0.5f * zo * zo) - row32_sum(on ? lso : 0.f) - llc;
          const float LR = expf(lln - llo), ad = ROW[sm * 4];
          const float s1 = LR * ad, s2 = fminf(fmaxf(LR, 1.0f - A.clip), 1.0f + A.clip) * ad;
          rloss = fminf(s1, s2);
          const bool inside = (LR >= 1.0f - A.clip) && (LR <= 1.0f + A.clip);
          wrow = (inside || s1 < s2) ? -ad * LR * invB : 0.f;
        }
        if (on) {
          D3[s * MS + a] = TR[288 + a] * (wrow * zn / sg);           // (over the mean this lane has just read)
          DLS[s * MS + a] = wrow * (zn * zn - 1.0f);                 // per-row term of dLoss/dlog_std (over the action it has read)
        }
      }
      if (on && a == 0) ROW[s * 4 + 1] = rloss;
    }
    __syncthreads();
    if (A.loss_trace && (tid >> 6) == PFIT_WAVES - 1) {     // the minibatch loss: one wave adds the rows' terms (fixed order)
      const int lane = tid & 63;
      const double lt = wave_sum(lane < B ? (double)ROW[lane * 4 + 1] : 0.0);
      if (lane == 0) A.loss_trace[step] = (A.loss == 0) ? lt / ((double)B * (double)m) : -lt / (double)B;
    }
    const float inv_bc2s = sh[0], step_size = sh[1];        // (thread 0, top of the step)
    // ---- 4a. D2 = (D3 W3) (1 - H2^2); b3 and log_std, which nothing reads before the next step ----
    fit_back(D3, MS, W + L.oW3, S2, B, M16, H, H2, S2, D2, S2, fresh(tid));
    pfw_bias_adam(D3, MS, B, m, W + L.ob3, mb[2], vb[2], inv_bc2s, step_size, fresh(tid));
    if (A.loss != 0) pfw_bias_adam(DLS, MS, B, m, W + L.oS, mb[3], vb[3], inv_bc2s, step_size, fresh(tid));
    __syncthreads();
    // ---- 4b. D1 = (D2 W2) (1 - H1^2); b2 ----
    fit_back(D2, S2, W + L.oW2, S2, B, H, H, H1, S2, D1, S2, fresh(tid));
    pfw_bias_adam(D2, S2, B, H, W + L.ob2, mb[1], vb[1], inv_bc2s, step_size, fresh(tid));
    __syncthreads();
    // ---- 4c. the three weight gradients with Adam in their epilogues (no cotangent product reads a weight any more); b1 ----
    pfw_wgrad_adam(D2, S2, H1, S2, B, H, H, W + L.oW2, S2, m2, v2, inv_bc2s, step_size, fresh(tid));
    pfw_wgrad_adam(D1, S2, X, S1, B, H, n, W + L.oW1, S1, m1, v1, inv_bc2s, step_size, fresh(tid));
    pfw_wgrad_adam(D3, MS, H2, S2, B, m, H, W + L.oW3, S2, m3, v3, inv_bc2s, step_size, (fresh(tid) + 64 * T3) & (PFIT_THREADS - 1));
    pfw_bias_adam(D1, S2, B, H, W + L.ob1, mb[0], vb[0], inv_bc2s, step_size, fresh(tid));
    __syncthreads();
  }
  // ---- write back: the parameters through a rolled loop, the moments from their owners ----
#pragma nounroll
  for (int i = tid; i < d; i += PFIT_THREADS) A.theta[i] = W[L.pad_of(i)];
  {
    const int ft = fresh(tid), t3 = (ft + 64 * T3) & (PFIT_THREADS - 1);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int i1 = pfw_owned(ft, H, n, rr), i2 = pfw_owned(ft, H, H, rr), i3 = pfw_owned(t3, m, H, rr);
      if (i1 >= 0) { A.adam_m[fW1 + i1] = m1[rr]; A.adam_v[fW1 + i1] = v1[rr]; }
      if (i2 >= 0) { A.adam_m[fW2 + i2] = m2[rr]; A.adam_v[fW2 + i2] = v2[rr]; }
      if (i3 >= 0) { A.adam_m[fW3 + i3] = m3[rr]; A.adam_v[fW3 + i3] = v3[rr]; }
    }
    const int u = ft >> 4; const bool own = (ft & 15) == 0;
    const int ib[4] = {own && u < H ? fb1 + u : -1, own && u < H ? fb2 + u : -1, own && u < m ? fb3 + u : -1,
                       own && u < m && A.loss != 0 ? fS + u : -1};          // (MSE: log_std's moments stay what they are)
#pragma unroll
    for (int e = 0; e < 4; ++e) if (ib[e] >= 0) { A.adam_m[ib[e]] = mb[e]; A.adam_v[ib[e]] = vb[e]; }
  }
}

}  // namespace mjx
