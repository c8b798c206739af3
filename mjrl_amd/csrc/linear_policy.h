// linear_policy.h -- the Gram route of the NPG / TRPO / DAPG updates for LinearPolicy (no hidden layer; n <= 63 observations, m <= 32 actions).
//
// With z_i = [x~_i ; 1] (the normalised observation and a ones column) the Hessian of mean_kl at theta_new == theta_old depends on
// the batch only through G = (1/N) sum_i z_i z_i^T: (F v)_[W|b] = diag(c) P G with c_j = 2 / (2 u_j + 1e-8) out_scale_j^2 and
// u_j = exp(log_std_j)^2, (F v)_log_std = s .* v_log_std with s_j = 4 u_j (2 u_j - 1e-8) / (2 u_j + 1e-8)^2.  So the update is one
// pass over the batch (k_lin_moments: G, the gradient and the surrogate sums), a solve that never touches the batch
// (k_lin_solve: the reference's CG in fp64 on the closed form), and one closing pass (k_lin_eval: surrogate and KL at the step).
//
// Dataflow of the two passes (v_mfma_f32_32x32x2_f32, a wave per tile of 32 rows, nothing shared between waves in the row loop):
//   stage    a tile's 32 n observations are one contiguous run of the batch: the wave loads it lane after lane (coalesced, into
//            registers, one tile AHEAD: the loads are issued in front of the reduction MFMAs of the tile before), normalises and
//            writes Z (32 x NP, row stride NP + 4, the ones column at n, zeros behind; a row beyond N is all zeros) to its own LDS.
//   forward  mu[row][action]: A = Z (the lane's row, k-slot hi of step (q, t) carries feature 8 q + 4 hi + t: one ds_read_b128 per
//            four steps), B = the [W | b] image of LDS in the same k order.  Only the quads up to feature n are walked.
//   head     in the accumulator layout: register r of lane (hi, j) is row unit_of(r, hi), action j.  Pass 1 forms D = adv (a - mu)
//            out_scale / u there; the closing pass the per-action terms of LL_new - LL_old and of the KL, summed over the 32 lanes
//            of a half by DPP.
//   reduce   (pass 1) the k dimension is the ROWS: step (q, r) pairs rows 8 q + r and 8 q + 4 + r -- the two lane halves of
//            accumulator register 4 q + r, so the D register is the B operand of Z^T D as it lies; A is Z read down a column
//            (lane j: feature j of the block, conflict-free).  The same Z value is both operands of the Gram step mfma(z, z, G).
//            NP = 64: two feature blocks, the three distinct Gram blocks 00, 01, 11 (10 is 01 transposed: the reduction mirrors it).
//
// Summation order.  A wave owns one CHAIN of at most 32 tiles (1024 rows): its MFMA accumulators are the only fp32 sums over
// rows.  At the chain's end it writes them as they lie (register images, 64 floats per store) to its slab; k_lin_reduce adds the
// slabs in fp64, chain groups of 16 in chain order and then the 16 groups in order, and mirrors / transposes into the moment
// block.  The sums that need no MFMA (d log_std, sum adv, the closing pass's two sums) are fp64 per lane from the first row on.
// No atomics: the chain split depends on N and the CU count alone, so two calls give the same bits.  (Decision: a slab per chain
// and a reduction kernel rather than fp64 register images -- 96 accumulator registers would need 192 more, and the slab costs
// 8 to 20 KB per 16 to 32 tiles of input, under a tenth of what the pass reads.)
//
// The closing pass forwards [W_new | b_new] and the DIFFERENCE image [W_new - W_old | b_new - b_old] on the same Z tile: mu_old -
// mu_new comes out of its own MFMA chain instead of the difference of two means (the KL is its square).  Both policies are taken
// through tr_new: the route starts from old_is_new, where the two transforms hold the same values.
//
// TRPO and DAPG run on the same route (update_host.h trpo_update_gram / dapg_update_gram).
//   DAPG  the gradient runs over [on-policy ; demonstration] rows, the metric over the on-policy prefix (dapg.py:97-103): pass 1
//         is launched as two row SEGMENTS into one slab / ds array, on-policy chains first.  k_lin_moments<NB, true> takes rows
//         [0, rows_on); k_lin_moments<NB, false> -- the same tile loop without the Gram steps, only the gradient blocks of its
//         slab written -- takes the rows behind them on offset pointers with its own row count, so its tiles start at row rows_on
//         whatever that is modulo 32 and its last tile is zero-filled behind the segment's end.  Each segment's chain split is the
//         rule above applied to its own row count: no chain straddles the boundary.  k_lin_reduce sums the G elements over the
//         on-policy chains only (the order above over those chains), everything else over all chains.  The surrogate slot holds
//         sum adv_on (LinArgs::adv_sum: the whitened on-policy advantages, not the first rows_on bound ones), the rows slot N_on.
//         The solve divides G by N_on and forms the gradient as sum / N_all x (N_all / N_on) in fp64; mjx_dapg_update applies
//         that factor as one fp32 product per element -- 6e-8 relative, inside TOL_VPG / TOL_STEP.
//   TRPO  the mean KL of a trial step is a closed form in G, so k_lin_solve<LIN_SOLVE_TRPO> decides all of the reference's 100
//         backtracking trials in LDS behind the CG (the comment there); k_lin_eval runs once, at the final theta_out.  Its batch
//         KL is what is logged; where it and the closed form disagree about kl_dist by rounding, the closed form stands.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_prims.h"
#include "vecops.h"

namespace mjx {

constexpr int LIN_MAX_N = 63, LIN_MAX_M = 32;
constexpr int LIN_WAVES = 4;                 // waves per workgroup of the two passes
constexpr int LIN_CHAIN_TILES = 32;          // tiles of 32 rows per chain at the most: no fp32 sum is longer than 1024 rows
constexpr int LIN_DS = 68;                   // doubles per chain beside the slab: d log_std per lane (64) | sum adv per half (2) | rows | 0
constexpr int LIN_SOLVE_NT = 1024;

// LDS of k_lin_moments / k_lin_eval in floats: image 0 ([W | b], 32 x S) | image 1 (the difference image, closing pass) |
// in_shift NP | in_scale + 1e-8 NP | out_scale, out_shift, sigma_new (closing pass: 1 / sigma_new), 1 / sigma_old, 1 / sigma_new - 1 / sigma_old: 32 each | Z of each wave.
// The moment block in doubles: G (NP x NP) | g_[W|b] (m x NP) | g_log_std (m) | sum LR adv, rows, 0, 0.
struct LinLayout {
  int NP, S, NB;
  __host__ __device__ constexpr explicit LinLayout(int n = 1) : NP(n + 1 <= 32 ? 32 : 64), S(NP + 4), NB(NP / 32) {}
  // the wide route (linear_policy_wide.h, 64 <= n <= 127): three or four feature blocks, everything below by the same arithmetic
  static __host__ __device__ constexpr LinLayout wide(int n) { LinLayout L; L.NP = n + 1 <= 96 ? 96 : 128; L.S = L.NP + 4; L.NB = L.NP / 32; return L; }
  __host__ __device__ constexpr int img() const { return 32 * S; }
  __host__ __device__ constexpr int off_vec() const { return 2 * img(); }
  __host__ __device__ constexpr int off_z() const { return off_vec() + 2 * NP + 5 * 32; }
  __host__ __device__ constexpr int floats() const { return off_z() + LIN_WAVES * img(); }
  __host__ __device__ constexpr size_t bytes() const { return sizeof(float) * (size_t)floats(); }
  __host__ __device__ constexpr int acc_blocks() const { return NB == 1 ? 2 : 5; }            // G00, gA0 | G00, G01, G11, gA0, gA1
  __host__ __device__ constexpr int slab_floats() const { return acc_blocks() * 16 * 64; }
  __host__ __device__ constexpr int64_t block_count(int m) const { return (int64_t)NP * NP + (int64_t)m * NP + m + 4; }
  // k_lin_solve's LDS in doubles: G | g, x, r, p, z (m NP + m each) | c, s (32 each) | the block sums' 32
  __host__ __device__ constexpr size_t solve_bytes(int m) const { return sizeof(double) * ((size_t)NP * NP + 5 * ((size_t)m * NP + m) + 96); }
};
static_assert(LinLayout(63).bytes() <= 64 * 1024 && LinLayout(31).NP == 32 && LinLayout(32).NP == 64, "the passes fit the default LDS");
static_assert(LinLayout(63).solve_bytes(32) <= 160 * 1024, "the solve fits LDS");

struct LinRoute { int route, NP; size_t lds; int chain_rows; };
inline LinRoute linear_route(int n, int m, int n_hidden, bool on) {
  if (!on || n_hidden != 0 || n > LIN_MAX_N || m > LIN_MAX_M) return LinRoute{0, 0, 0, 0};
  const LinLayout L(n);
  return LinRoute{1, L.NP, L.bytes(), 32 * LIN_CHAIN_TILES};
}

struct LinArgs {
  const float *obs, *act, *adv;
  int64_t N;
  int n, m;
  const float *theta, *theta_old, *tr;       // theta_old: closing pass only
  int chain_tiles;
  int64_t chains;
  float* slab;                               // pass 1: chains x slab_floats
  double* ds;                                // pass 1: chains x LIN_DS; closing pass: chains x 4
  const float* adv_sum = nullptr;            // pass 1, optional: the vector whose sum goes to the surrogate-sum slot (null: adv)
};

__device__ __forceinline__ float lin_sum32(float v) {        // every lane: the sum over its 32-lane half
  v = row16_sum(v);
  auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}

// all 256 threads, before the barrier: the images and the per-column / per-action vectors (IM: images in front of the vectors;
// the wide route's pass 1 keeps one)
template <bool EVAL, int IM = 2>
__device__ __forceinline__ void lin_stage_policy(float* lds, const LinLayout L, const LinArgs& a, int tid) {
  const int lane = tid & 63, n = a.n, m = a.m, oB = m * n, oS = oB + m;
  float* w0 = lds; float* w1 = lds + L.img(); float* vec = lds + IM * L.img();
  for (int u = tid >> 6; u < 32; u += LIN_WAVES)
    for (int c = lane; c < L.S; c += 64) {
      const int i = c < n ? u * n + c : oB + u;
      const bool on = u < m && c <= n;
      const float wn = on ? a.theta[i] : 0.f;
      w0[u * L.S + c] = wn;
      if (EVAL) w1[u * L.S + c] = on ? wn - a.theta_old[i] : 0.f;
    }
  for (int c = tid; c < L.NP; c += 64 * LIN_WAVES) {
    vec[c] = c < n ? a.tr[c] : 0.f;
    vec[L.NP + c] = c < n ? a.tr[n + c] + 1e-8f : 1.f;
  }
  float* pa = vec + 2 * L.NP;
  for (int i = tid; i < 32; i += 64 * LIN_WAVES) {
    const bool on = i < m;
    const float lsn = on ? a.theta[oS + i] : 0.f, lso = (on && EVAL) ? a.theta_old[oS + i] : lsn;
    pa[i] = on ? a.tr[2 * n + m + i] : 0.f;           // out_scale
    pa[32 + i] = on ? a.tr[2 * n + i] : 0.f;          // out_shift
    // (closing pass: 1 / sigma_new, 1 / sigma_old and their DIFFERENCE, formed in fp64: z_new - z_old is built from the difference)
    const double isn = exp(-(double)lsn), iso = exp(-(double)lso);
    pa[64 + i] = on ? (EVAL ? (float)isn : expf(lsn)) : 1.f;
    pa[96 + i] = on ? (float)iso : 1.f;
    pa[128 + i] = on ? (float)(isn - iso) : 0.f;
  }
}

// One tile ahead in registers: LE loads of the observations (element lane + 64 i of the tile's run), the lane's action column
// and the advantages of its 16 accumulator rows.  Nothing outside [0, N) is read.
template <int LE>
struct LinTile { float o[LE]; float act[16]; float adv[16]; };

template <int LE>
__device__ __forceinline__ void lin_load_tile(LinTile<LE>& t, const LinArgs& a, int64_t row0, int lane) {
  const int j = lane & 31, hi = lane >> 5;
  const int64_t base = row0 * a.n, lim = a.N * a.n;
  const int cnt = 32 * a.n;
#pragma unroll
  for (int i = 0; i < LE; ++i) {
    const int e = lane + 64 * i;
    t.o[i] = (e < cnt && base + e < lim) ? a.obs[base + e] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t gr = row0 + unit_of(r, hi);
    const bool valid = gr < a.N;
    t.act[r] = (valid && j < a.m) ? a.act[gr * a.m + j] : 0.f;
    t.adv[r] = valid ? a.adv[gr] : 0.f;
  }
}

// the loaded run, normalised, into the wave's Z; (row, f) of the lane's first element and the step of 64 elements are the caller's
template <int LE>
__device__ __forceinline__ void lin_write_tile(float* Z, const LinLayout L, const float* vec, const LinTile<LE>& t, const LinArgs& a,
                                               int64_t row0, int lane, int row_l, int f_l, int q64, int r64) {
  const int cnt = 32 * a.n;
  int row = row_l, f = f_l;
#pragma unroll
  for (int i = 0; i < LE; ++i) {
    const int e = lane + 64 * i;
    if (e < cnt) Z[row * L.S + f] = (row0 + row < a.N) ? (t.o[i] - vec[f]) / vec[L.NP + f] : 0.f;
    f += r64; row += q64;
    if (f >= a.n) { f -= a.n; ++row; }
  }
  if (lane < 32) Z[lane * L.S + a.n] = (row0 + lane < a.N) ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------- pass 1
// GRAM = false (a row segment that feeds the gradient only -- DAPG's demonstrations): the same tile loop without the G00 / G01 /
// G11 steps; only the gradient blocks of the slab are written, and the chain's surrogate-sum and row-count slots hold 0.
template <int NB, bool GRAM = true>
__global__ __launch_bounds__(64 * LIN_WAVES) void k_lin_moments(const LinArgs a) {
  extern __shared__ float lin_lds[];
  constexpr int LE = 16 * NB;                         // 32 n / 64 loads per lane: n <= 31 -> 16, n <= 63 -> 32
  const LinLayout L(a.n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hi = lane >> 5;
  lin_stage_policy<false>(lin_lds, L, a, tid);
  float* Z = lin_lds + L.off_z() + wave * L.img();
  for (int i = lane; i < L.img(); i += 64) Z[i] = 0.f;
  __syncthreads();
  const int64_t chain = (int64_t)blockIdx.x * LIN_WAVES + wave;
  if (chain >= a.chains) return;
  const float* w0 = lin_lds; const float* vec = lin_lds + L.off_vec(); const float* pa = vec + 2 * L.NP;
  const float osc = pa[j], osh = pa[32 + j], sg = pa[64 + j];
  const int row_l = lane / a.n, f_l = lane - row_l * a.n, q64 = 64 / a.n, r64 = 64 - q64 * a.n;
  const int nq = (a.n + 8) >> 3;                      // quads of 8 features that reach the ones column
  const int64_t tile0 = chain * a.chain_tiles, tiles = (a.N + 31) >> 5;
  const int64_t tile1 = tile0 + a.chain_tiles < tiles ? tile0 + a.chain_tiles : tiles;

  f32x16 G00 = (f32x16)(0.f), G01 = (f32x16)(0.f), G11 = (f32x16)(0.f), gA0 = (f32x16)(0.f), gA1 = (f32x16)(0.f);
  double gls = 0.0, sadv = 0.0, sadv2 = 0.0;
  LinTile<LE> t;
  lin_load_tile(t, a, tile0 * 32, lane);
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t row0 = tile * 32;
    // (adv_sum: row `lane` of the tile, one coalesced load, added behind the MFMAs below)
    const float w2 = (GRAM && a.adv_sum && lane < 32 && row0 + lane < a.N) ? a.adv_sum[row0 + lane] : 0.f;
    lin_write_tile(Z, L, vec, t, a, row0, lane, row_l, f_l, q64, r64);
    wave_sync();
    // forward
    f32x16 mu = (f32x16)(0.f);
    const float* zrow = &Z[j * L.S + 4 * hi];
    const float* wrow = &w0[j * L.S + 4 * hi];
#pragma unroll
    for (int q = 0; q < 4 * NB; ++q) {
      if (q < nq) {
        const f32x4 z4 = *(const f32x4*)(zrow + 8 * q), w4 = *(const f32x4*)(wrow + 8 * q);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) mu = MJX_MFMA(z4[tt], w4[tt], mu);
      }
    }
    // head: D in the accumulator layout
    f32x16 D;
    const int left = (int)(a.N - row0 < 32 ? a.N - row0 : 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool valid = unit_of(r, hi) < left, ok = valid && j < a.m;
      const float mn = mu[r] * osc + osh;
      const float zn = ok ? (t.act[r] - mn) / sg : 0.f;
      const float w = t.adv[r];                       // (0 beyond N)
      D[r] = ok ? osc * (w * zn / sg) : 0.f;
      if (ok) gls += (double)(w * (zn * zn - 1.0f));
      if (j == 0) sadv += (double)w;
    }
    if (tile + 1 < tile1) lin_load_tile(t, a, row0 + 32, lane);      // in flight under the MFMAs below
    // Z^T [Z | D] over the tile's rows
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* zc = &Z[(8 * q + 4 * hi + r) * L.S + j];
        const float z0 = zc[0];
        if (GRAM) G00 = MJX_MFMA(z0, z0, G00);
        gA0 = MJX_MFMA(z0, D[4 * q + r], gA0);
        if (NB == 2) {
          const float z1 = zc[32];
          if (GRAM) { G01 = MJX_MFMA(z0, z1, G01); G11 = MJX_MFMA(z1, z1, G11); }
          gA1 = MJX_MFMA(z1, D[4 * q + r], gA1);
        }
      }
    }
    sadv2 += (double)w2;
    wave_sync();
  }
  // the chain's register images
  float* sl = a.slab + chain * L.slab_floats() + lane;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (GRAM) sl[(0 * 16 + r) * 64] = G00[r];
    if (NB == 1) sl[(1 * 16 + r) * 64] = gA0[r];
    else {
      if (GRAM) { sl[(1 * 16 + r) * 64] = G01[r]; sl[(2 * 16 + r) * 64] = G11[r]; }
      sl[(3 * 16 + r) * 64] = gA0[r]; sl[(4 * 16 + r) * 64] = gA1[r];
    }
  }
  double* ds = a.ds + chain * LIN_DS;
  ds[lane] = gls;
  if (!GRAM) {
    if (lane < 4) ds[64 + lane] = 0.0;
    return;
  }
  if (a.adv_sum) {                                   // (uniform: every lane of the wave takes the same side)
    const double s2 = wave_sum(sadv2);
    if (lane < 2) ds[64 + lane] = lane == 0 ? s2 : 0.0;
  } else if (j == 0) {
    ds[64 + hi] = sadv;
  }
  if (lane == 0) { const int64_t r1 = tile1 * 32 < a.N ? tile1 * 32 : a.N; ds[66] = (double)(r1 - tile0 * 32); ds[67] = 0.0; }
}

// block[e] = the fp64 sum over the chains of what the slabs hold for element e: 16 elements x 16 chain groups per workgroup, a
// group adds its chains in chain order, then the groups are added in order.  The G elements are summed over the first chains_g
// chains only (a segmented pass: the chains of the GRAM = true segment come first; otherwise chains_g == chains).
__global__ __launch_bounds__(256) void k_lin_reduce(const float* __restrict__ slab, const double* __restrict__ ds, int64_t chains, int64_t chains_g,
                                                    int n, int m, double* __restrict__ block) {
  __shared__ double sh[16][17];
  const LinLayout L(n);
  const int el = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int64_t e = (int64_t)blockIdx.x * 16 + el, nG = (int64_t)L.NP * L.NP, nA = nG + (int64_t)m * L.NP, cnt = L.block_count(m);
  double acc = 0.0;
  if (e < nA) {
    int blk, i, jj;
    if (e < nG) {
      int k1 = (int)(e / L.NP), k2 = (int)(e % L.NP);
      if ((k1 >> 5) > (k2 >> 5)) { const int s = k1; k1 = k2; k2 = s; }        // block 10 is block 01 transposed
      blk = L.NB == 1 ? 0 : (k1 >> 5) + (k2 >> 5);
      i = k1 & 31; jj = k2 & 31;
    } else {
      const int act = (int)((e - nG) / L.NP), k = (int)((e - nG) % L.NP);
      blk = (L.NB == 1 ? 1 : 3) + (k >> 5);
      i = k & 31; jj = act;
    }
    const int off = (blk * 16 + (i & 3) + 4 * (i >> 3)) * 64 + 32 * ((i >> 2) & 1) + jj;      // register, lane half, column
    const size_t SL = (size_t)L.slab_floats();
    const int64_t cn = e < nG ? chains_g : chains;
    for (int64_t c = grp; c < cn; c += 16) acc += (double)slab[c * SL + off];
  } else if (e < cnt) {
    const int k = (int)(e - nA);
    for (int64_t c = grp; c < chains; c += 16) {
      const double* d = ds + c * LIN_DS;
      if (k < m) { acc += d[k]; acc += d[32 + k]; }
      else if (k == m) { acc += d[64]; acc += d[65]; }
      else if (k == m + 1) acc += d[66];
    }
  }
  sh[grp][el] = acc;
  __syncthreads();
  if (grp == 0 && e < cnt) {
    double t = 0.0;
    for (int g = 0; g < 16; ++g) t += sh[g][el];
    block[e] = t;
  }
}

__global__ void k_lin_zero(double* p, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) p[i] = 0.0;
}

// ---------------------------------------------------------------------------- the solve
// One workgroup: cg_solve.py:3-22 in fp64 with A p = [diag(c) P G | s .* p_log_std] + damping p (G and g divided by N here),
// then g.x, the step length and the stepped parameters as k_apply_npg_step / k_apply_step form them.  Vectors are kept in the
// padded layout [m x NP | m]; a padded column meets zero rows of G and a zero gradient and stays exactly 0.
//
// MODE LIN_SOLVE_DAPG: the gradient is the block's sum / N_all x (N_all / N_on) in fp64 (dapg.py:97-98; mjx_dapg_update forms the
// quotient in fp64 too but applies it as one fp32 product per element: a relative 6e-8 apart, inside TOL_VPG = 3e-6), G / N_on.
//
// MODE LIN_SOLVE_TRPO: TRPO's backtracking line search (trpo.py:107-126) behind the CG, without the batch.  mu_old - mu_new =
// out_scale .* (Delta z) with Delta = [W_new - W_old | b_new - b_old], so the mean KL of a trial is
//   KL_t = sum_j [(out_scale_j^2 Delta_j^T G Delta_j + u_old,j - u_new,j) / (2 u_new,j + 1e-8) + ls_new,j - ls_old,j],  u = exp(ls)^2
// (gaussian_mlp.py:135-145).  Trial t: every thread forms its padded elements of theta_t = step_add(theta, (float)alpha_t,
// (float)x) with the clamp -- the fp32 values the epilogue would store -- and leaves Delta (fp64, exact) in the CG's r; after a
// barrier element (j, k) forms (Delta_j G)_k Delta_jk / (2 u_new,j + 1e-8) out_scale_j^2 like the CG's P G product, a log_std
// element its three terms, and one block_sum gives KL_t to every thread.  KL_t < kl_dist accepts; else alpha <- 0.9 alpha (fp64,
// cast per trial: what k_trpo_try / k_trpo_check carry).  After max_trials rejections the step is zero.  results[9..12] and the
// ring are mjx_trpo_update's ([17 + 2 (k % 24)] = KL_t x N_global: a sum, like a K3 pass leaves there); the surrogate slots
// [16 + 2 (k % 24)] hold NaN (no trial's surrogate is evaluated).  The closing pass at the final theta_out gives the batch KL
// that is logged; where it and KL_t disagree about kl_dist by rounding, the closed form has decided.
enum { LIN_SOLVE_NPG = 0, LIN_SOLVE_TRPO = 1, LIN_SOLVE_DAPG = 2 };
struct LinSolveArgs {
  const double* block;
  int n, m, iters;
  double inv_N, damping, tol, step_size, const_alpha;        // const_alpha: NaN = the NPG step length
  float min_log_std;
  const float *theta, *tr;
  float *grad_out, *x_out, *theta_out;
  double* results;
  double g_scale = 0.0;                                      // DAPG: 1 / N_all x (N_all / N_on), what the gradient sums are multiplied by
  double kl_dist = 0.0, N_global = 0.0;                      // TRPO
  int max_trials = 0;
};

template <int MODE>
__global__ __launch_bounds__(LIN_SOLVE_NT) void k_lin_solve(const LinSolveArgs a) {
  extern __shared__ double lin_sol[];
  const LinLayout L(a.n);
  const int NP = L.NP, n = a.n, m = a.m, MN = m * NP, E = MN + m, oB = m * n, oS = oB + m, tid = threadIdx.x;
  double* G = lin_sol; double* gv = G + NP * NP; double* x = gv + E; double* r = x + E; double* p = r + E; double* z = p + E;
  double* cv = z + E; double* sv = cv + 32; double* sh = sv + 32;
  for (int i = tid; i < NP * NP; i += LIN_SOLVE_NT) G[i] = a.block[i] * a.inv_N;
  for (int e = tid; e < E; e += LIN_SOLVE_NT) {
    const double g = a.block[NP * NP + e] * (MODE == LIN_SOLVE_DAPG ? a.g_scale : a.inv_N);
    gv[e] = g; x[e] = 0.0; r[e] = g; p[e] = g;
  }
  if (tid < m) {
    const double sg = exp((double)a.theta[oS + tid]), u = sg * sg, eps = 1e-8, osc = (double)a.tr[2 * n + m + tid];
    cv[tid] = 2.0 / (2.0 * u + eps) * osc * osc;
    sv[tid] = 4.0 * u * (2.0 * u - eps) / ((2.0 * u + eps) * (2.0 * u + eps));
  }
  __syncthreads();
  auto dot = [&](const double* u, const double* v) {
    double s = 0.0;
    for (int e = tid; e < E; e += LIN_SOLVE_NT) s += u[e] * v[e];
    return block_sum(s, sh);
  };
  double rdotr = dot(r, r);
  for (int it = 0; it < a.iters; ++it) {
    for (int e = tid; e < E; e += LIN_SOLVE_NT) {
      if (e < MN) {
        const int act = e / NP, k = e - act * NP;
        double s = 0.0;
        for (int kk = 0; kk < NP; ++kk) s += p[act * NP + kk] * G[kk * NP + k];
        z[e] = cv[act] * s + a.damping * p[e];
      } else {
        z[e] = sv[e - MN] * p[e] + a.damping * p[e];
      }
    }
    __syncthreads();
    const double al = rdotr / dot(p, z);
    for (int e = tid; e < E; e += LIN_SOLVE_NT) { x[e] += al * p[e]; r[e] -= al * z[e]; }
    __syncthreads();
    const double nw = dot(r, r);
    for (int e = tid; e < E; e += LIN_SOLVE_NT) p[e] = r[e] + (nw / rdotr) * p[e];
    rdotr = nw;
    __syncthreads();
    if (rdotr < a.tol) break;                          // (every thread holds the same sum)
  }
  const double gx = dot(gv, x);
  const bool npg = a.const_alpha != a.const_alpha;
  const double a64 = npg ? sqrt(fabs(a.step_size / (gx + 1e-20))) : a.const_alpha;
  float alpha = (float)a64;
  if (tid == 0) { a.results[8] = gx; if (npg) a.results[9] = a64; }
  if (tid < 4) a.results[4 + tid] = a.block[L.block_count(m) - 4 + tid];
  if (MODE == LIN_SOLVE_TRPO) {
    // r: Delta (log_std elements: the new log_std itself); cv: out_scale^2; sv: 1 / (2 u_new + 1e-8) of the trial
    double* dl = r;
    __syncthreads();
    if (tid < m) { const double osc = (double)a.tr[2 * n + m + tid]; cv[tid] = osc * osc; }
    double at = a64, tried = a64;
    int trials = 0;
    bool accepted = false;
    while (trials < a.max_trials && !accepted) {
      const float af = (float)at;
      for (int e = tid; e < E; e += LIN_SOLVE_NT) {
        if (e < MN) {
          const int act = e / NP, k = e - act * NP;
          double d = 0.0;
          if (k <= n) {
            const float th = a.theta[k < n ? act * n + k : oB + act];
            d = (double)step_add(th, af, (float)x[e]) - (double)th;
          }
          dl[e] = d;
        } else {
          const double ln = (double)fmaxf(step_add(a.theta[oS + e - MN], af, (float)x[e]), a.min_log_std), sg = exp(ln);
          dl[e] = ln;
          sv[e - MN] = 1.0 / (2.0 * sg * sg + 1e-8);
        }
      }
      __syncthreads();
      double s = 0.0;
      for (int e = tid; e < E; e += LIN_SOLVE_NT) {
        if (e < MN) {
          const int act = e / NP, k = e - act * NP;
          double q = 0.0;
          for (int kk = 0; kk < NP; ++kk) q += dl[act * NP + kk] * G[kk * NP + k];
          s += cv[act] * sv[act] * (q * dl[e]);
        } else {
          const double lo = (double)a.theta[oS + e - MN], so = exp(lo), sn = exp(dl[e]);
          s += (so * so - sn * sn) * sv[e - MN] + dl[e] - lo;
        }
      }
      const double kl = block_sum(s, sh);               // (every thread holds the same sum; its barriers also free dl / sv for the next trial)
      if (tid == 0) { a.results[16 + 2 * (trials % 24)] = nan(""); a.results[17 + 2 * (trials % 24)] = kl * a.N_global; }
      ++trials;
      tried = at;
      if (kl < a.kl_dist) accepted = true;
      else at = 0.9 * at;
    }
    alpha = accepted ? (float)tried : 0.f;
    if (tid == 0) { a.results[9] = tried; a.results[10] = accepted ? 1.0 : 0.0; a.results[11] = (double)trials; a.results[12] = at; }
  }
  for (int e = tid; e < E; e += LIN_SOLVE_NT) {
    int i;
    if (e < MN) {
      const int act = e / NP, k = e - act * NP;
      if (k > n) continue;
      i = k < n ? act * n + k : oB + act;
    } else {
      i = oS + (e - MN);
    }
    const float xf = (float)x[e];
    a.grad_out[i] = (float)gv[e];
    a.x_out[i] = xf;
    float v = step_add(a.theta[i], alpha, xf);
    if (i >= oS) v = fmaxf(v, a.min_log_std);
    a.theta_out[i] = v;
  }
}

// ---------------------------------------------------------------------------- the closing pass
// (Tile, WIDE: the wide route, linear_policy_wide.h, runs this kernel at NB = 3 / 4 on LinLayout::wide with its row-wise
// LinTileW, whose lin_load_tile / lin_write_tile overloads are found at instantiation)
template <int NB, class Tile = LinTile<16 * NB>, bool WIDE = false>
__global__ __launch_bounds__(64 * LIN_WAVES) void k_lin_eval(const LinArgs a) {
  extern __shared__ float lin_lds[];
  const LinLayout L = WIDE ? LinLayout::wide(a.n) : LinLayout(a.n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hi = lane >> 5;
  lin_stage_policy<true>(lin_lds, L, a, tid);
  float* Z = lin_lds + L.off_z() + wave * L.img();
  for (int i = lane; i < L.img(); i += 64) Z[i] = 0.f;
  __syncthreads();
  const int64_t chain = (int64_t)blockIdx.x * LIN_WAVES + wave;
  if (chain >= a.chains) return;
  const float* w0 = lin_lds; const float* w1 = lin_lds + L.img(); const float* vec = lin_lds + L.off_vec(); const float* pa = vec + 2 * L.NP;
  const float osc = pa[j], osh = pa[32 + j], rn = pa[64 + j], ro = pa[96 + j], rd = pa[128 + j];
  const float rkl = j < a.m ? (float)(1.0 / (2.0 * exp(2.0 * (double)a.theta[a.m * a.n + a.m + j]) + 1e-8)) : 0.f;
  double dsum64 = 0.0;
  for (int k = 0; k < a.m; ++k) dsum64 += (double)a.theta[a.m * a.n + a.m + k] - (double)a.theta_old[a.m * a.n + a.m + k];
  const float dsum = (float)dsum64;
  const int row_l = lane / a.n, f_l = lane - row_l * a.n, q64 = 64 / a.n, r64 = 64 - q64 * a.n;
  const int nq = (a.n + 8) >> 3;
  const int64_t tile0 = chain * a.chain_tiles, tiles = (a.N + 31) >> 5;
  const int64_t tile1 = tile0 + a.chain_tiles < tiles ? tile0 + a.chain_tiles : tiles;

  double ssurr = 0.0, skl = 0.0;
  Tile t;
  lin_load_tile(t, a, tile0 * 32, lane);
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t row0 = tile * 32;
    lin_write_tile(Z, L, vec, t, a, row0, lane, row_l, f_l, q64, r64);
    wave_sync();
    f32x16 yn = (f32x16)(0.f), dy = (f32x16)(0.f);
    const float* zrow = &Z[j * L.S + 4 * hi];
    const float* wrow = &w0[j * L.S + 4 * hi];
    const float* drow = &w1[j * L.S + 4 * hi];
#pragma unroll
    for (int q = 0; q < 4 * NB; ++q) {
      if (q < nq) {
        const f32x4 z4 = *(const f32x4*)(zrow + 8 * q), w4 = *(const f32x4*)(wrow + 8 * q), d4 = *(const f32x4*)(drow + 8 * q);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) { yn = MJX_MFMA(z4[tt], w4[tt], yn); dy = MJX_MFMA(z4[tt], d4[tt], dy); }
      }
    }
    wave_sync();                                       // (Z is free: the next tile may be written)
    float act[16], adv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { act[r] = t.act[r]; adv[r] = t.adv[r]; }
    if (tile + 1 < tile1) lin_load_tile(t, a, row0 + 32, lane);      // in flight under the head
    const int left = (int)(a.N - row0 < 32 ? a.N - row0 : 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool valid = unit_of(r, hi) < left, ok = valid && j < a.m;
      const float mn = yn[r] * osc + osh, dm = dy[r] * osc;          // dm = mu_new - mu_old
      // z_new - z_old = an (1 / sigma_new - 1 / sigma_old) - dm / sigma_old: two small products, not the difference of two z of
      // size ~2 (whose roundings, ~2e-7, times z_new + z_old, times a likelihood ratio in the hundreds, were what a 32-action
      // case's surrogate missed its bar by); z_new + z_old = 2 z_new - (z_new - z_old)
      const float an = act[r] - mn, zn = an * rn;
      const float dz = an * rd - dm * ro;
      const float dll = lin_sum32(ok ? -0.5f * dz * (2.0f * zn - dz) : 0.f) - dsum;
      const float kl = lin_sum32(ok ? dm * dm * rkl : 0.f);            // (the row-independent part of the KL: k_lin_eval_reduce, fp64)
      if (j == 0 && valid) { ssurr += (double)(expf(dll) * adv[r]); skl += (double)kl; }
    }
  }
  if (j == 0) { a.ds[chain * 4 + 2 * hi] = ssurr; a.ds[chain * 4 + 2 * hi + 1] = skl; }
}

// res[0] = sum LR adv, res[1] = sum KL over the chains (thread t adds chains t, t + 256, ... in order, lane half 0 before 1; then
// the block's fixed order); res[2] = res[3] = 0.  The KL's row-independent part, sum_j (u_old - u_new) / (2 u_new + 1e-8) + log_std_new
// - log_std_old, is two terms of size ~delta that cancel to delta^2: formed here once in fp64 and added `rows` times.  (In the
// row loop's fp32 it was an error of ~1e-7 per action that no sum over rows averages out: 6e-6 of the KL at 70 001 rows.)
__global__ __launch_bounds__(256) void k_lin_eval_reduce(const double* __restrict__ part, int64_t chains, const float* __restrict__ ls_new,
                                                         const float* __restrict__ ls_old, int m, double rows, double* __restrict__ res) {
  __shared__ double sh[17];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t c = threadIdx.x; c < chains; c += 256) {
    const double* d = part + c * 4;
    s0 += d[0]; s0 += d[2]; s1 += d[1]; s1 += d[3];
  }
  s0 = block_sum(s0, sh);
  s1 = block_sum(s1, sh);
  if (threadIdx.x == 0) {
    double kc = 0.0;
    for (int j = 0; j < m; ++j) {
      const double ln = (double)ls_new[j], lo = (double)ls_old[j], un = exp(2.0 * ln), uo = exp(2.0 * lo);
      kc += (uo - un) / (2.0 * un + 1e-8) + ln - lo;
    }
    res[0] = s0; res[1] = s1 + rows * kc; res[2] = 0.0; res[3] = 0.0;
  }
}

}  // namespace mjx
