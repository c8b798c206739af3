// linear_policy_wide.h -- the Gram route of linear_policy.h for 64 <= n <= 127 observations (m <= 32 actions; NPG and TRPO).
//
// The mathematics, the moment block, the staging of a tile and the closing pass are linear_policy.h's (LinLayout::wide: NP = 96
// or 128, three or four feature blocks of 32).  Two things are divided differently.
//
// Pass 1 (k_lin_moments_wide).  G has NB (NB + 1) / 2 distinct 32 x 32 blocks: 10 at NB = 4.  A wave that kept all of them beside
// its gradient blocks and mu would need 240 accumulator registers, so here a WORKGROUP shares them.  A round is 128 rows: each of
// the four waves stages its own tile of 32 rows into its Z of LDS (tile-ahead loads, as in k_lin_moments), forwards it, forms D in
// the accumulator layout and adds its NB gradient blocks Z^T D -- all of that on its own rows, with no other wave involved.
// After a barrier the distinct Gram blocks, dealt out over the waves (block id w, w + 4, w + 8 to wave w: 3, 3, 2, 2 at NB = 4 and
// 2, 2, 1, 1 at NB = 3), are reduced over ALL FOUR tiles of the round: A is Z read down a column of block bi, B is Z read down
// a column of block bj (one read serves both on a diagonal block).  A second barrier frees the tiles for the next round.
// Per wave: 16 (mu) + 16 (D) + 16 NB (gradient) + 48 (Gram) accumulator registers at the most.
//
// Summation order.  A workgroup owns one chain of at most 8 rounds (1024 rows): no fp32 sum runs over more rows.  At the chain's
// end the Gram images go to the slab as they lie; the four waves' gradient images (256 rows each) are added through the free Z
// tiles, wave 0 to 3 in order, and go to the slab once.  k_lin_reduce_wide adds the slabs in fp64 in k_lin_reduce's order and
// mirrors the blocks below the diagonal.  d log_std, sum adv and the row count are fp64 per lane, a LIN_DS record per wave.  No
// atomics; the split depends on N and the CU count alone.
//
// The solve (k_lin_solve_wide).  linear_policy.h keeps G and five vectors in LDS: 297 KB at NP = 128, m = 32.  Here G stays
// where the reduction wrote it (the fp64 moment block, 128 KB, read through L2), every thread keeps its at most 5 elements of
// g, x, r, z in registers, and only the vector that is multiplied (p, or TRPO's Delta) lives in LDS (33 KB).  Thread (k, ag)
// owns column k of the action rows ag, ag + AG, ag + 2 AG, ag + 3 AG (AG = 1024 / NP action groups), so one read of G[kk][k]
// serves four rows and G is read AG times per product instead of m times.  The CG, the step, the TRPO trials on the closed-form
// KL and what is written to results[] are k_lin_solve's, statement by statement.
#pragma once
#include <type_traits>

#include "linear_policy.h"

namespace mjx {

constexpr int LINW_MIN_N = 64, LINW_MAX_N = 127;
constexpr int LINW_CHAIN_ROUNDS = 8;         // rounds of 128 rows per workgroup chain at the most: 1024 rows
constexpr int LINW_ACTS = 4;                 // action rows per thread of the solve

__host__ __device__ constexpr int linw_gram_blocks(int NB) { return NB * (NB + 1) / 2; }
// a chain's slab: the distinct Gram blocks (block id order: 00, 01, .., 0 NB-1, 11, ..) | the NB gradient blocks, summed over the waves
__host__ __device__ constexpr int linw_slab_floats(int NB) { return (linw_gram_blocks(NB) + NB) * 16 * 64; }
// id of the distinct block (bi <= bj)
__host__ __device__ constexpr int linw_block_id(int NB, int bi, int bj) { return bi * NB - bi * (bi - 1) / 2 + (bj - bi); }
static_assert(LinLayout::wide(64).NP == 96 && LinLayout::wide(95).NP == 96 && LinLayout::wide(96).NP == 128 && LinLayout::wide(127).NP == 128, "NP");
static_assert(LinLayout::wide(127).bytes() <= 160 * 1024 && LinLayout::wide(127).bytes() - sizeof(float) * LinLayout::wide(127).img() <= 88 * 1024, "the passes fit LDS");
static_assert(4 * 16 * 64 <= LinLayout::wide(127).img() && 3 * 16 * 64 <= LinLayout::wide(64).img(), "a wave's gradient images fit its Z tile");
static_assert(linw_block_id(4, 3, 3) == 9 && linw_block_id(3, 1, 2) == 4, "block ids");

// pass 1 stages ONE [W | b] image: its vectors and Z tiles lie an image earlier than LinLayout's, which serves the closing pass
__host__ __device__ constexpr int linw_moments_off_vec(const LinLayout L) { return L.img(); }
__host__ __device__ constexpr int linw_moments_off_z(const LinLayout L) { return L.off_z() - L.img(); }
__host__ __device__ constexpr size_t linw_moments_bytes(const LinLayout L) { return L.bytes() - sizeof(float) * (size_t)L.img(); }

inline LinRoute linear_route_wide(int n, int m, int n_hidden, bool on, bool on_wide) {
  if (!on) return LinRoute{0, 0, 0, 0};
  if (!on_wide || n_hidden != 0 || n < LINW_MIN_N || n > LINW_MAX_N || m > LIN_MAX_M) return linear_route(n, m, n_hidden, on);
  return LinRoute{2, LinLayout::wide(n).NP, linw_moments_bytes(LinLayout::wide(n)), 128 * LINW_CHAIN_ROUNDS};
}

// One tile ahead in registers, ROW-WISE: with n >= 64 a lane keeps columns lane and lane + 64 of each of the 32 rows (two
// coalesced loads per row; the second is masked beyond n).  The lane's two column constants and Z offsets are then the same for
// every row -- LinTile's element walk, unrolled 64 times, kept ~190 loop-invariant registers alive across the tile loop and spilled.
struct LinTileW { float o[64]; float act[16]; float adv[16]; };

__device__ __forceinline__ void lin_load_tile(LinTileW& t, const LinArgs& a, int64_t row0, int lane) {
  const int j = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const bool valid = row0 + i < a.N;
    const float* o = a.obs + (row0 + i) * a.n;
    t.o[2 * i] = valid ? o[lane] : 0.f;                                  // (lane < 64 <= n)
    t.o[2 * i + 1] = (valid && lane + 64 < a.n) ? o[lane + 64] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t gr = row0 + unit_of(r, hi);
    const bool valid = gr < a.N;
    t.act[r] = (valid && j < a.m) ? a.act[gr * a.m + j] : 0.f;
    t.adv[r] = valid ? a.adv[gr] : 0.f;
  }
}

// (k_lin_eval hands every tile type the four constants of LinTile's element walk; a row-wise lane needs none of them)
__device__ __forceinline__ void lin_write_tile(float* Z, const LinLayout L, const float* vec, const LinTileW& t, const LinArgs& a,
                                               int64_t row0, int lane, int = 0, int = 0, int = 0, int = 0) {
  const bool c1 = lane + 64 < a.n;
  const float s0 = vec[lane], d0 = vec[L.NP + lane], s1 = c1 ? vec[lane + 64] : 0.f, d1 = c1 ? vec[L.NP + lane + 64] : 1.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const bool valid = row0 + i < a.N;
    Z[i * L.S + lane] = valid ? (t.o[2 * i] - s0) / d0 : 0.f;
    if (c1) Z[i * L.S + lane + 64] = valid ? (t.o[2 * i + 1] - s1) / d1 : 0.f;
  }
  if (lane < 32) Z[lane * L.S + a.n] = (row0 + lane < a.N) ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------- pass 1
// a.chain_tiles: ROUNDS per chain; a.chains: the grid (a workgroup per chain); a.ds: 4 LIN_DS records per chain; a.adv_sum unused.
template <int NB>
__global__ __launch_bounds__(64 * LIN_WAVES) void k_lin_moments_wide(const LinArgs a) {
  extern __shared__ float lin_lds[];
  constexpr int NG = linw_gram_blocks(NB), KW = (NG + LIN_WAVES - 1) / LIN_WAVES;
  const LinLayout L = LinLayout::wide(a.n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hi = lane >> 5;
  lin_stage_policy<false, 1>(lin_lds, L, a, tid);
  float* Z0 = lin_lds + linw_moments_off_z(L);
  float* Z = Z0 + wave * L.img();
  for (int i = lane; i < L.img(); i += 64) Z[i] = 0.f;
  __syncthreads();
  const int64_t chain = blockIdx.x;
  const float* w0 = lin_lds; const float* vec = lin_lds + linw_moments_off_vec(L); const float* pa = vec + 2 * L.NP;
  const float osc = pa[j], osh = pa[32 + j], sg = pa[64 + j];
  const int nq = (a.n + 8) >> 3;
  const int64_t rounds = (a.N + 127) >> 7, round0 = chain * a.chain_tiles;
  const int64_t round1 = round0 + a.chain_tiles < rounds ? round0 + a.chain_tiles : rounds;
  // the wave's Gram blocks: ids wave, wave + 4, wave + 8 below NG (the last one may be missing: wave-uniform)
  int ca[KW], cb[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    int b = wave + LIN_WAVES * k, bi = 0;
    if (b >= NG) b = 0;                                // (not computed; any valid columns)
    while (b >= NB - bi) { b -= NB - bi; ++bi; }
    ca[k] = 32 * bi + j; cb[k] = 32 * (bi + b) + j;
  }
  const bool last = wave + LIN_WAVES * (KW - 1) < NG;

  f32x16 G[KW], gA[NB];
#pragma unroll
  for (int k = 0; k < KW; ++k) G[k] = (f32x16)(0.f);
#pragma unroll
  for (int b = 0; b < NB; ++b) gA[b] = (f32x16)(0.f);
  double gls = 0.0, sadv = 0.0;
  int64_t rows = 0;
  LinTileW t;
  lin_load_tile(t, a, (round0 * LIN_WAVES + wave) * 32, lane);
  for (int64_t round = round0; round < round1; ++round) {
    const int64_t row0 = (round * LIN_WAVES + wave) * 32;
    if (round > round0) __syncthreads();               // every wave has read the tiles of the round before
    lin_write_tile(Z, L, vec, t, a, row0, lane);      // (a tile beyond N: all zeros)
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
    const int64_t over = a.N - row0;
    const int left = (int)(over < 0 ? 0 : over < 32 ? over : 32);
    rows += left;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool valid = unit_of(r, hi) < left, ok = valid && j < a.m;
      const float mn = mu[r] * osc + osh;
      const float zn = ok ? (t.act[r] - mn) / sg : 0.f;
      const float w = t.adv[r];                         // (0 beyond N)
      D[r] = ok ? osc * (w * zn / sg) : 0.f;
      if (ok) gls += (double)(w * (zn * zn - 1.0f));
      if (j == 0) sadv += (double)w;
    }
    if (round + 1 < round1) lin_load_tile(t, a, row0 + 32 * LIN_WAVES, lane);      // in flight under the MFMAs below
    // Z^T D over the wave's own rows
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* zc = &Z[(8 * q + 4 * hi + r) * L.S + j];
#pragma unroll
        for (int b = 0; b < NB; ++b) gA[b] = MJX_MFMA(zc[32 * b], D[4 * q + r], gA[b]);
      }
    }
    __syncthreads();                                   // the round's four tiles are staged
    // the wave's Gram blocks over all four tiles
    auto gram = [&](auto kc) {
      constexpr int K = decltype(kc)::value;
#pragma unroll 1
      for (int tl = 0; tl < LIN_WAVES; ++tl) {
        const float* zt = Z0 + tl * L.img() + 4 * hi * L.S;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float* zr = zt + (8 * q + r) * L.S;
#pragma unroll
            for (int k = 0; k < K; ++k) {
              const float za = zr[ca[k]], zb = ca[k] == cb[k] ? za : zr[cb[k]];
              G[k] = MJX_MFMA(za, zb, G[k]);
            }
          }
        }
      }
    };
    if (last) gram(std::integral_constant<int, KW>{});
    else gram(std::integral_constant<int, KW - 1>{});
  }
  // the chain's register images: Gram blocks as they lie
  float* sl = a.slab + chain * linw_slab_floats(NB);
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    if (k < KW - 1 || last) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sl[((wave + LIN_WAVES * k) * 16 + r) * 64 + lane] = G[k][r];
    }
  }
  // the gradient images: the four waves' sums through the free tiles, wave 0 to 3 in order
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Z[(b * 16 + r) * 64 + lane] = gA[b][r];
  __syncthreads();
  for (int i = tid; i < NB * 16 * 64; i += 64 * LIN_WAVES)
    sl[NG * 16 * 64 + i] = ((Z0[i] + Z0[L.img() + i]) + Z0[2 * L.img() + i]) + Z0[3 * L.img() + i];
  double* ds = a.ds + (chain * LIN_WAVES + wave) * LIN_DS;
  ds[lane] = gls;
  if (j == 0) ds[64 + hi] = sadv;
  if (lane == 0) { ds[66] = (double)rows; ds[67] = 0.0; }
}

// k_lin_reduce for the wide slabs: 16 elements x 16 chain groups per workgroup, a group adds its chains in chain order, then the
// groups are added in order; a block below the diagonal is its mirror image transposed.  `chains` workgroup chains, 4 LIN_DS records each.
__global__ __launch_bounds__(256) void k_lin_reduce_wide(const float* __restrict__ slab, const double* __restrict__ ds, int64_t chains,
                                                         int n, int m, double* __restrict__ block) {
  __shared__ double sh[16][17];
  const LinLayout L = LinLayout::wide(n);
  const int el = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int64_t e = (int64_t)blockIdx.x * 16 + el, nG = (int64_t)L.NP * L.NP, nA = nG + (int64_t)m * L.NP, cnt = L.block_count(m);
  double acc = 0.0;
  if (e < nA) {
    int blk, i, jj;
    if (e < nG) {
      int k1 = (int)(e / L.NP), k2 = (int)(e % L.NP);
      if ((k1 >> 5) > (k2 >> 5)) { const int s = k1; k1 = k2; k2 = s; }
      blk = linw_block_id(L.NB, k1 >> 5, k2 >> 5);
      i = k1 & 31; jj = k2 & 31;
    } else {
      const int act = (int)((e - nG) / L.NP), k = (int)((e - nG) % L.NP);
      blk = linw_gram_blocks(L.NB) + (k >> 5);
      i = k & 31; jj = act;
    }
    const int off = (blk * 16 + (i & 3) + 4 * (i >> 3)) * 64 + 32 * ((i >> 2) & 1) + jj;      // register, lane half, column
    const size_t SL = (size_t)linw_slab_floats(L.NB);
    for (int64_t c = grp; c < chains; c += 16) acc += (double)slab[c * SL + off];
  } else if (e < cnt) {
    const int k = (int)(e - nA);
    for (int64_t c = grp; c < chains * LIN_WAVES; c += 16) {
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

// ---------------------------------------------------------------------------- the solve
// LDS in doubles: the multiplied vector in the padded layout [m x NP | m] | c, s (32 each) | the block sums' 32
inline size_t linw_solve_bytes(const LinLayout L, int m) { return sizeof(double) * ((size_t)m * L.NP + m + 96); }

template <int MODE>
__global__ __launch_bounds__(LIN_SOLVE_NT) void k_lin_solve_wide(const LinSolveArgs a) {
  static_assert(MODE == LIN_SOLVE_NPG || MODE == LIN_SOLVE_TRPO, "the wide route serves NPG and TRPO");
  extern __shared__ double lin_sol[];
  const LinLayout L = LinLayout::wide(a.n);
  const int NP = L.NP, n = a.n, m = a.m, MN = m * NP, oB = m * n, oS = oB + m, tid = threadIdx.x;
  const int AG = LIN_SOLVE_NT / NP, k = tid % NP, ag = tid / NP;        // (NP = 96: the 64 threads of ag == AG own no matrix element)
  static_assert(LINW_ACTS * (LIN_SOLVE_NT / 128) >= LIN_MAX_M, "four rows per thread cover every action");
  constexpr int E = LINW_ACTS + 1;                                       // slots 0..3: (ag + AG i, k); slot 4: log_std tid
  double* p = lin_sol; double* cv = p + MN + m; double* sv = cv + 32; double* sh = sv + 32;
  const double* G = a.block + k;
  bool on[E]; int pe[E], act[E];
  double g[E], x[E], r[E], z[E];
#pragma unroll
  for (int i = 0; i < E; ++i) {
    act[i] = i < LINW_ACTS ? ag + AG * i : tid;
    on[i] = i < LINW_ACTS ? (ag < AG && act[i] < m) : tid < m;
    pe[i] = i < LINW_ACTS ? act[i] * NP + k : MN + tid;
    g[i] = on[i] ? a.block[NP * NP + pe[i]] * a.inv_N : 0.0;
    x[i] = 0.0; r[i] = g[i]; z[i] = 0.0;
    if (on[i]) p[pe[i]] = g[i];
  }
  if (tid < m) {
    const double sg = exp((double)a.theta[oS + tid]), u = sg * sg, eps = 1e-8, osc = (double)a.tr[2 * n + m + tid];
    cv[tid] = 2.0 / (2.0 * u + eps) * osc * osc;
    sv[tid] = 4.0 * u * (2.0 * u - eps) / ((2.0 * u + eps) * (2.0 * u + eps));
  }
  __syncthreads();
  // s[i] = (row act[i] of the LDS vector) . (column k of G / N): rows of G behind the ones column are zero and are not read
  auto times_G = [&](double* s) {
#pragma unroll
    for (int i = 0; i < LINW_ACTS; ++i) s[i] = 0.0;
    if (ag < AG) {
#pragma unroll 4
      for (int kk = 0; kk <= n; ++kk) {
        const double gv = G[kk * NP];
#pragma unroll
        for (int i = 0; i < LINW_ACTS; ++i) if (on[i]) s[i] += p[act[i] * NP + kk] * gv;
      }
    }
#pragma unroll
    for (int i = 0; i < LINW_ACTS; ++i) s[i] *= a.inv_N;
  };
  auto dot = [&](const double* u, const double* v) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < E; ++i) s += u[i] * v[i];      // (a slot that is off holds zeros)
    return block_sum(s, sh);
  };
  double rdotr = dot(r, r);
  for (int it = 0; it < a.iters; ++it) {
    double s[LINW_ACTS], pv[E];
    times_G(s);
#pragma unroll
    for (int i = 0; i < E; ++i) {
      pv[i] = on[i] ? p[pe[i]] : 0.0;
      z[i] = !on[i] ? 0.0 : (i < LINW_ACTS ? cv[act[i]] * s[i] : sv[tid] * pv[i]) + a.damping * pv[i];
    }
    const double al = rdotr / dot(pv, z);
#pragma unroll
    for (int i = 0; i < E; ++i) { x[i] += al * pv[i]; r[i] -= al * z[i]; }
    const double nw = dot(r, r);                       // (its barriers: every thread is past times_G before p changes)
#pragma unroll
    for (int i = 0; i < E; ++i) if (on[i]) p[pe[i]] = r[i] + (nw / rdotr) * pv[i];
    rdotr = nw;
    __syncthreads();
    if (rdotr < a.tol) break;                          // (every thread holds the same sum)
  }
  const double gx = dot(g, x);
  const bool npg = a.const_alpha != a.const_alpha;
  const double a64 = npg ? sqrt(fabs(a.step_size / (gx + 1e-20))) : a.const_alpha;
  float alpha = (float)a64;
  if (tid == 0) { a.results[8] = gx; if (npg) a.results[9] = a64; }
  if (tid < 4) a.results[4 + tid] = a.block[L.block_count(m) - 4 + tid];
  // where slot i lives in theta (-1: a padded column)
  int ti[E];
#pragma unroll
  for (int i = 0; i < E; ++i) ti[i] = !on[i] ? -1 : i == LINW_ACTS ? oS + tid : k < n ? act[i] * n + k : k == n ? oB + act[i] : -1;
  if (MODE == LIN_SOLVE_TRPO) {
    // p: Delta (log_std elements: the new log_std itself); cv: out_scale^2; sv: 1 / (2 u_new + 1e-8) of the trial
    __syncthreads();
    if (tid < m) { const double osc = (double)a.tr[2 * n + m + tid]; cv[tid] = osc * osc; }
    double at = a64, tried = a64;
    int trials = 0;
    bool accepted = false;
    while (trials < a.max_trials && !accepted) {
      const float af = (float)at;
      double dl[E], s[LINW_ACTS];
#pragma unroll
      for (int i = 0; i < E; ++i) {
        dl[i] = 0.0;
        if (i < LINW_ACTS) {
          if (ti[i] >= 0) { const float th = a.theta[ti[i]]; dl[i] = (double)step_add(th, af, (float)x[i]) - (double)th; }
          if (on[i]) p[pe[i]] = dl[i];
        } else if (on[i]) {
          const double ln = (double)fmaxf(step_add(a.theta[ti[i]], af, (float)x[i]), a.min_log_std), sg = exp(ln);
          dl[i] = ln; p[pe[i]] = ln;
          sv[tid] = 1.0 / (2.0 * sg * sg + 1e-8);
        }
      }
      __syncthreads();
      times_G(s);
      double sum = 0.0;
#pragma unroll
      for (int i = 0; i < LINW_ACTS; ++i) if (on[i]) sum += cv[act[i]] * sv[act[i]] * (s[i] * dl[i]);
      if (on[LINW_ACTS]) {
        const double lo = (double)a.theta[oS + tid], so = exp(lo), sn = exp(dl[LINW_ACTS]);
        sum += (so * so - sn * sn) * sv[tid] + dl[LINW_ACTS] - lo;
      }
      const double kl = block_sum(sum, sh);             // (every thread holds the same sum; its barriers also free p / sv for the next trial)
      if (tid == 0) { a.results[16 + 2 * (trials % 24)] = nan(""); a.results[17 + 2 * (trials % 24)] = kl * a.N_global; }
      ++trials;
      tried = at;
      if (kl < a.kl_dist) accepted = true;
      else at = 0.9 * at;
    }
    alpha = accepted ? (float)tried : 0.f;
    if (tid == 0) { a.results[9] = tried; a.results[10] = accepted ? 1.0 : 0.0; a.results[11] = (double)trials; a.results[12] = at; }
  }
#pragma unroll
  for (int i = 0; i < E; ++i) {
    if (ti[i] < 0) continue;
    const float xf = (float)x[i];
    a.grad_out[ti[i]] = (float)g[i];
    a.x_out[ti[i]] = xf;
    float v = step_add(a.theta[ti[i]], alpha, xf);
    if (i == LINW_ACTS) v = fmaxf(v, a.min_log_std);
    a.theta_out[ti[i]] = v;
  }
}

// ---------------------------------------------------------------------------- the closing pass: k_lin_eval's body at NB = 3 / 4
// k_lin_eval<NB, LinTileW, true>: the kernel of linear_policy.h itself, on the wide layout and the row-wise tile.

}  // namespace mjx
