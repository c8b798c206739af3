// lw_plan.h -- the host-side decisions of the layer-wise path, as plain C++: what a product is (GemmArgs), which switches the
// environment sets (LwSwitches), which kernel instances a product goes to (lw_plan_gemm) and over how many sample splits a weight
// gradient runs (wgrad_splits).  No kernels and no HIP calls: tests/c/lw_plan.cpp compiles it with g++ and checks the routes
// against a table.  lw_launch.h is the only code that turns a plan into launches; the kernels are in lw_gemm.h / lw_gemm_p.h.
#pragma once
#include <stdint.h>

#include <cstdlib>

#include "launch_state.h"

namespace mjx {

enum { EPI_STORE = 0, EPI_BIAS_TANH, EPI_BIAS_AFFINE, EPI_TANGENT, EPI_BACK, EPI_BIAS, EPI_BIAS_RELU, EPI_BACK_RELU, EPI_RBACK, EPI_FVP_HEAD };

struct GemmArgs {
  int M, N, npairs;
  int K[2];
  const float* A[2]; int64_t a_rs[2], a_ks[2];   // A(i,k) = A[i*a_rs + k*a_ks]
  const float* B[2]; int64_t b_cs[2], b_ks[2];   // B(k,j) = B[j*b_cs + k*b_ks]
  float* C; int64_t ldc;                          // C(i,j) = C[i*ldc + j*c_cs] (+ z*c_zs for split-K); c_cs == 0 means 1
  int64_t c_zs, c_cs;
  float* colsum;                                  // optional [gridDim.y][cs_ld]: per-block column sums of the stored values (bias gradients)
  int64_t cs_ld;                                  // row stride of colsum (0: N)
  const float* bias;                              // per column
  const float* aux; int64_t ld_aux;               // activation for the (1 - y^2) factor
  const float* aux2; const float* aux3;           // EPI_RBACK: tangent activation t and the pre-activation cotangent
  const float* osc; const float* osh;             // per-column affine (EPI_BIAS_AFFINE)
  const float* ls; float inv_N;                   // EPI_FVP_HEAD: log_std per column, 1 / N_global
  int fast;                                       // set by the launcher: the interior fast path of the 256-column tiles may be used
  int rows_padded;                                // A / aux / C are workspace blocks with rows allocated up to a multiple of 128
  int epi;
#ifdef MJX_PHASE_CLOCK
  long long* clk;                                 // timing build: 8 int64 per workgroup (tools/lw_clock.py)
#endif
};

// Tile geometry of the two GEMM kernels (k_gemm: lw_gemm.h, k_gemm_p: lw_gemm_p.h) and the dynamic LDS their operand tiles take
constexpr int GBN = 128, GBK = 32, GLD = GBK + 4;
constexpr int LW_BM = 128;                                                             // rows per workgroup tile, every instance
constexpr size_t gemm_lds_bytes(int BM, int BN) {
  return 2 * sizeof(float) * (size_t)(((BM * GLD > GBK * (BM + 4)) ? BM * GLD : GBK * (BM + 4)) + ((BN * GLD > GBK * (BN + 4)) ? BN * GLD : GBK * (BN + 4)));
}
constexpr int GP_BM = 128, GP_BN = 256, GP_BK = 32, GP_LD = GP_BK + 4, GP_NTH = 512;
constexpr int GP_ASZ = GP_BM * GP_LD;                                                  // [row][k] image of the A tile
template <int LB> constexpr int gp_bsz() { return LB ? GP_BK * (GP_BN + 4) : GP_BN * GP_LD; }
template <int LB> constexpr size_t gp_lds_bytes() { return sizeof(float) * (size_t)(2 * GP_ASZ + 2 * gp_bsz<LB>() + 2 * GP_BN); }

// ---- switches.  Every MJX_LW_* switch of the path, its default, and when it is read:
//   switch              default  selects                                                                        read
//   MJX_LW_TILES        1        0: 128 x 128 tiles in 512-thread workgroups only (and the scalar split          per operation
//                                reduction), 1: 128 x 256 tiles + the persistent kernel, 2: 128 x 128 tiles in
//                                256-thread workgroups, two per CU
//   MJX_LW_FAST         1        the interior fast k-loop of the 256-column tiles                                per operation
//   MJX_LW_PERSIST      1        steady-state sample-major products on the persistent kernel (lw_gemm_p.h)       per operation
//   MJX_LW_THIN         1        weight gradients of 33..128 columns in 256-thread workgroups, two per CU        per operation
//   MJX_LW_THIN64       1        ... of up to 64 columns on a 128 x 64 tile                                      per operation
//   MJX_LW_SPLITS       1        round balancing of the weight gradients' sample splits (pick_splits)            per operation
//   MJX_LW_CHAIN        1024     samples one workgroup accumulates in one fp32 MFMA chain (>= 256)               per operation
//   MJX_LW_WG_CAP       8192     workgroup budget that caps the sample splits (>= 64)                            per operation
//   MJX_LW_OVERLAP      0        weight gradients on a side stream beside the delta products (N >= 65536)        per operation
//   MJX_LW_HEAD         1        the output layer of the Fisher-vector product as one pass (lw_head.h)           per operation
//   MJX_LW_HEAD8        1        ... its eight-wave build at 256 / 512 units                                     per operation
//   MJX_LW_HEAD_KTRIM   1        ... with the contraction over the actions trimmed to ceil(m / 2) steps          per operation
//   MJX_LW_WT           1        W_l^T of the hidden layers for the delta products (LayerwiseWS::Wt)             once per process, at the first forward pass that fills the activation cache
//   MJX_LW_OLD_OUTPUTS  1        K3 / the trial evaluations reuse K1's outputs as the old policy's               once per process, at the first LayerwiseWS::eval
// "per operation": LwSwitches::read() at the start of forward / backward / fvp / hvp_general, and by lw_launch_gemm /
// lw_reduce_split when a caller outside the path passes none.  bench.lw_switch_ab and tests/test_gpu_dispatch_matrix.py flip
// switches between calls in one process, so nothing but the last two may be read less often.
struct LwSwitches {
  int tiles = 1;
  bool fast = true, persist = true, thin = true, thin64 = true, splits = true, overlap = false, head = true, head8 = true, head_ktrim = true;
  int chain = 1024, wg_cap = 8192;
  static LwSwitches read() {
    LwSwitches s;
    if (const char* e = getenv("MJX_LW_TILES")) if (e[0] >= '0' && e[0] <= '2') s.tiles = e[0] - '0';
    s.fast = env_flag("MJX_LW_FAST", true); s.persist = env_flag("MJX_LW_PERSIST", true);
    s.thin = env_flag("MJX_LW_THIN", true); s.thin64 = env_flag("MJX_LW_THIN64", true);
    s.splits = env_flag("MJX_LW_SPLITS", true); s.overlap = env_flag("MJX_LW_OVERLAP", false);
    s.head = env_flag("MJX_LW_HEAD", true); s.head8 = env_flag("MJX_LW_HEAD8", true); s.head_ktrim = env_flag("MJX_LW_HEAD_KTRIM", true);
    if (const char* e = getenv("MJX_LW_CHAIN")) { const int x = atoi(e); if (x >= 256) s.chain = x; }
    if (const char* e = getenv("MJX_LW_WG_CAP")) { const int x = atoi(e); if (x >= 64) s.wg_cap = x; }
    return s;
  }
  static bool wt() { static const bool on = env_flag("MJX_LW_WT", true); return on; }
  static bool old_outputs() { static const bool on = env_flag("MJX_LW_OLD_OUTPUTS", true); return on; }
};

// ---- GemmArgs builders: the three product kinds of the path.  Everything a builder does not set is zero.
// Sample-major ("NT"): C[M x N] = act[M x K] W^T, W = N rows of K weights (row stride ldw), activations of row stride lda
inline void gemm_nt_pair(GemmArgs& g, int p, int K, const float* act, int64_t lda, const float* W, int64_t ldw) {
  g.npairs = p + 1; g.K[p] = K;
  g.A[p] = act; g.a_rs[p] = lda; g.a_ks[p] = 1;
  g.B[p] = W; g.b_cs[p] = ldw; g.b_ks[p] = 1;
}
inline GemmArgs gemm_nt(int M, int N, int K, const float* act, int64_t lda, const float* W, int64_t ldw, float* C, int epi) {
  GemmArgs g{};
  g.M = M; g.N = N; g.C = C; g.ldc = N; g.epi = epi;
  gemm_nt_pair(g, 0, K, act, lda, W, ldw);
  return g;
}
// Delta product: C[M x hi] = delta[M x ho] W, W = the layer's ho x hi weight block as it lies, or (transposed) its hi x ho transpose
inline void gemm_delta_pair(GemmArgs& g, int p, int ho, int hi, const float* delta, const float* W, bool transposed = false) {
  g.npairs = p + 1; g.K[p] = ho;
  g.A[p] = delta; g.a_rs[p] = ho; g.a_ks[p] = 1;
  g.B[p] = W; g.b_cs[p] = transposed ? ho : 1; g.b_ks[p] = transposed ? 1 : hi;
}
inline GemmArgs gemm_delta(int M, int ho, int hi, const float* delta, const float* W, bool transposed, float* C, const float* aux, int epi) {
  GemmArgs g{};
  g.M = M; g.N = hi; g.C = C; g.ldc = hi; g.aux = aux; g.ld_aux = hi; g.epi = epi;
  gemm_delta_pair(g, 0, ho, hi, delta, W, transposed);
  return g;
}
// Weight gradient over `rows` samples (the split dimension): C[ho x cols] = delta^T in, delta = rows x ho, in = rows x cols of
// row stride ld_in; slabs of ho * cols floats per split.  transposed (narrow outputs, ho <= 32): the product is formed as
// in^T delta (cols x ho, so that the padding goes to 32 columns instead of 128 rows) and stored transposed, into the same C
inline void gemm_wgrad_pair(GemmArgs& g, int p, int rows, int ho, const float* delta, const float* in, int64_t ld_in, bool transposed = false) {
  g.npairs = p + 1; g.K[p] = rows;
  const float *a = transposed ? in : delta, *b = transposed ? delta : in;
  const int64_t lda = transposed ? ld_in : ho, ldb = transposed ? ho : ld_in;
  g.A[p] = a; g.a_rs[p] = 1; g.a_ks[p] = lda;
  g.B[p] = b; g.b_cs[p] = 1; g.b_ks[p] = ldb;
}
inline GemmArgs gemm_wgrad(int rows, int ho, int cols, const float* delta, const float* in, int64_t ld_in, float* C, bool transposed = false) {
  GemmArgs g{};
  g.M = transposed ? cols : ho; g.N = transposed ? ho : cols;
  g.C = C; g.c_zs = (int64_t)ho * cols; g.epi = EPI_STORE;
  if (transposed) { g.ldc = 1; g.c_cs = cols; } else g.ldc = cols;       // C^T(i = input unit, j = output unit) -> gW[j][i]
  gemm_wgrad_pair(g, 0, rows, ho, delta, in, ld_in, transposed);
  return g;
}

// grid of an element-wise kernel over cnt elements, 256 threads per workgroup
inline int ew_grid(int64_t cnt) { int64_t g = (cnt + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// ---- the plan of one product
struct LwTileStep { int BN, NTH, j0, ncols; unsigned gx, gy, gz; size_t lds; };      // k_gemm<128, BN, NTH> over columns [j0, j0 + ncols)
struct LwPlan {
  int ntile = 0;                                   // tile steps (1 or 2); 0: one persistent step
  LwTileStep tile[2];
  int LB = 0, epi = 0, row_tiles = 0, col_blocks = 0, grid = 0;     // k_gemm_p<LB, epi>
  size_t lds = 0;
};

// the launch restricted to columns [j0, j0 + ncols)
inline GemmArgs lw_col_slice(const GemmArgs& g, int j0, int ncols) {
  GemmArgs h = g;
  if (!h.cs_ld) h.cs_ld = g.N;
  h.N = ncols;
  for (int p = 0; p < g.npairs; ++p) h.B[p] = g.B[p] + (int64_t)j0 * g.b_cs[p];
  h.C = g.C + (int64_t)j0 * (g.c_cs ? g.c_cs : 1);
  if (g.colsum) h.colsum = g.colsum + j0;
  if (g.bias) h.bias = g.bias + j0;
  if (g.aux) h.aux = g.aux + j0;
  if (g.aux2) h.aux2 = g.aux2 + j0;
  if (g.aux3) h.aux3 = g.aux3 + j0;
  if (g.osc) h.osc = g.osc + j0;
  if (g.osh) h.osh = g.osh + j0;
  if (g.ls) h.ls = g.ls + j0;
  return h;
}
// Weight gradients with 33..128 columns (the first layer of a narrow observation: 512 x 40 at configs[4]) are bound by the
// bytes they keep in flight, not by the matrix cores (3.3 us per k-tile against 1 us of MFMAs): 128 x 128 tiles in
// 256-thread workgroups, two per CU (MJX_LW_THIN=0: one 512-thread workgroup per CU as for the wide ones)
inline bool lw_thin_wgrad(int ncols, const LwSwitches& sw) { return sw.thin && ncols > 32 && ncols <= 128 && sw.tiles == 1; }
// column blocks a product covers N columns with
inline int lw_col_blocks(int N, const LwSwitches& sw) {
  if (N <= 32) return 1;
  if (sw.tiles != 1) return (N + 127) / 128;
  return N / 256 + ((N % 256) ? 1 : 0);
}
// Sample-major products in their steady-state shape go to the persistent kernel (lw_gemm_p.h): the B layout it can run
// with (0 / 1), -1: not eligible.  MJX_LW_PERSIST=0, or a device without ticket counters, keeps everything on the general kernel.
inline int lw_persistent_lb(const GemmArgs& g, int splits, const LwSwitches& sw, bool has_ring) {
  if (!sw.persist || !has_ring || splits != 1 || sw.tiles != 1 || g.M < 2 * GP_BM || g.N < GP_BN || (g.N % GP_BN) != 0) return -1;
  if ((g.M % GP_BM) != 0 && !g.rows_padded) return -1;
  if ((g.epi != EPI_TANGENT && g.epi != EPI_BACK && g.epi != EPI_BIAS_TANH) || (g.c_cs != 0 && g.c_cs != 1) || g.c_zs != 0) return -1;
  if (g.epi != EPI_BIAS_TANH && !g.aux) return -1;
  if (g.epi != EPI_BACK && !g.bias) return -1;
  if (g.ldc >= (1 << 24) || g.ld_aux >= (1 << 24) || (((uintptr_t)g.C | (uintptr_t)g.aux) & 3)) return -1;
  int lb = -1;
  for (int p = 0; p < g.npairs; ++p) {
    if (g.K[p] < 2 * GP_BK || (g.K[p] % GP_BK) != 0) return -1;       // whole k-tiles, at least two
    if (g.a_ks[p] != 1 || (g.a_rs[p] & 3) != 0 || (((uintptr_t)g.A[p]) & 15) != 0) return -1;
    int l;
    if (g.b_ks[p] == 1 && (g.b_cs[p] & 3) == 0 && (((uintptr_t)g.B[p]) & 15) == 0) l = 0;
    else if (g.b_cs[p] == 1 && (g.b_ks[p] & 3) == 0 && (((uintptr_t)g.B[p]) & 15) == 0) l = 1;
    else return -1;
    if (lb >= 0 && l != lb) return -1;
    lb = l;
  }
  return lb;
}
// Which kernel instances serve product g over `splits` sample splits on a device of ncu CUs.  has_ring: the device has the
// persistent kernel's ticket counters (lw_launch.h allocates them at the first product of more than 32 columns, MJX_LW_PERSIST on).
inline LwPlan lw_plan_gemm(const GemmArgs& g, int splits, const LwSwitches& sw, int ncu, bool has_ring) {
  LwPlan pl;
  auto tile = [&](int BN, int NTH, int j0, int ncols) {
    pl.tile[pl.ntile++] = LwTileStep{BN, NTH, j0, ncols, (unsigned)((ncols + BN - 1) / BN), (unsigned)((g.M + LW_BM - 1) / LW_BM), (unsigned)splits, gemm_lds_bytes(LW_BM, BN)};
  };
  if (g.N <= 32) { tile(32, 256, 0, g.N); return pl; }
  const int lb = lw_persistent_lb(g, splits, sw, has_ring);
  if (lb >= 0) {
    pl.LB = lb; pl.epi = g.epi;
    pl.row_tiles = (g.M + GP_BM - 1) / GP_BM; pl.col_blocks = g.N / GP_BN;
    const int ntiles = pl.row_tiles * pl.col_blocks;
    pl.grid = ntiles < ncu ? ntiles : ncu;
    pl.lds = lb ? gp_lds_bytes<1>() : gp_lds_bytes<0>();
    return pl;
  }
  if (sw.tiles == 2) { tile(128, 256, 0, g.N); return pl; }
  if (sw.tiles != 1) { tile(128, 512, 0, g.N); return pl; }
  if (splits > 1 && lw_thin_wgrad(g.N, sw)) {
    // (r04) up to 64 columns -- the 512 x 39 first-layer gradient of configs[4], stored 64 wide -- a 128 x 64 tile: the 128-column
    // tile spent half its matrix work and half its B-operand LDS traffic on padding (MJX_LW_THIN64=0: the r03 shape)
    tile((sw.thin64 && g.N <= 64) ? 64 : 128, 256, 0, g.N);
    return pl;
  }
  // 256-column blocks; a remainder of up to 128 columns gets its own 128-column launch (a half-empty 256-column
  // block would spend matrix-core time on padding), a larger one rides in one more 256-column block
  int n256 = (g.N / 256) * 256, rem = g.N - n256;
  if (rem > 128) { n256 = g.N; rem = 0; }
  if (n256) tile(256, 512, 0, n256);
  if (rem) tile(128, 512, n256, rem);
  return pl;
}

// ---- sample splits of a weight-gradient launch
// Whole rounds of workgroups over the CUs.  One workgroup per CU runs at a time (LDS), so tiles x splits = 490 workgroups on
// 256 CUs (configs[3]: 2 row tiles x 245 splits) is two rounds, the second 91 % full, each paying the per-workgroup prologue /
// epilogue; 2 x 128 is ONE full round of twice-as-long workgroups.
// cost(s) = rounds(s) x (samples per workgroup + ~9 us of fixed cost in sample units); the search keeps s within [cap/4, cap].
inline int lw_pick_splits(int64_t N, int row_tiles, int ncols, int cap, const LwSwitches& sw, int ncu) {
  if (cap < 4 || !sw.splits) return cap;
  int cb = 1;                                        // column blocks of the main launch (lw_plan_gemm)
  if (ncols > 32) {
    if (sw.tiles != 1) cb = (ncols + 127) / 128;
    else { cb = ncols / 256 + ((ncols % 256) > 128 ? 1 : 0); if (cb < 1) cb = 1; }
  }
  const int64_t tl = (int64_t)row_tiles * cb;
  const int slots = ncu * (lw_thin_wgrad(ncols, sw) ? 2 : 1);     // (thin products run two 256-thread workgroups per CU)
  int best = cap;
  double bestc = 1e300;
  for (int s = cap; s >= cap / 4 && s >= 1; --s) {
    const int64_t rounds = (tl * s + slots - 1) / slots;
    const double c = (double)rounds * ((double)N / s + 74.0);
    if (c < bestc * 0.999) { bestc = c; best = s; }
  }
  return best;
}
// Splits of the ho x hi gradient over N samples (narrow: formed transposed, hi x ho).  sw.chain: samples one workgroup accumulates
// in ONE fp32 MFMA chain before its partial goes to the fp64 split reduction; sw.wg_cap: the workgroup budget that caps the number
// of splits.  r05: at 1M rows x 512^2 the r04 values (2 048 samples, 1 024 workgroups -> chains of 7 800 samples) left the DAPG
// step 1.5e-5 from the reference (which itself sits 3.2e-6 from fp64 truth): round-off of a sequential fp32 chain grows with its
// length.  Chains of 1 024 samples (up to 8 192 workgroups, 1 GB of partial slabs at that size): 7.2e-6, and the Fisher-vector
// product is 1 % FASTER (19.27 -> 19.01 ms, tools/probe_chain_error.py: more, shorter workgroups fill the last round better).
// (256-row tiles were tried for the weight gradients: 256 x 256 needs 128 accumulator + 80 operand registers per lane and
//  spills 874 VGPRs at two waves per SIMD; 256 x 128 buys nothing over 128 x 256)
inline int wgrad_splits(int64_t N, int ho, int hi, bool narrow, const LwSwitches& sw, int ncu) {
  const int row_tiles = ((narrow ? hi : ho) + LW_BM - 1) / LW_BM;
  const int tiles = narrow ? row_tiles : row_tiles * lw_col_blocks(hi, sw);
  int splits = (int)((N + sw.chain - 1) / sw.chain);
  const int maxs = (sw.wg_cap + tiles - 1) / tiles;
  if (splits > maxs) splits = maxs;
  if (splits < 1) splits = 1;
  return lw_pick_splits(N, row_tiles, narrow ? ho : hi, splits, sw, ncu);
}

}  // namespace mjx
