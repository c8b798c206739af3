// lw_plan.cpp -- the routing of the layer-wise path (mjrl_amd/csrc/lw_plan.h: lw_plan_gemm, wgrad_splits, the GemmArgs builders,
// LwSwitches) against a table, as a plain C++ program: no HIP library, no GPU.  tests/test_lw_plan_cpu.py builds and runs it.
//
// The table below was written by hand from the dispatcher this header replaced (launch_gemm / persistent_lb / col_slice /
// pick_splits of the former LayerwiseWS) and cross-checked against the kernel trace of tests/_gemm_chain_worker.py's default arm
// (profiles/r19_lw_owner/).  256 CUs and a ticket ring unless a row says otherwise.  Switch arms are set through the
// environment and read with LwSwitches::read(), as the library does.
#include "../../mjrl_amd/csrc/lw_plan.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace mjx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d  ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// operand blocks: only the addresses are used (16-byte aligned, far enough apart for any column slice)
alignas(16) static float ACT[1 << 10], W[1 << 18], OUT[1 << 18], BIAS[1 << 10], AUX[1 << 18], CSUM[1 << 10];

static LwSwitches arm(const char* name = nullptr, const char* value = nullptr) {
  for (const char* s : {"MJX_LW_TILES", "MJX_LW_FAST", "MJX_LW_PERSIST", "MJX_LW_THIN", "MJX_LW_THIN64", "MJX_LW_SPLITS", "MJX_LW_OVERLAP", "MJX_LW_HEAD",
                        "MJX_LW_HEAD8", "MJX_LW_HEAD_KTRIM", "MJX_LW_CHAIN", "MJX_LW_WG_CAP"}) unsetenv(s);
  if (name) setenv(name, value, 1);
  return LwSwitches::read();
}

struct Tile { int BN, NTH, j0, ncols; unsigned gx, gy, gz; size_t lds; };
static void expect_tiles(const char* what, const LwPlan& p, std::initializer_list<Tile> want) {
  CHECK(p.ntile == (int)want.size(), "%s: %d tile steps, want %d", what, p.ntile, (int)want.size());
  int i = 0;
  for (const Tile& w : want) {
    if (i >= p.ntile) break;
    const LwTileStep& t = p.tile[i++];
    CHECK(t.BN == w.BN && t.NTH == w.NTH && t.j0 == w.j0 && t.ncols == w.ncols && t.gx == w.gx && t.gy == w.gy && t.gz == w.gz && t.lds == w.lds,
          "%s step %d: k_gemm<128, %d, %d> cols [%d, +%d) grid (%u, %u, %u) lds %zu; want <128, %d, %d> [%d, +%d) (%u, %u, %u) %zu", what, i - 1, t.BN, t.NTH,
          t.j0, t.ncols, t.gx, t.gy, t.gz, t.lds, w.BN, w.NTH, w.j0, w.ncols, w.gx, w.gy, w.gz, w.lds);
  }
}
static void expect_persistent(const char* what, const LwPlan& p, int LB, int epi, int row_tiles, int col_blocks, int grid, size_t lds) {
  CHECK(p.ntile == 0 && p.LB == LB && p.epi == epi && p.row_tiles == row_tiles && p.col_blocks == col_blocks && p.grid == grid && p.lds == lds,
        "%s: ntile %d, k_gemm_p<%d, %d> %d x %d tiles grid %d lds %zu; want persistent <%d, %d> %d x %d grid %d lds %zu", what, p.ntile, p.LB, p.epi,
        p.row_tiles, p.col_blocks, p.grid, p.lds, LB, epi, row_tiles, col_blocks, grid, lds);
}

// dynamic LDS of the instances (two buffers per operand tile; the persistent kernel adds two rows of column sums)
constexpr size_t LDS_256 = 110592, LDS_128 = 73728, LDS_64 = 55296, LDS_32 = 46080, LDS_P0 = 112640, LDS_P1 = 105472;
constexpr int NCU = 256;

// hidden forward: M rows, N units, K = 256 inputs, bias + tanh, activations in padded workspace blocks
static GemmArgs hidden_fwd(int M, int N) {
  GemmArgs g = gemm_nt(M, N, 256, ACT, 256, W, 256, OUT, EPI_BIAS_TANH);
  g.bias = BIAS; g.rows_padded = 1;
  return g;
}
// delta product of a 256 x 256 layer over 3376 rows, EPI_BACK with the activation and per-block column sums
static GemmArgs delta256(const float* Wl, bool transposed) {
  GemmArgs g = gemm_delta(3376, 256, 256, ACT, Wl, transposed, OUT, AUX, EPI_BACK);
  g.rows_padded = 1; g.colsum = CSUM;
  return g;
}

int main() {
  const LwSwitches dflt = arm();
  CHECK(dflt.tiles == 1 && dflt.fast && dflt.persist && dflt.thin && dflt.thin64 && dflt.splits && !dflt.overlap && dflt.head && dflt.head8 && dflt.head_ktrim &&
        dflt.chain == 1024 && dflt.wg_cap == 8192, "defaults");
  CHECK(arm("MJX_LW_CHAIN", "255").chain == 1024 && arm("MJX_LW_WG_CAP", "63").wg_cap == 8192 && arm("MJX_LW_TILES", "3").tiles == 1, "out-of-range values keep the defaults");
  CHECK(arm("MJX_LW_OVERLAP", "1").overlap && !arm("MJX_LW_HEAD", "0").head && arm("MJX_LW_HEAD", "x").head, "on / off switches");

  // ---- the builders
  {
    GemmArgs g = hidden_fwd(3376, 256);
    CHECK(g.M == 3376 && g.N == 256 && g.npairs == 1 && g.K[0] == 256 && g.A[0] == ACT && g.a_rs[0] == 256 && g.a_ks[0] == 1 && g.B[0] == W && g.b_cs[0] == 256 &&
          g.b_ks[0] == 1 && g.C == OUT && g.ldc == 256 && g.c_zs == 0 && g.c_cs == 0 && g.epi == EPI_BIAS_TANH, "gemm_nt");
    gemm_nt_pair(g, 1, 128, AUX, 128, W + 4, 128);
    CHECK(g.npairs == 2 && g.K[1] == 128 && g.A[1] == AUX && g.a_rs[1] == 128 && g.a_ks[1] == 1 && g.B[1] == W + 4 && g.b_cs[1] == 128 && g.b_ks[1] == 1, "gemm_nt_pair");
    GemmArgs d = gemm_delta(3376, 192, 320, ACT, W, false, OUT, AUX, EPI_BACK);
    CHECK(d.M == 3376 && d.N == 320 && d.K[0] == 192 && d.a_rs[0] == 192 && d.a_ks[0] == 1 && d.b_cs[0] == 1 && d.b_ks[0] == 320 && d.ldc == 320 && d.aux == AUX &&
          d.ld_aux == 320 && d.epi == EPI_BACK, "gemm_delta, the weights as they lie");
    d = gemm_delta(3376, 192, 320, ACT, W, true, OUT, AUX, EPI_BACK);
    CHECK(d.b_cs[0] == 192 && d.b_ks[0] == 1, "gemm_delta, transposed weights");
    GemmArgs w = gemm_wgrad(3376, 256, 100, AUX, ACT, 104, OUT);
    CHECK(w.M == 256 && w.N == 100 && w.K[0] == 3376 && w.A[0] == AUX && w.a_rs[0] == 1 && w.a_ks[0] == 256 && w.B[0] == ACT && w.b_cs[0] == 1 && w.b_ks[0] == 104 &&
          w.ldc == 100 && w.c_cs == 0 && w.c_zs == 25600 && w.epi == EPI_STORE, "gemm_wgrad");
    w = gemm_wgrad(3376, 17, 256, AUX, ACT, 256, OUT, true);
    CHECK(w.M == 256 && w.N == 17 && w.A[0] == ACT && w.a_rs[0] == 1 && w.a_ks[0] == 256 && w.B[0] == AUX && w.b_cs[0] == 1 && w.b_ks[0] == 17 && w.ldc == 1 &&
          w.c_cs == 256 && w.c_zs == 17 * 256, "gemm_wgrad, transposed (narrow) form");
  }

  // ---- sample-major products
  expect_persistent("hidden forward M 3376", lw_plan_gemm(hidden_fwd(3376, 256), 1, dflt, NCU, true), 0, EPI_BIAS_TANH, 27, 1, 27, LDS_P0);
  expect_persistent("hidden forward M 3376, 8 CUs", lw_plan_gemm(hidden_fwd(3376, 256), 1, dflt, 8, true), 0, EPI_BIAS_TANH, 27, 1, 8, LDS_P0);
  expect_persistent("hidden forward M 256, N 1024", lw_plan_gemm(hidden_fwd(256, 1024), 1, dflt, NCU, true), 0, EPI_BIAS_TANH, 2, 4, 8, LDS_P0);
  expect_tiles("hidden forward M 255", lw_plan_gemm(hidden_fwd(255, 256), 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 2, 1, LDS_256}});
  expect_tiles("hidden forward, PERSIST=0", lw_plan_gemm(hidden_fwd(3376, 256), 1, arm("MJX_LW_PERSIST", "0"), NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
  expect_tiles("hidden forward, no ring", lw_plan_gemm(hidden_fwd(3376, 256), 1, dflt, NCU, false), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
  expect_tiles("hidden forward, TILES=0", lw_plan_gemm(hidden_fwd(3376, 256), 1, arm("MJX_LW_TILES", "0"), NCU, true), {{128, 512, 0, 256, 2, 27, 1, LDS_128}});
  expect_tiles("hidden forward, TILES=2", lw_plan_gemm(hidden_fwd(3376, 256), 1, arm("MJX_LW_TILES", "2"), NCU, true), {{128, 256, 0, 256, 2, 27, 1, LDS_128}});
  {
    GemmArgs g = hidden_fwd(3376, 256);
    g.rows_padded = 0;                                   // 3376 is not a multiple of 128: only workspace blocks may run persistent
    expect_tiles("hidden forward, rows not padded", lw_plan_gemm(g, 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
    g = hidden_fwd(3328, 256); g.rows_padded = 0;
    expect_persistent("hidden forward M 3328, rows not padded", lw_plan_gemm(g, 1, dflt, NCU, true), 0, EPI_BIAS_TANH, 26, 1, 26, LDS_P0);
    g = hidden_fwd(3376, 256); g.K[0] = 40;              // K not a whole number of k-tiles
    expect_tiles("hidden forward, K 40", lw_plan_gemm(g, 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
    g = hidden_fwd(3376, 256); g.epi = EPI_BIAS_AFFINE;  // an epilogue the persistent kernel does not have
    expect_tiles("output affine, 256 columns", lw_plan_gemm(g, 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
  }
  {
    const GemmArgs g = hidden_fwd(3376, 384);
    const LwPlan p = lw_plan_gemm(g, 1, dflt, NCU, true);
    expect_tiles("N 384", p, {{256, 512, 0, 256, 1, 27, 1, LDS_256}, {128, 512, 256, 128, 1, 27, 1, LDS_128}});
    GemmArgs c = g; c.colsum = CSUM; c.aux = AUX;
    const GemmArgs h = lw_col_slice(c, 256, 128);
    CHECK(h.N == 128 && h.M == 3376 && h.B[0] == W + 256 * 256 && h.C == OUT + 256 && h.bias == BIAS + 256 && h.colsum == CSUM + 256 && h.aux == AUX + 256 &&
          h.cs_ld == 384 && h.ldc == 384 && h.A[0] == ACT && h.osc == nullptr && h.ls == nullptr, "column slice [256, 384)");
    GemmArgs t = gemm_wgrad(3376, 17, 384, AUX, ACT, 384, OUT, true);     // transposed store: a column of the product is a row of C
    t.N = 384; t.c_cs = 100;
    CHECK(lw_col_slice(t, 256, 128).C == OUT + 256 * 100 && lw_col_slice(t, 256, 128).B[0] == AUX + 256, "column slice with a column stride");
  }
  expect_tiles("N 320", lw_plan_gemm(hidden_fwd(3376, 320), 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}, {128, 512, 256, 64, 1, 27, 1, LDS_128}});
  expect_tiles("N 192", lw_plan_gemm(hidden_fwd(3376, 192), 1, dflt, NCU, true), {{256, 512, 0, 192, 1, 27, 1, LDS_256}});
  expect_tiles("N 640", lw_plan_gemm(hidden_fwd(3376, 640), 1, dflt, NCU, true), {{256, 512, 0, 512, 2, 27, 1, LDS_256}, {128, 512, 512, 128, 1, 27, 1, LDS_128}});
  expect_tiles("N 100", lw_plan_gemm(hidden_fwd(3376, 100), 1, dflt, NCU, true), {{128, 512, 0, 100, 1, 27, 1, LDS_128}});
  expect_tiles("N 17", lw_plan_gemm(hidden_fwd(3376, 17), 1, dflt, NCU, true), {{32, 256, 0, 17, 1, 27, 1, LDS_32}});
  expect_tiles("N 32, TILES=0", lw_plan_gemm(hidden_fwd(3376, 32), 1, arm("MJX_LW_TILES", "0"), NCU, true), {{32, 256, 0, 32, 1, 27, 1, LDS_32}});
  {
    GemmArgs g = hidden_fwd(3376, 256);                  // tangent: two operand pairs, the activation for the (1 - y^2) factor
    g.epi = EPI_TANGENT; g.aux = AUX; g.ld_aux = 256;
    gemm_nt_pair(g, 1, 256, AUX, 256, W + 65536, 256);
    expect_persistent("tangent, two pairs", lw_plan_gemm(g, 1, dflt, NCU, true), 0, EPI_TANGENT, 27, 1, 27, LDS_P0);
    g.aux = nullptr;
    expect_tiles("tangent without its activation", lw_plan_gemm(g, 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
  }

  // ---- delta products
  expect_persistent("delta, W^T", lw_plan_gemm(delta256(W, true), 1, dflt, NCU, true), 0, EPI_BACK, 27, 1, 27, LDS_P0);
  expect_persistent("delta, W as it lies (MJX_LW_WT=0)", lw_plan_gemm(delta256(W, false), 1, dflt, NCU, true), 1, EPI_BACK, 27, 1, 27, LDS_P1);
  expect_tiles("delta, misaligned W", lw_plan_gemm(delta256(W + 1, false), 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
  {
    GemmArgs g = gemm_delta(3376, 256, 250, ACT, W, false, OUT, AUX, EPI_BACK);      // hidden width below: not a multiple of 4 (and of 256)
    expect_tiles("delta to 250 units", lw_plan_gemm(g, 1, dflt, NCU, true), {{256, 512, 0, 250, 1, 27, 1, LDS_256}});
    g = delta256(W, true); gemm_delta_pair(g, 1, 256, 256, AUX, W + 65536, false);  // pairs with different B layouts
    expect_tiles("delta, mixed B layouts", lw_plan_gemm(g, 1, dflt, NCU, true), {{256, 512, 0, 256, 1, 27, 1, LDS_256}});
  }

  // ---- weight gradients (256 output units: two row tiles)
  const GemmArgs w100 = gemm_wgrad(3376, 256, 100, AUX, ACT, 100, OUT), w64 = gemm_wgrad(3376, 256, 64, AUX, ACT, 64, OUT);
  expect_tiles("wgrad 100 columns, 4 splits", lw_plan_gemm(w100, 4, dflt, NCU, true), {{128, 256, 0, 100, 1, 2, 4, LDS_128}});
  expect_tiles("wgrad 64 columns, 4 splits", lw_plan_gemm(w64, 4, dflt, NCU, true), {{64, 256, 0, 64, 1, 2, 4, LDS_64}});
  expect_tiles("wgrad 64 columns, THIN64=0", lw_plan_gemm(w64, 4, arm("MJX_LW_THIN64", "0"), NCU, true), {{128, 256, 0, 64, 1, 2, 4, LDS_128}});
  expect_tiles("wgrad 64 columns, THIN=0", lw_plan_gemm(w64, 4, arm("MJX_LW_THIN", "0"), NCU, true), {{128, 512, 0, 64, 1, 2, 4, LDS_128}});
  expect_tiles("wgrad 100 columns, one split", lw_plan_gemm(w100, 1, dflt, NCU, true), {{128, 512, 0, 100, 1, 2, 1, LDS_128}});
  expect_tiles("wgrad 64 columns, TILES=2", lw_plan_gemm(w64, 4, arm("MJX_LW_TILES", "2"), NCU, true), {{128, 256, 0, 64, 1, 2, 4, LDS_128}});
  expect_tiles("wgrad 384 columns, 4 splits", lw_plan_gemm(gemm_wgrad(3376, 256, 384, AUX, ACT, 384, OUT), 4, dflt, NCU, true),
               {{256, 512, 0, 256, 1, 2, 4, LDS_256}, {128, 512, 256, 128, 1, 2, 4, LDS_128}});
  expect_tiles("wgrad, narrow transposed form", lw_plan_gemm(gemm_wgrad(3376, 17, 256, AUX, ACT, 256, OUT, true), 4, dflt, NCU, true), {{32, 256, 0, 17, 1, 2, 4, LDS_32}});

  // ---- sample splits: ceil(N / chain), capped by wg_cap / tiles, then whole rounds of workgroups over the CUs
  struct { const char* what; const char* sw; const char* val; int64_t N; int ho, hi; bool narrow; int ncu, want; } rows[] = {
      {"humanoid hidden layer", nullptr, nullptr, 3376, 256, 256, false, 256, 4},
      {"narrow output layer", nullptr, nullptr, 3376, 17, 256, true, 256, 4},
      {"one chain", nullptr, nullptr, 1024, 256, 256, false, 256, 1},
      {"one chain + 1", nullptr, nullptr, 1025, 256, 256, false, 256, 2},
      // 2 tiles x 245 splits = 490 workgroups is two rounds on 256 CUs; 2 x 128 is one round of longer workgroups
      {"round balancing: 245 -> 128", nullptr, nullptr, 250000, 256, 256, false, 256, 128},
      {"the same without it", "MJX_LW_SPLITS", "0", 250000, 256, 256, false, 256, 245},
      // 128 x 128 tiles: 4 tiles per split, rounds of 64 splits: 245 (4 rounds) -> 192 (3) -> 128 (2) -> 64 (1)
      {"round balancing, TILES=0", "MJX_LW_TILES", "0", 250000, 256, 256, false, 256, 64},
      // thin gradient (64 columns): two workgroups per CU, 4 x 98 = 392 <= 512 slots is one round already
      {"thin gradient: one round", nullptr, nullptr, 100000, 512, 64, false, 256, 98},
      {"the same on wide tiles", "MJX_LW_THIN", "0", 100000, 512, 64, false, 256, 64},
      {"fewer CUs", nullptr, nullptr, 250000, 256, 256, false, 64, 64},
      {"CHAIN=256 binds", "MJX_LW_CHAIN", "256", 3376, 256, 256, false, 256, 14},
      {"WG_CAP=64 binds", "MJX_LW_WG_CAP", "64", 250000, 256, 256, false, 256, 32},
  };
  for (const auto& r : rows) {
    const int got = wgrad_splits(r.N, r.ho, r.hi, r.narrow, arm(r.sw, r.val), r.ncu);
    CHECK(got == r.want, "wgrad_splits %s: (%lld, %d, %d) -> %d, want %d", r.what, (long long)r.N, r.ho, r.hi, got, r.want);
  }

  CHECK(ew_grid(0) == 1 && ew_grid(256) == 1 && ew_grid(257) == 2 && ew_grid((int64_t)1 << 40) == 8192, "ew_grid");
  if (failures) { printf("lw_plan: %d failures\n", failures); return 1; }
  printf("lw_plan ok\n");
  return 0;
}
