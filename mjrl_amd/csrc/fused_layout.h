// fused_layout.h -- what the fused policy kernels (fused_policy.h) and their host side (fused_host.h) agree on: the modes, the
// kernel's argument block, the LDS layout, the flat parameter offsets, the accumulator-order partial (RawSlab), the tile sizes of
// the two caches, the snapshot length and the rows of the per-action constants.  Host and device, no kernel, no assembly; it is
// written for the HIP compiler (__host__ __device__ members).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace mjx {

enum { MODE_VPG = 0, MODE_FVP = 1, MODE_EVAL = 2 };

struct FusedArgs {
  const float* obs;      // (N, n)
  const float* act;      // (N, m)   VPG / EVAL
  const float* adv;      // (N)      VPG / EVAL
  int64_t N;             // local samples
  float inv_N;           // 1 / N_global
  const float* thetaA;   // new parameters (flat)
  const float* thetaB;   // FVP: the vector v (flat);  VPG/EVAL: old parameters
  const float* trA;      // packed transforms of the new net (never null)
  const float* trB;      // packed transforms of the old net (never null)
  int old_is_new;        // VPG: skip the old forward (LR == 1 exactly)
  float* partials;       // [gridDim.x][d]   VPG / FVP
  double* spartials;     // [gridDim.x][4]
  float* dbg;            // optional dump of tile 0 (block 0, wave 0)
  long long* clk;        // optional: workgroup 0 stamps {cycle, real time} at entry / exit
  int reverse;           // cached FVP: walk the tiles from the far end (alternate launches: what the previous sweep touched
                         // last is still in the memory-side cache when this one starts there)
  float* hcache;         // forward-activation cache [tile][MT1+MT2][4][64 lanes][4]: written by MODE_VPG, read by cached FVP
                         // (FusedLayout::hc_tile floats per tile)
  float* ocache;         // old-policy outputs [tile][MP + 1][32]: mean per action + log-likelihood; written by MODE_VPG
                         // (old == new), read by MODE_EVAL when thetaB / trB still equal `snap` (oc_tile floats per tile)
  const float* snap;     // [snap_len: d + 2n + 2m] parameters and transforms the ocache was computed with
  int snap_trusted;      // MODE_EVAL: the caller vouches that thetaB / trB / trA still equal `snap` (the one-call updates: nothing
                         // outside the library ran since K1) -- the bit-exact compare in the prologue is skipped (~4 us per launch)
  float* snap_out;       // MODE_VPG: the kernel writes that snapshot (thetaB | trB) while it fills the ocache
  int n, m;
  int raw_dr;            // > 0: the gradient partial of a workgroup is written in ACCUMULATOR order (RawSlab<..>::DR floats per
                         // workgroup, see RawSlab below); k_reduce_partials4 maps the columns to the flat order (perm)
};

// the old-policy output cache: floats per 32-sample tile of an instance with mp padded actions -- [mp means + the log-likelihood][32]
__host__ __device__ constexpr int oc_tile(int mp) { return (mp + 1) * 32; }
// the snapshot K1 leaves beside that cache: the d flat parameters, then the packed transforms (in_shift, in_scale: n each;
// out_shift, out_scale: m each)
__host__ __device__ constexpr int tr_len(int n, int m) { return 2 * (n + m); }
template <class T>
__host__ __device__ constexpr T snap_len(T d, int n, int m) { return d + tr_len(n, m); }

// Rows of the per-action constants cst[row][MP] (FusedLayout::oCST); in a struct, so that the short names stay out of namespace
// mjx.  C_FVP2 starts the two rows the product keeps as MP {c3, osc^2 Dk / N} pairs: cst[C_FVP2 * MP + 2 a], + 1.  MODE_EVAL keeps
// mean_kl's per-action constants -- 1 / Dr, sigma_old^2, sigma_new^2, log_std_new - log_std_old -- in the rows only the other modes
// read (over C_DK, the pair rows, C_SG): the 16-action 64 x 64 instance with 17 observations sits exactly AT the 160 KB limit, no
// row to spare.
struct CstRows {
  enum Row { C_OSC = 0, C_OSH, C_SG, C_LS,              // out_scale, out_shift, sigma, log_std of the new net
             C_OSCB, C_OSHB, C_SGB, C_LSB,              // the same of the old net
             C_DK,                                      // Dk = 2 / (2 sigma^2 + 1e-8)
             C_FVP2,                                    // MODE_FVP: the {c3, scale} pairs (two rows)
             C_ISG = C_FVP2 + 2, C_ISGB,                // 1 / sigma new, old
             C_ROWS,
             C_RD = C_DK, C_SO2 = C_FVP2, C_SN2 = C_FVP2 + 1, C_KD = C_SG };   // MODE_EVAL only
  static_assert(C_DK == 8 && C_FVP2 == 9 && C_ISG == 11 && C_ROWS == 13, "cst rows");
};

template <int H1, int H2, int NT1, int MP>
struct FusedLayout {
  static constexpr int MT1 = H1 / 32, MT2 = H2 / 32;
  static constexpr int S2 = H1 + 4;             // row stride of W2 (ds_read_b128, S2/4 odd)
  static constexpr int ST = 36;                 // row stride of [unit][sample] scratch
  static constexpr int S3 = H2 + 4;             // row stride of W3 ([MP][S3])
  static constexpr int HM = (H1 > H2 ? H1 : H2);
  int NP;                                       // features + ones column, padded to 4
  int S1;                                       // row stride of xs / W1a (ds_read_b64, == 2 mod 4)
  int oW1, oW2, oW3, oB2, oB3, SLOT;            // weight slot (one per parameter set)
  int oXS, oXT, oD3, oBA, oBB, WAVE;            // per-wave scratch
  int oTR, oCST, oWAVES, TOTAL;
  static constexpr int NCST = CstRows::C_ROWS;  // rows of per-action constants
  // the forward-activation cache, floats per 32-sample tile: h1, h2 in the sample-lane accumulator layout [mt][q][lane][4] (HC_H),
  // then the normalised observations as the layer-1 operand image [NP / 4][lane][2] (NP: the layout's, or the instance's NPC)
  static constexpr int HC_H = (MT1 + MT2) * 4 * 64 * 4;
  __host__ __device__ static constexpr int hc_tile(int np) { return HC_H + (np / 4) * 128; }
  // eval_only: the layout of MODE_EVAL launches -- no backward pass, so a wave's scratch is just the raw image of its
  // observation tile (3.2 KB instead of 25 KB at HalfCheetah shapes); the workgroup then needs ~64 KB and TWO of them
  // share a CU, i.e. two waves per SIMD: one wave's tanh / likelihood VALU work runs under the other's MFMAs
  // bf3: the cached Fisher-vector product on bf16x3 MFMAs (k_fused<..., BF3 = true>).  After its prologue it reads no fp32 W2 of
  // either slot: the prologue overwrites each slot's W2 region with that matrix's bf16 pieces (F2_IMG floats: V2 in R2's operand
  // order in slot B, W2^T in R8's in slot A), so the region is padded to hold them.  The raw observation image xs is never read
  // by the cached schedule (x~ comes from the cache) and has no room in it.
  static constexpr int F2_IMG = 3 * H1 * H2 / 2;
  __host__ __device__ explicit FusedLayout(int n, bool eval_only = false, bool bf3 = false) {
    NP = (n + 1 + 3) & ~3;
    S1 = NP + 2;
    oW1 = 0;
    oW2 = oW1 + H1 * S1;
    oW3 = oW2 + ((bf3 && H2 * S2 < F2_IMG) ? F2_IMG : H2 * S2);   // [MP][S3]
    oB2 = oW3 + MP * S3;
    oB3 = oB2 + H2;
    SLOT = ((oB3 + MP + 3) / 4) * 4;
    oXS = 0;                                    // raw image of the tile: 32*n floats (+ float4 slack)
    oXT = bf3 ? 0 : ((oXS + 32 * n + 4 * 64 + 3) / 4) * 4; // [NP][ST]
    oD3 = oXT + NP * ST;                        // [MP][ST]
    oBA = oD3 + MP * ST;                        // [HM][ST]
    oBB = oBA + HM * ST;                        // [HM][ST]
    WAVE = eval_only ? ((oXT + 3) / 4) * 4 : ((oBB + HM * ST + 3) / 4) * 4;
    oTR = 2 * SLOT;                             // in_shift / in_scale of A and B: 4 * NP
    oCST = oTR + 4 * NP;                        // per-action constants [NCST][MP]
    oWAVES = oCST + NCST * MP;
    TOTAL = oWAVES + 4 * WAVE;
  }
  __host__ __device__ size_t bytes() const { return (size_t)TOTAL * 4; }
  __host__ __device__ bool fits(int n) const { return n + 1 <= 32 * NT1; }
};

// offsets into the flat parameter vector
struct FlatOff {
  int W1, b1, W2, b2, W3, b3, S, d;
  __host__ __device__ FlatOff(int n, int m, int h1, int h2) {
    W1 = 0; b1 = W1 + h1 * n; W2 = b1 + h1; b2 = W2 + h2 * h1; W3 = b2 + h2; b3 = W3 + m * h2; S = b3 + m; d = S + m;
  }
};

// The gradient partial of a workgroup in ACCUMULATOR order (r06).  The kernels keep the weight gradients in MFMA accumulator
// layout; writing a workgroup's partial in the flat parameter order cost every launch ~8 400 cycles (4 us: per-element index
// arithmetic with the runtime observation width, scattered LDS writes) -- 4 % of a 1M-sample product, 8 % of a 125 k-sample one
// (one rank of eight).  Now every wave drops register r of accumulator X at slot [X][r][lane] of its LDS copy (one ds_write with
// an immediate offset), the four copies are added as they lie, and the COLUMN -> flat index map (a table made once per context
// on the host: perm[], -1 for the padding slots) is applied where each column's 256 partials have been summed
// (k_reduce_partials4).  Same additions in the same order: the same bits as the flat-order epilogue (MJX_RAW_SLAB=0).
template <int H1, int H2, int NT1, int MP, int NPC>
struct RawSlab {
  static constexpr int MT1 = H1 / 32, MT2 = H2 / 32, RA = MP / 2;
  static constexpr int QPI3 = 16 / (MP / 4), UPI3 = 4 * QPI3, NT3 = H2 / UPI3;
  static constexpr int NFQ = NPC ? NPC / 4 : 1;
  static constexpr int oW2 = 0, nW2 = MT2 * MT1 * 16 * 64;                         // [mt][nt][r][lane]
  static constexpr int oW1 = oW2 + nW2, nW1 = NPC ? MT1 * NFQ * 4 * 32 : MT1 * NT1 * 16 * 64;   // [mt][fq][r][lane < 32] | [mt][nt][r][lane]
  static constexpr int oW3 = oW1 + nW1, nW3 = NT3 * 4 * 64;                        // [nt][r][lane]
  static constexpr int oB2 = oW3 + nW3, nB2 = MT2 * 32;                            // [nt][j]
  static constexpr int oB3 = oB2 + nB2;                                            // [r][hi]
  static constexpr int oS = oB3 + 2 * RA;                                          // [r][hi]
  static constexpr int DR = ((oS + 2 * RA) + 3) & ~3;
  static int unit(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
  // perm[slot] = flat parameter index (mirrors the flat-order epilogue of k_fused) or -1; -> true when every flat index is hit exactly once
  static bool fill_perm(int* perm, int n, int m) {
    const FlatOff fo(n, m, H1, H2);
    for (int i = 0; i < DR; ++i) perm[i] = -1;
    auto w1 = [&](int u, int f) { return f < n ? fo.W1 + u * n + f : f == n ? fo.b1 + u : -1; };
    for (int mt = 0; mt < MT2; ++mt) for (int nt = 0; nt < MT1; ++nt) for (int r = 0; r < 16; ++r) for (int l = 0; l < 64; ++l)
      perm[oW2 + ((mt * MT1 + nt) * 16 + r) * 64 + l] = fo.W2 + (32 * mt + unit(r, l >> 5)) * H1 + 32 * nt + (l & 31);
    if (NPC) {
      for (int mt = 0; mt < MT1; ++mt) for (int fq = 0; fq < NFQ; ++fq) for (int r = 0; r < 4; ++r) for (int l = 0; l < 32; ++l)
        perm[oW1 + ((mt * NFQ + fq) * 4 + r) * 32 + l] = w1(32 * mt + 4 * ((l >> 2) & 7) + r, 4 * fq + (l & 3));
    } else {
      for (int mt = 0; mt < MT1; ++mt) for (int nt = 0; nt < NT1; ++nt) for (int r = 0; r < 16; ++r) for (int l = 0; l < 64; ++l)
        perm[oW1 + ((mt * NT1 + nt) * 16 + r) * 64 + l] = w1(32 * mt + unit(r, l >> 5), 32 * nt + (l & 31));
    }
    for (int nt = 0; nt < NT3; ++nt) for (int r = 0; r < 4; ++r) for (int l = 0; l < 64; ++l) {
      const int blk = l >> 2, a = 4 * (blk / QPI3) + r, u = 4 * (blk % QPI3) + (l & 3) + UPI3 * nt;
      perm[oW3 + (nt * 4 + r) * 64 + l] = a < m ? fo.W3 + a * H2 + u : -1;
    }
    for (int nt = 0; nt < MT2; ++nt) for (int jj = 0; jj < 32; ++jj) perm[oB2 + nt * 32 + jj] = fo.b2 + 32 * nt + jj;
    for (int r = 0; r < RA; ++r) for (int hi = 0; hi < 2; ++hi) {
      const int a = unit(r, hi);
      perm[oB3 + 2 * r + hi] = a < m ? fo.b3 + a : -1;
      perm[oS + 2 * r + hi] = a < m ? fo.S + a : -1;
    }
    std::vector<int> hits(fo.d, 0);
    for (int i = 0; i < DR; ++i) if (perm[i] >= 0) { if (perm[i] >= fo.d) return false; ++hits[perm[i]]; }
    for (int i = 0; i < fo.d; ++i) if (hits[i] != 1) return false;
    return true;
  }
};

}  // namespace mjx
