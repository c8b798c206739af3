// fit_host.h -- host side of the baseline and minibatch trainers (baseline.h, mlp_fit.h, policy_fit.h): the feature-table cache and the
// routes of the ridge Gram, the MLP-baseline fit and the policy minibatch fit as plain arithmetic.  Included by mjx.hip after model_host.h.
#pragma once
namespace mjx {

// torch.optim.Adam's bias corrections after t steps, as the k_adam launches take them: 1 - b1^t and sqrt(1 - b2^t)
struct AdamBias { float bc1, bc2s; };
inline AdamBias adam_bias(double b1, double b2, int64_t t) { return {(float)(1.0 - std::pow(b1, (double)t)), (float)std::sqrt(1.0 - std::pow(b2, (double)t))}; }
// ---- ridge baseline: the last feature table of each kind, per thread and device
struct FeatTableCache { int kind = -1, n = -1, F = 0; FeatDesc* dev = nullptr; };
struct FeatTables { FeatTableCache kind[3]; };
inline int get_feat_table(int kind, int n, FeatTableCache** out) {
  static thread_local PerDevice<FeatTables> cache;
  if (kind < 0 || kind > 2 || n <= 0 || n > 4096) return fail(MJX_ERR_ARG, "bad feature kind / obs dim");
  FeatTableCache& c = cache.here().kind[kind];
  if (c.n != n) {
    std::vector<FeatDesc> t = build_feat_table(kind, n);
    if (c.dev) hipFree(c.dev);
    HIPCHK(hipMalloc(&c.dev, t.size() * sizeof(FeatDesc)));
    HIPCHK(hipMemcpy(c.dev, t.data(), t.size() * sizeof(FeatDesc), hipMemcpyHostToDevice));
    c.kind = kind; c.n = n; c.F = (int)t.size();
  }
  *out = &c;
  return MJX_OK;
}
// The Gram kernel for F features (+ the target column) of n observations over N samples (MJX_GRAM_FMA=1, read per call: no_mfma): fp64
// matrix cores with one persistent workgroup per sample range, or one per (128 x 128 block pair, sample range) at ~3 rounds of workgroups
// on the chip, or 64 x 64 tiles on the vector ALU.  Z sample ranges on a grid (gx, Z); k_bl_gram_reduce sums them (`blk` features a side).
enum { GRAM_MFMA, GRAM_MFMA_BLK, GRAM_FMA };
struct GramRoute { int arm, Z, nblk, gx, blk; size_t lds; };
inline GramRoute gram_route(int F, int n, int64_t N, bool no_mfma) {
  const int FA = F + 1, T16 = (FA + 15) / 16;
  auto ranges = [N](int per, int cap) { const int64_t z = (N + per - 1) / per; return (int)(z > cap ? cap : z < 1 ? 1 : z); };
  if (T16 <= GM_TMAX && n <= 24 && !no_mfma)
    return {GRAM_MFMA, ranges(2048, 512), 0, 1, 16, ((size_t)32 * (n + 7) + (size_t)32 * 16 * (T16 | 1)) * sizeof(double)};
  if (!no_mfma && n <= 64) {
    const int nb = (FA + GB_F - 1) / GB_F, nbp = nb * (nb + 1) / 2;
    return {GRAM_MFMA_BLK, ranges(2048, (768 + nbp - 1) / nbp), nb, nbp, GB_F, (size_t)(32 * (n + 7) + 2 * 32 * GB_FS) * sizeof(double)};
  }
  const int nbt = (FA + GT - 1) / GT, npairs = nbt * (nbt + 1) / 2;
  return {GRAM_FMA, ranges(4096, (2048 + npairs - 1) / npairs), nbt, npairs, GT, ((size_t)GKS * n + 2 * (size_t)GKS * (GT + 1)) * sizeof(double)};
}

// ---- MLP-baseline fit (mlp_fit.h): persistent trainers for the reference's default baseline shape, 128 x 128 at minibatches of 64 with at
// least one step and one epoch; every other shape, and every shape no trainer takes, runs the launch route.  HALVES: one workgroup, a step as
// two 32-sample halves, while the layout of d_in inputs fits LDS; ONEPASS: one workgroup, one pass over the 64 rows, up to 23 inputs,
// register-resident moments (REGMOM) only; WIDE: feature slices of MLPFIT_FS on up to MLPFIT_GMAX workgroups of the two-halves trainer.
enum { MLPFIT_LAUNCHES, MLPFIT_HALVES, MLPFIT_ONEPASS, MLPFIT_WIDE };
constexpr int MLPFIT_FS = 48, MLPFIT_GMAX = 16;
// the four switches, read per call: launch route for all / for the wide shapes, moments through L2 (so no one-pass trainer), two halves for all
struct MlpFitSwitches { bool launches, wide, regmom, onepass; };
inline MlpFitSwitches mlp_fit_switches() {
  return {env_flag("MJX_MLP_FIT_LAUNCHES", false), env_flag("MJX_FIT_WIDE", true), env_flag("MJX_FIT_REGMOM", true), env_flag("MJX_FIT_ONEPASS", true)};
}
struct MlpFitRoute { int kind = MLPFIT_LAUNCHES, nf1 = 0, regmom = 0, G = 0; size_t bytes = 0; int site = SITE_MLP_FIT_LAUNCHES; };
inline MlpFitRoute mlp_fit_route(int d_in, const int* hidden, int n_hidden, int batch, int64_t N, int epochs, const MlpFitSwitches& sw) {
  if (sw.launches || n_hidden != 2 || hidden[0] != 128 || hidden[1] != 128 || batch != 64 || N / batch - 1 <= 0 || epochs <= 0) return {};
  const int nf1 = d_in <= 31 ? 1 : 2, G = (d_in + MLPFIT_FS - 1) / MLPFIT_FS;
  const size_t halves = MlpFitLayout<128>(d_in, nf1 == 2).bytes(), onepass = MlpFit1pLayout<128>(d_in).bytes();
  if (d_in <= 63 && halves <= LDS_MAX) {
    if (d_in <= 23 && sw.regmom && sw.onepass && onepass <= LDS_MAX) return {MLPFIT_ONEPASS, nf1, 1, 1, onepass, SITE_MLP_FIT};
    return {MLPFIT_HALVES, nf1, sw.regmom, 1, halves, SITE_MLP_FIT};
  }
  if (sw.wide && d_in > 48 && G <= MLPFIT_GMAX) return {MLPFIT_WIDE, 2, sw.regmom, G, MlpFitLayout<128>(MLPFIT_FS, true).bytes(), SITE_MLP_FIT_WIDE};
  return {};
}
// the one table of the seven trainer instances, in the order they have in the code object: [REGMOM][NF1 - 1], the one-pass trainer, [REGMOM]
typedef void (*MlpFitKernel)(MlpFitArgs);
inline MlpFitKernel mlp_fit_kernel(const MlpFitRoute& r) {
  static const MlpFitKernel halves[2][2] = {{k_mlp_fit<128, 1, false>, k_mlp_fit<128, 2, false>}, {k_mlp_fit<128, 1, true>, k_mlp_fit<128, 2, true>}};
  static const MlpFitKernel onepass = k_mlp_fit1p<128>, wide[2] = {k_mlp_fit<128, 2, false, true>, k_mlp_fit<128, 2, true, true>};
  return r.kind == MLPFIT_ONEPASS ? onepass : r.kind == MLPFIT_WIDE ? wide[r.regmom] : halves[r.regmom][r.nf1 - 1];
}

// ---- policy minibatch fit (policy_fit.h): two layers of H = 64 or 32, minibatches of 8 .. 64 rows in fours, every step in ONE launch; H = 0: none
// serves (MJX_NO_POLICY_FIT=1, read per call: no_fit).  PPO with an old network of its own keeps a third parameter image in LDS.
struct PolicyFitRoute { int H = 0; size_t bytes = 0; };
inline PolicyFitRoute policy_fit_route(int n, int m, const std::vector<int>& hidden, int B, int loss, int old_tracks_new, bool no_fit) {
  if (no_fit || hidden.size() != 2 || hidden[0] != hidden[1] || (hidden[0] != 64 && hidden[0] != 32) || B % 4 || B < 8 || B > 64 ||
      n > hidden[0] || n > 63 || m > 16)
    return {};
  const int H = hidden[0]; const bool old_net = loss == 2 && !old_tracks_new;
  const size_t bytes = 4 * (H == 64 ? PolicyFitLayout<64>(n, m).lds_floats(B, old_net) : PolicyFitLayout<32>(n, m).lds_floats(B, old_net));
  return bytes <= LDS_MAX ? PolicyFitRoute{H, bytes} : PolicyFitRoute{};
}

}  // namespace mjx
