// model_host.h -- host side of the learned-model kernels (dynamics.h, dyn_fit_ens.h, plan.h, path_reward.h, plan_wide.h, policy_rollout.h, policy_rollout_wide.h, rollout_batch.h, rows_wide.h): their shared
// argument checks, their routes as plain arithmetic, the launches more than one entry makes, and the four entries that have a wide
// route (plan rollout, path rewards, policy rollout, rollout disagreement) with their route queries: mjx.hip only forwards to them.
// The rule that orders an entry's routes is plain C++ on top (tests/c/model_host.cpp checks it against a table without a GPU); the
// rest needs the HIP compiler and is included by mjx.hip after fail / HIPCHK / lds_limit / dev_scratch / capped_grid / MJX_DEVICE_ENTRY.
#pragma once
namespace mjx {

// ---- the route ladder.  Route 2 is the wide LDS-tile kernel, route 1 the register-chained instance, route 0 the entry's generic
// tail.  From what was asked (the ..._wide entry), the entry's two switches and what the two shape functions answered: the MFMA
// routes to try, in order (a route whose LDS image the device refuses falls through to the next, at last to route 0), and what a
// call without rows reports, which is the first of them.
struct ModelRoutes {
  int n = 0, route[2] = {0, 0};
  int empty() const { return n ? route[0] : 0; }
};
inline ModelRoutes model_routes(bool asked_wide, bool mfma_on, bool wide_on, bool wide_fits, bool chained_fits) {
  ModelRoutes r;
  if (asked_wide && wide_on && mfma_on && wide_fits) r.route[r.n++] = 2;
  if (mfma_on && chained_fits) r.route[r.n++] = 1;
  return r;
}

}  // namespace mjx

#ifdef __HIPCC__

namespace mjx {

inline int dyn_net(const int* sizes, int n_sizes, DynNet& net) {
  if (!sizes || !net.init(sizes, n_sizes)) return fail(MJX_ERR_ARG, "bad layer sizes (2 .. %d entries, all > 0)", DYN_MAXL + 1);
  return MJX_OK;
}
// K members on gridDim.y (1: a single net), a known activation and target mode, and d_out <= d_in wherever the output is added to the input
inline bool dyn_args_ok(const DynNet& net, int K, int act, int target_mode = DYN_TGT_PLAIN, bool residual = false) {
  return K > 0 && K <= 65535 && (act == DYN_ACT_RELU || act == DYN_ACT_TANH) && target_mode >= DYN_TGT_AFFINE && target_mode <= DYN_TGT_RESIDUAL &&
         !((residual || target_mode == DYN_TGT_RESIDUAL) && net.dout() > net.din());
}
inline void launch_dyn_prep(const float* x, const float* y, int64_t N, int din, int dout, const float* in_tr, const float* out_tr,
                            int target_mode, float* xn, float* tg, hipStream_t st) {
  hipLaunchKernelGGL(k_dyn_prep, dim3(capped_grid(N * (din > dout ? din : dout), 256, 4096)), dim3(256), 0, st, x, y, N, din, dout, in_tr,
                     out_tr, target_mode, xn, tg);
}
// k_model_rollout on K x ceil(N / DYN_RT) workgroups.  The caller has set a.dyn and, where a policy acts, a.pol with its
// parameters, transform, noise and clamps; `actions` given means no policy (a.pol stays empty).
inline int launch_model_rollout(RolloutArgs a, const float* s0, int64_t N, int H, int K, const float* actions, const float* dyn_params,
                                const float* dyn_tr, int act, int flags, float* obs_out, float* act_out, hipStream_t st) {
  const int n = a.dyn.dout(), m = a.dyn.din() - n;
  a.N = N; a.H = H; a.s0 = s0; a.actions = actions; a.dyn_P = dyn_params; a.dyn_tr = dyn_tr; a.act = act; a.flags = flags; a.obs = obs_out; a.act_out = act_out;
  a.W = a.dyn.maxw > a.pol.maxw ? a.dyn.maxw : a.pol.maxw;
  const int64_t Ppol = actions ? 0 : a.pol.P + m;
  const size_t bytes = sizeof(float) * (size_t)(((Ppol + 3) & ~3) + DYN_RT * (n + m) + 4 * DYN_RT * (int64_t)a.W);
  if (int rc = lds_limit((const void*)k_model_rollout, bytes)) return rc;
  hipLaunchKernelGGL(k_model_rollout, dim3((unsigned)((N + DYN_RT - 1) / DYN_RT), (unsigned)K), dim3(256), bytes, st, a);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}
// the one start state of a call tiled to N rows at dst, for k_model_rollout, which reads a state per trajectory -> dst
inline const float* tile_s0(const float* s0, int64_t N, int n, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_plan_tile_s0, dim3(capped_grid(N * n, 256, 1024)), dim3(256), 0, st, s0, N, n, dst);
  return dst;
}

// ---- the three register-chained MFMA routes (k_plan_rollout, k_path_rewards, k_policy_rollout; csrc/mfma_chain.h).  What serves a
// call: the instance's block counts (RB: the reward blocks, path rewards only) and the bytes of its LDS image.
struct ChainShape { int HB = 0, NB = 0, RB = 0; size_t bytes = 0; };
// One launch of such a kernel: 256 threads (the wide kernels: DFE_THREADS), the image as its dynamic LDS.  -> MJX_OK with `launched` set, or the launch's error.
// Not launched: the device refused the image and the caller takes its generic route.  A refusal that is not LDS_OVER came from the
// runtime, whose error is cleared here so that the generic route's own check does not report it.
template <class Args>
inline int launch_chained(void (*kern)(Args), size_t lds_bytes, dim3 grid, const Args& a, hipStream_t st, bool& launched, dim3 block = dim3(256)) {
  launched = false;
  const int e = dyn_lds((const void*)kern, lds_bytes);
  if (e != 0) {
    if (e != LDS_OVER) (void)hipGetLastError();
    return MJX_OK;
  }
  hipLaunchKernelGGL(kern, grid, block, lds_bytes, st, a);
  HIPCHK(hipGetLastError());
  launched = true;
  return MJX_OK;
}

// ---- plan rollout.  The k_plan_rollout instance that serves a net, if one does: exactly two hidden layers, both widths multiples
// of 32 up to 128, n <= 64, actions within the slots a lane keeps ahead, and an LDS image within LDS_MAX (the kernel has no static
// LDS, so the image is its whole footprint).  MJX_PLAN_MFMA=0 (read per call by mjx_plan_rollout): the generic route.
inline bool plan_shape(const DynNet& net, int m, ChainShape& ps) {
  if (net.nl != 3) return false;
  const int n = net.dout(), h1 = net.sz[1], h2 = net.sz[2];
  if (h1 % 32 || h2 % 32 || h1 > 128 || h2 > 128 || n > 64 || pad8(m) > PLAN_MAX_M8) return false;
  ps.HB = (h1 > h2 ? h1 : h2) / 32; ps.NB = (n + 31) / 32;
  ps.bytes = sizeof(float) * plan_lds_floats(ps.HB, ps.NB, n, m);
  return ps.bytes <= LDS_MAX;
}
typedef void (*PlanKernel)(PlanArgs);
inline PlanKernel plan_kernel(int HB, int NB) {
  static const PlanKernel tab[4][2] = {{k_plan_rollout<1, 1>, k_plan_rollout<1, 2>}, {k_plan_rollout<2, 1>, k_plan_rollout<2, 2>},
                                       {k_plan_rollout<3, 1>, k_plan_rollout<3, 2>}, {k_plan_rollout<4, 1>, k_plan_rollout<4, 2>}};
  return tab[HB - 1][NB - 1];
}

// ---- policy rollout.  The k_policy_rollout instance that serves a (policy, dynamics) pair, if one does: a dynamics net as
// plan_shape accepts it, a policy [n, p1, p2, m] with 1 <= p1, p2 <= 64 (each padded to whole 32-blocks in the image; the kernel
// runs the blocks in use, so one instance per dynamics instance serves every policy width), BOTH images together within LDS_MAX
// (the kernel has no static LDS), and an instance that is kept (pol_roll_kept).  MJX_POLICY_ROLLOUT_MFMA=0 (read per call by
// mjx_policy_rollout): the generic route.
inline bool pol_roll_kept(int HB, int NB) { (void)HB; (void)NB; return true; }
inline bool pol_roll_shape(const DynNet& dyn, const DynNet& pol, ChainShape& ps) {
  const int n = dyn.dout(), m = dyn.din() - n;
  ChainShape dp;
  if (!plan_shape(dyn, m, dp) || pol.nl != 3) return false;
  const int p1 = pol.sz[1], p2 = pol.sz[2];
  if (p1 > 32 * POL_MAX_PB || p2 > 32 * POL_MAX_PB || !pol_roll_kept(dp.HB, dp.NB)) return false;
  ps.HB = dp.HB; ps.NB = dp.NB;
  ps.bytes = dp.bytes + sizeof(float) * pol_lds_floats(p1, p2, n, dp.NB);
  return ps.bytes <= LDS_MAX;
}
typedef void (*PolRollKernel)(PolRollArgs);
inline PolRollKernel pol_roll_kernel(int HB, int NB) {
  static const PolRollKernel tab[4][2] = {{k_policy_rollout<1, 1>, k_policy_rollout<1, 2>}, {k_policy_rollout<2, 1>, k_policy_rollout<2, 2>},
                                          {k_policy_rollout<3, 1>, k_policy_rollout<3, 2>}, {k_policy_rollout<4, 1>, k_policy_rollout<4, 2>}};
  return tab[HB - 1][NB - 1];
}
// ---- the wide LDS-tile kernels (dfe_tiles.h: plan_wide.h, policy_rollout_wide.h, rows_wide.h).  A wide kernel takes the dynamics net and the
// net beside it (a policy or a reward net; null: none): exactly two hidden layers each, every hidden width 1 .. 256, n <= 64,
// m <= 64, n + m <= 128.  Plain arithmetic; each kernel adds the bytes of its own LDS layout.
inline bool wide_nets_ok(const DynNet& dyn, const DynNet* other) {
  if (dyn.nl != 3 || (other && other->nl != 3)) return false;
  const int n = dyn.dout(), m = dyn.din() - n;
  for (int l = 1; l <= 2; ++l) if (dyn.sz[l] > WIDE_MAXH || (other && other->sz[l] > WIDE_MAXH)) return false;
  return n <= WIDE_MAXN && m <= WIDE_MAXM && n + m <= WIDE_MAXIN;
}
// The grid of the kernels that walk tiles of stored rows: a workgroup per tile_rows rows up to one workgroup per CU, the K members
// (gridDim.y) sharing the CUs
inline dim3 tile_grid(int64_t rows, int tile_rows, int K) {
  const int64_t tiles = (rows + tile_rows - 1) / tile_rows, cap = (cu_count() + K - 1) / K;
  return dim3((unsigned)(tiles < cap ? tiles : cap), (unsigned)K);
}
// The walk over an entry's MFMA routes: the wide kernel on tiles of wide_tile rows, then the instance `chained` names for ps on
// tiles of 128.  per_cu: the kernels walk stored rows (tile_grid); else a workgroup per tile of trajectories.  -> MJX_OK with
// `route` 2 or 1, whichever launched, or 0: none did and the caller takes its generic route; or a launch's error.
template <class Args>
inline int launch_routes(const ModelRoutes& r, void (*wide)(Args), size_t wide_bytes, int wide_tile, void (*(*chained)(int, int))(Args),
                         const ChainShape& ps, int64_t rows, int K, bool per_cu, const Args& a, hipStream_t st, int& route) {
  auto grid = [&](int tile) { return per_cu ? tile_grid(rows, tile, K) : dim3((unsigned)((rows + tile - 1) / tile), (unsigned)K); };
  route = 0;
  for (int i = 0; i < r.n; ++i) {
    bool launched;
    if (int rc = r.route[i] == 2 ? launch_chained(wide, wide_bytes, grid(wide_tile), a, st, launched, dim3(DFE_THREADS))
                                 : launch_chained(chained(ps.HB, ps.NB), ps.bytes, grid(128), a, st, launched))
      return rc;
    if (launched) { route = r.route[i]; break; }
  }
  return MJX_OK;
}
// an entry's last statement: the route that served the call, where the caller asked for it
inline int route_done(int* route_out, int route) { if (route_out) *route_out = route; return MJX_OK; }
// ---- wide policy rollout.  What k_policy_rollout_wide (policy_rollout_wide.h) serves: nets as wide_nets_ok takes them and its LDS
// layout (the kernel has no static LDS) within LDS_MAX.  It does not ask what pol_roll_shape answers: the shapes the chained
// kernel takes are served as well.  MJX_POLICY_ROLLOUT_WIDE=0 or MJX_POLICY_ROLLOUT_MFMA=0 (read per call by
// mjx_policy_rollout_wide): mjx_policy_rollout's routes.
inline bool wide_roll_shape(const DynNet& dyn, const DynNet& pol, size_t& bytes) {
  if (!wide_nets_ok(dyn, &pol)) return false;
  const int n = dyn.dout(), m = dyn.din() - n;
  bytes = sizeof(float) * wide_roll_lds_floats(n, m, dyn.sz[1], dyn.sz[2], pol.sz[1], pol.sz[2]);
  return bytes <= LDS_MAX;
}
// ---- wide plan rollout.  What k_plan_rollout_wide (plan_wide.h) serves: a dynamics net as wide_nets_ok takes it and its LDS layout
// (the kernel has no static LDS) within LDS_MAX.  It does not ask what plan_shape answers: the shapes the chained kernel takes are
// served as well.  MJX_PLAN_WIDE=0 or MJX_PLAN_MFMA=0 (read per call by mjx_plan_rollout_wide): mjx_plan_rollout's routes.
inline bool wide_plan_shape(const DynNet& dyn, size_t& bytes) {
  if (!wide_nets_ok(dyn, nullptr)) return false;
  const int n = dyn.dout(), m = dyn.din() - n;
  bytes = sizeof(float) * plan_wide_lds_floats(n, m, dyn.sz[1], dyn.sz[2]);
  return bytes <= LDS_MAX;
}
// the two nets of one call, parsed: sizes that fit each other ([n, p..., m] and [n + m, h..., n])
inline int pol_roll_nets(const int* pol_sizes, int pol_n_sizes, const int* dyn_sizes, int dyn_n_sizes, DynNet& pol, DynNet& dyn) {
  if (int rc = dyn_net(dyn_sizes, dyn_n_sizes, dyn)) return rc;
  if (int rc = dyn_net(pol_sizes, pol_n_sizes, pol)) return rc;
  const int n = dyn.dout(), m = dyn.din() - n;
  if (m <= 0 || pol.din() != n || pol.dout() != m) return fail(MJX_ERR_ARG, "sizes must be [n, p..., m] and [n + m, h..., n] with m > 0");
  return MJX_OK;
}
// the remaining arguments of mjx_policy_rollout / mjx_policy_rollout_wide
inline bool pol_roll_args_ok(const DynNet& dyn, const float* s0, int64_t s0_stride, int64_t N, int H, int K, const float* pol_params,
                             const float* pol_tr, int64_t noise_stride, const float* dyn_params, const float* dyn_tr, int act, int flags,
                             const float* a_min, const float* a_max, const float* s_min, const float* s_max, const float* obs_out,
                             const float* act_out) {
  const int n = dyn.dout(), m = dyn.din() - n;
  return !(!s0 || !pol_params || !pol_tr || !dyn_params || !dyn_tr || !obs_out || !act_out || N < 0 || H < 0 || !dyn_args_ok(dyn, K, act) ||
           (flags & ~(DYN_OUT_AFFINE | DYN_MASK | DYN_RESIDUAL)) || (s0_stride != 0 && s0_stride != n) ||
           (noise_stride != 0 && noise_stride != (int64_t)H * N * m) || (!a_min) != (!a_max) || (!s_min) != (!s_max));
}

// ---- learned path rewards.  The k_path_rewards instance that serves a (dynamics, reward) pair, if one does: a dynamics net as
// plan_shape accepts it, a reward net [2 n + m, g1, g2, 1] with 1 <= g1, g2 <= 128, and BOTH images together within LDS_MAX (the
// kernel has no static LDS).  Each reward width is padded to whole 32-blocks in the image (W2's K dimension to the first width's
// blocks) and the kernel runs the blocks in use, so one instance per dynamics instance serves every reward width (eight in all, as
// many as the plan rollout has): up to four reward blocks beside HB <= 3, up to two (widths <= 64) beside the 128-wide dynamics
// nets, where four would spill registers to scratch and 100 x 100 (205 KB together) would not fit anyway.
// MJX_PATH_REWARDS_MFMA=0 (read per call by mjx_path_rewards): the generic route.
inline bool path_rew_shape(const DynNet& dyn, const DynNet& rew, ChainShape& ps) {
  const int n = dyn.dout(), m = dyn.din() - n;
  ChainShape dp;
  if (!plan_shape(dyn, m, dp) || rew.nl != 3) return false;
  const int g1 = rew.sz[1], g2 = rew.sz[2];
  ps.HB = dp.HB; ps.NB = dp.NB; ps.RB = dp.HB == 4 ? 2 : 4;
  if (g1 > 32 * ps.RB || g2 > 32 * ps.RB) return false;
  ps.bytes = dp.bytes + sizeof(float) * path_rew_lds_floats(g1, g2, n, m);
  return ps.bytes <= LDS_MAX;
}
typedef void (*PathRewKernel)(PathRewArgs);
inline PathRewKernel path_rew_kernel(int HB, int NB) {
  static const PathRewKernel tab[4][2] = {{k_path_rewards<1, 1, 4>, k_path_rewards<1, 2, 4>}, {k_path_rewards<2, 1, 4>, k_path_rewards<2, 2, 4>},
                                          {k_path_rewards<3, 1, 4>, k_path_rewards<3, 2, 4>}, {k_path_rewards<4, 1, 2>, k_path_rewards<4, 2, 2>}};
  return tab[HB - 1][NB - 1];
}
// the two nets of one call, parsed: sizes that fit each other ([n + m, h..., n] and [2 n + m, g..., 1])
inline int path_rew_nets(const int* dyn_sizes, int dyn_n_sizes, const int* rew_sizes, int rew_n_sizes, DynNet& dyn, DynNet& rew) {
  if (int rc = dyn_net(dyn_sizes, dyn_n_sizes, dyn)) return rc;
  if (int rc = dyn_net(rew_sizes, rew_n_sizes, rew)) return rc;
  const int n = dyn.dout(), m = dyn.din() - n;
  if (m <= 0 || rew.dout() != 1 || rew.din() != 2 * n + m) return fail(MJX_ERR_ARG, "sizes must be [n + m, h..., n] and [2 n + m, g..., 1] with m > 0");
  return MJX_OK;
}

// ---- disagreement of stored rollouts.  The k_rollout_disagree instance is the one plan_shape names: the kernel holds the dynamics
// image alone.  MJX_ROLLOUT_DISAGREE_MFMA=0 (read per call by mjx_rollout_disagreement): the generic route.
typedef void (*RollDisKernel)(RollDisArgs);
inline RollDisKernel roll_dis_kernel(int HB, int NB) {
  static const RollDisKernel tab[4][2] = {{k_rollout_disagree<1, 1>, k_rollout_disagree<1, 2>}, {k_rollout_disagree<2, 1>, k_rollout_disagree<2, 2>},
                                          {k_rollout_disagree<3, 1>, k_rollout_disagree<3, 2>}, {k_rollout_disagree<4, 1>, k_rollout_disagree<4, 2>}};
  return tab[HB - 1][NB - 1];
}
// the net of one call, parsed: [n + m, h..., n] with m > 0
inline int roll_dis_net(const int* dyn_sizes, int dyn_n_sizes, DynNet& dyn) {
  if (int rc = dyn_net(dyn_sizes, dyn_n_sizes, dyn)) return rc;
  if (dyn.din() <= dyn.dout()) return fail(MJX_ERR_ARG, "dyn_sizes must be [n + m, h..., n] with m > 0");
  return MJX_OK;
}

// the remaining arguments of mjx_rollout_disagreement / mjx_rollout_disagreement_wide
inline bool roll_dis_args_ok(const DynNet& dyn, const float* obs, const float* act, int64_t P, int H, int K, const float* dyn_params,
                             const float* dyn_tr, int dyn_act, int dyn_flags, const float* err_out) {
  return !(!obs || !act || !dyn_params || !dyn_tr || !err_out || P < 0 || H < 0 || (dyn_flags & ~(DYN_OUT_AFFINE | DYN_MASK | DYN_RESIDUAL)) ||
           !dyn_args_ok(dyn, K, dyn_act, DYN_TGT_PLAIN, dyn_flags & DYN_RESIDUAL));
}
// ... and of mjx_path_rewards / mjx_path_rewards_wide
inline bool path_rew_args_ok(const DynNet& dyn, const DynNet& rew, const float* obs, const float* act, int64_t act_stride, int64_t rows, int K,
                             const float* dyn_params, const float* dyn_tr, int dyn_act, int dyn_flags, const float* rew_params,
                             const float* rew_tr, int rew_act, const float* r32_out, const double* r64_out) {
  const int m = dyn.din() - dyn.dout();
  return !(!obs || !act || !dyn_params || !dyn_tr || !rew_params || !rew_tr || (!r32_out && !r64_out) || rows < 0 ||
           (act_stride != 0 && act_stride != rows * m) || (dyn_flags & ~(DYN_OUT_AFFINE | DYN_MASK | DYN_RESIDUAL)) ||
           !dyn_args_ok(dyn, K, dyn_act, DYN_TGT_PLAIN, dyn_flags & DYN_RESIDUAL) || !dyn_args_ok(rew, K, rew_act));
}

// ---- the wide passes over stored rollouts.  What k_rollout_disagree_wide (rew null) and k_path_rewards_wide (rows_wide.h) serve:
// nets as wide_nets_ok takes them and the LDS layout (the kernels have no static LDS) within LDS_MAX.  They do not ask what
// plan_shape / path_rew_shape answer: the shapes the chained kernels take are served as well.  MJX_ROLLOUT_DISAGREE_WIDE=0 /
// MJX_PATH_REWARDS_WIDE=0 or the matching ..._MFMA=0 (read per call by mjx_rollout_disagreement_wide / mjx_path_rewards_wide): the
// narrow entry's routes.
inline bool wide_rows_shape(const DynNet& dyn, const DynNet* rew, size_t& bytes) {
  if (!wide_nets_ok(dyn, rew)) return false;
  const int n = dyn.dout(), m = dyn.din() - n;
  bytes = sizeof(float) * rows_wide_lds_floats(n, m, dyn.sz[1], dyn.sz[2], rew ? rew->sz[1] : 0, rew ? rew->sz[2] : 0);
  return bytes <= LDS_MAX;
}

// ---- dynamics fit.  k_dyn_fit, the persistent trainer, serves hidden widths <= 128 at minibatches <= 64 (shape) whose activations fit in LDS beside
// its static LDS (128 B; asked of the runtime only where the shape leaves the question open); MJX_DYN_FIT_LAUNCHES=1, read per call: the launch route.
inline size_t dyn_fit_lds_bytes(const DynNet& net, int B) {
  int wmax = 0; size_t acts = 0;
  for (int l = 0; l <= net.nl; ++l) acts += net.sz[l];
  for (int l = 1; l <= net.nl; ++l) wmax = net.sz[l] > wmax ? net.sz[l] : wmax;
  return sizeof(float) * (size_t)B * (acts + net.dout() + 2 * (size_t)wmax);
}
inline bool dyn_fit_shape(const DynNet& net, int batch, bool force_launches) {
  for (int l = 1; l < net.nl; ++l) if (net.sz[l] > 128) return false;
  return !force_launches && batch <= 64;
}
inline bool dyn_fit_persistent(size_t bytes, size_t static_bytes) { return static_bytes + bytes <= LDS_MAX; }
// The shapes k_dyn_fit_ens serves (MJX_DYN_FIT_ENS=0, read per call: none).  Plain arithmetic.
inline bool dfe_serves(const DynNet& net, int batch, int target_mode) {
  if (net.nl != 3 || batch < 1 || batch > DFE_MAXB) return false;
  if (target_mode != DYN_TGT_PLAIN && target_mode != DYN_TGT_RESIDUAL) return false;
  for (int l = 1; l <= 2; ++l) if (net.sz[l] % 32 || net.sz[l] < 32 || net.sz[l] > DFE_MAXH) return false;
  return net.din() <= DFE_MAXIN && net.dout() <= DFE_MAXOUT;
}
// The shapes k_dyn_fit_ens<true> serves for mjx_reward_fit_ensemble (target mode 0; MJX_REWARD_FIT_ENS=0, read per call: none): any two
// hidden widths the padded tiles hold.  Plain arithmetic.
inline bool reward_fit_serves(const DynNet& net, int batch) {
  if (net.nl != 3 || batch < 1 || batch > DFE_MAXB) return false;
  for (int l = 1; l <= 2; ++l) if (net.sz[l] < 1 || net.sz[l] > DFE_MAXH) return false;
  return net.din() <= DFE_MAXIN && net.dout() <= DFE_MAXOUT;
}

// ---------------------------------------------------------------------------- the four entries with a wide route, and their route queries
// Each: parse the nets, check the arguments, model_routes from the entry's two switches (read per call: A/B runs in one process;
// ..._MFMA=0 means no MFMA route at all) and its two shape functions, the answer of a call without rows before any device work,
// launch_routes, then the entry's own generic tail.  `wide`: the ..._wide entry (the query: of the wide route).

// ---- MPC planning on learned models (plan.h, plan_wide.h)
inline int plan_route(bool wide, const int* dyn_sizes, int dyn_n_sizes, int act_dim) {
  DynNet net;
  if (int rc = dyn_net(dyn_sizes, dyn_n_sizes, net)) return rc;
  if (act_dim <= 0 || net.din() != net.dout() + act_dim) return fail(MJX_ERR_ARG, "dyn_sizes must be [n + m, h..., n] with m = act_dim > 0");
  ChainShape ps; size_t bytes;
  return (wide ? wide_plan_shape(net, bytes) : plan_shape(net, act_dim, ps)) ? 1 : 0;
}
// (mjx_plan_rollout takes any flags, as it always has; mjx_plan_rollout_wide refuses unknown bits)
inline int plan_rollout(bool wide, const float* s0, int64_t s0_stride, int64_t N, int H, int K, const float* actions, const int* dyn_sizes,
                        int dyn_n_sizes, const float* dyn_params, const float* dyn_tr, int act, int flags, float* obs_out, int* route_out,
                        void* stream) {
  DynNet net;
  if (int rc = dyn_net(dyn_sizes, dyn_n_sizes, net)) return rc;
  const int n = net.dout(), m = net.din() - n;
  if (!s0 || !actions || !dyn_params || !dyn_tr || !obs_out || N < 0 || H < 0 || m <= 0 || (s0_stride != 0 && s0_stride != n) ||
      !dyn_args_ok(net, K, act) || (wide && (flags & ~(DYN_OUT_AFFINE | DYN_MASK | DYN_RESIDUAL))))
    return fail(MJX_ERR_ARG, "bad arguments");
  ChainShape ps; size_t wide_bytes = 0;
  const ModelRoutes r = model_routes(wide, env_flag("MJX_PLAN_MFMA", true), env_flag("MJX_PLAN_WIDE", true), wide_plan_shape(net, wide_bytes),
                                     plan_shape(net, m, ps));
  if (N == 0 || H == 0) return route_done(route_out, r.empty());
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  const PlanArgs p{s0, s0_stride, actions, dyn_params, dyn_tr, obs_out, N, net.P, H, n, m, net.sz[1], net.sz[2], act, flags};
  int route;
  if (int rc = launch_routes(r, k_plan_rollout_wide, wide_bytes, 32, plan_kernel, ps, N, K, false, p, st, route)) return rc;
  if (route) return route_done(route_out, route);
  // generic route: k_model_rollout with the actions given, as mjx_model_rollout launches it; its action copy and the tiled
  // start state go to scratch
  float* scr = nullptr;
  const size_t act_floats = (size_t)K * N * H * m, s0_floats = s0_stride ? 0 : (size_t)N * n;
  if (int rc = dev_scratch(SITE_PLAN_ROLLOUT, stream, (act_floats + s0_floats) * sizeof(float), &scr)) return rc;
  if (!s0_stride) s0 = tile_s0(s0, N, n, scr + act_floats, st);
  RolloutArgs a{};
  a.dyn = net;
  if (int rc = launch_model_rollout(a, s0, N, H, K, actions, dyn_params, dyn_tr, act, flags, obs_out, scr, st)) return rc;
  return route_done(route_out, 0);
}

// ---- learned path rewards (path_reward.h, rows_wide.h)
inline int path_rewards_route(bool wide, const int* dyn_sizes, int dyn_n_sizes, const int* rew_sizes, int rew_n_sizes) {
  DynNet dyn, rew;
  if (int rc = path_rew_nets(dyn_sizes, dyn_n_sizes, rew_sizes, rew_n_sizes, dyn, rew)) return rc;
  ChainShape ps; size_t bytes;
  return (wide ? wide_rows_shape(dyn, &rew, bytes) : path_rew_shape(dyn, rew, ps)) ? 1 : 0;
}
inline int path_rewards(bool wide, const float* obs, const float* act, int64_t act_stride, int64_t rows, int K, const int* dyn_sizes,
                        int dyn_n_sizes, const float* dyn_params, const float* dyn_tr, int dyn_act, int dyn_flags, const int* rew_sizes,
                        int rew_n_sizes, const float* rew_params, const float* rew_tr, int rew_act, float* r32_out, double* r64_out,
                        int* route_out, void* stream) {
  DynNet dyn, rew;
  if (int rc = path_rew_nets(dyn_sizes, dyn_n_sizes, rew_sizes, rew_n_sizes, dyn, rew)) return rc;
  const int n = dyn.dout(), m = dyn.din() - n;
  if (!path_rew_args_ok(dyn, rew, obs, act, act_stride, rows, K, dyn_params, dyn_tr, dyn_act, dyn_flags, rew_params, rew_tr, rew_act, r32_out, r64_out))
    return fail(MJX_ERR_ARG, "bad arguments");
  ChainShape ps; size_t wide_bytes = 0;
  const ModelRoutes r = model_routes(wide, env_flag("MJX_PATH_REWARDS_MFMA", true), env_flag("MJX_PATH_REWARDS_WIDE", true),
                                     wide_rows_shape(dyn, &rew, wide_bytes), path_rew_shape(dyn, rew, ps));
  if (rows == 0) return route_done(route_out, r.empty());
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  const PathRewArgs a{obs, act, act_stride, dyn_params, dyn_tr, rew_params, rew_tr, r32_out, r64_out, rows, dyn.P, rew.P,
                      n, m, dyn.sz[1], dyn.sz[2], dyn_act, dyn_flags, rew.sz[1], rew.sz[2], rew_act};
  // (route 1: a wave owns tiles of 32 rows; one workgroup per CU holds the image, so the K members share the CUs and a wave walks
  //  the tiles beyond that -- the staging prologue is paid once per workgroup)
  int route;
  if (int rc = launch_routes(r, k_path_rewards_wide<RW_NS>, wide_bytes, 32 * RW_NS, path_rew_kernel, ps, rows, K, true, a, st, route)) return rc;
  if (route) return route_done(route_out, route);
  // generic route: mjx_dyn_forward's kernel twice, over [s, a] and over [s, a, s'], both assembled in scratch
  const int din = n + m, rin = din + n;
  const int64_t kr = (int64_t)K * rows;
  float* scr = nullptr;
  if (int rc = dev_scratch(SITE_PATH_REWARDS, stream, (size_t)kr * (din + rin + n + 1) * sizeof(float), &scr)) return rc;
  float* X1 = scr; float* X2 = X1 + kr * din; float* sp = X2 + kr * rin; float* r32 = r32_out ? r32_out : sp + kr * n;
  const size_t b1 = sizeof(float) * 3 * DYN_FT * (size_t)dyn.maxw, b2 = sizeof(float) * 3 * DYN_FT * (size_t)rew.maxw;
  if (int rc = lds_limit((const void*)k_dyn_forward, b1 > b2 ? b1 : b2)) return rc;
  const dim3 grid((unsigned)((rows + DYN_FT - 1) / DYN_FT), (unsigned)K);
  hipLaunchKernelGGL(k_pr_gather_sa, dim3(capped_grid(kr * din, 256, 4096)), dim3(256), 0, st, obs, act, act_stride, rows, K, n, m, X1, X2);
  DynFwdArgs fa{dyn, X1, rows * din, rows, dyn_params, dyn_tr, dyn_act, dyn_flags, sp};
  hipLaunchKernelGGL(k_dyn_forward, grid, dim3(256), b1, st, fa);
  hipLaunchKernelGGL(k_pr_gather_sp, dim3(capped_grid(kr * n, 256, 4096)), dim3(256), 0, st, sp, kr, n, m, X2);
  DynFwdArgs fr{rew, X2, rows * rin, rows, rew_params, rew_tr, rew_act, DYN_OUT_AFFINE, r32};
  hipLaunchKernelGGL(k_dyn_forward, grid, dim3(256), b2, st, fr);
  if (r64_out) hipLaunchKernelGGL(k_pr_widen, dim3(capped_grid(kr, 256, 4096)), dim3(256), 0, st, r32, kr, r64_out);
  HIPCHK(hipGetLastError());
  return route_done(route_out, 0);
}

// ---- policy rollout on learned models (policy_rollout.h, policy_rollout_wide.h)
inline int policy_rollout_route(bool wide, const int* pol_sizes, int pol_n_sizes, const int* dyn_sizes, int dyn_n_sizes) {
  DynNet pol, dyn;
  if (int rc = pol_roll_nets(pol_sizes, pol_n_sizes, dyn_sizes, dyn_n_sizes, pol, dyn)) return rc;
  ChainShape ps; size_t bytes;
  return (wide ? wide_roll_shape(dyn, pol, bytes) : pol_roll_shape(dyn, pol, ps)) ? 1 : 0;
}
inline int policy_rollout(bool wide, const float* s0, int64_t s0_stride, int64_t N, int H, int K, const int* pol_sizes, int pol_n_sizes,
                          const float* pol_params, const float* pol_tr, const float* noise, int64_t noise_stride, const int* dyn_sizes,
                          int dyn_n_sizes, const float* dyn_params, const float* dyn_tr, int act, int flags, const float* a_min,
                          const float* a_max, const float* s_min, const float* s_max, float* obs_out, float* act_out, int* route_out,
                          void* stream) {
  RolloutArgs a{};
  if (int rc = pol_roll_nets(pol_sizes, pol_n_sizes, dyn_sizes, dyn_n_sizes, a.pol, a.dyn)) return rc;
  const int n = a.dyn.dout(), m = a.dyn.din() - n;
  if (!pol_roll_args_ok(a.dyn, s0, s0_stride, N, H, K, pol_params, pol_tr, noise_stride, dyn_params, dyn_tr, act, flags, a_min, a_max, s_min,
                        s_max, obs_out, act_out))
    return fail(MJX_ERR_ARG, "bad arguments");
  ChainShape ps; size_t wide_bytes = 0;
  const ModelRoutes r = model_routes(wide, env_flag("MJX_POLICY_ROLLOUT_MFMA", true), env_flag("MJX_POLICY_ROLLOUT_WIDE", true),
                                     wide_roll_shape(a.dyn, a.pol, wide_bytes), pol_roll_shape(a.dyn, a.pol, ps));
  if (N == 0 || H == 0) return route_done(route_out, r.empty());
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  const PolRollArgs p{s0, s0_stride, noise, noise_stride ? (int64_t)H : 0, pol_params, pol_tr, dyn_params, dyn_tr, a_min, a_max, s_min, s_max,
                      obs_out, act_out, N, a.dyn.P, H, n, m, a.dyn.sz[1], a.dyn.sz[2], act, flags, a.pol.sz[1], a.pol.sz[2]};
  int route;
  if (int rc = launch_routes(r, k_policy_rollout_wide, wide_bytes, 32, pol_roll_kernel, ps, N, K, false, p, st, route)) return rc;
  if (route) return route_done(route_out, route);
  // generic route: k_model_rollout as mjx_model_rollout launches it; the tiled start state and the K copies of a shared noise
  // block go to the calling thread's scratch block of this site on (device, stream)
  const size_t s0_floats = s0_stride ? 0 : (size_t)N * n, nz_floats = (noise && !noise_stride && K > 1) ? (size_t)K * H * N * m : 0;
  if (s0_floats + nz_floats) {
    float* scr = nullptr;
    if (int rc = dev_scratch(SITE_POLICY_ROLLOUT, stream, (s0_floats + nz_floats) * sizeof(float), &scr)) return rc;
    if (s0_floats) s0 = tile_s0(s0, N, n, scr, st);
    if (nz_floats) {
      hipLaunchKernelGGL(k_pol_expand_noise, dim3(capped_grid((int64_t)nz_floats, 256, 4096)), dim3(256), 0, st, noise, (int64_t)H * N * m, K,
                         scr + s0_floats);
      noise = scr + s0_floats;
    }
    HIPCHK(hipGetLastError());
  }
  a.pol_P = pol_params; a.pol_tr = pol_tr; a.noise = noise; a.a_lo = a_min; a.a_hi = a_max; a.s_lo = s_min; a.s_hi = s_max;
  if (int rc = launch_model_rollout(a, s0, N, H, K, nullptr, dyn_params, dyn_tr, act, flags, obs_out, act_out, st)) return rc;
  return route_done(route_out, 0);
}

// ---- disagreement of stored rollouts (rollout_batch.h, rows_wide.h)
inline int rollout_disagreement_route(bool wide, const int* dyn_sizes, int dyn_n_sizes) {
  DynNet dyn;
  if (int rc = roll_dis_net(dyn_sizes, dyn_n_sizes, dyn)) return rc;
  ChainShape ps; size_t bytes;
  return (wide ? wide_rows_shape(dyn, nullptr, bytes) : plan_shape(dyn, dyn.din() - dyn.dout(), ps)) ? 1 : 0;
}
inline int rollout_disagreement(bool wide, const float* obs, const float* act, int64_t P, int H, int K, const int* dyn_sizes, int dyn_n_sizes,
                                const float* dyn_params, const float* dyn_tr, int dyn_act, int dyn_flags, float* err_out, int* route_out,
                                void* stream) {
  DynNet dyn;
  if (int rc = roll_dis_net(dyn_sizes, dyn_n_sizes, dyn)) return rc;
  const int n = dyn.dout(), m = dyn.din() - n;
  if (!roll_dis_args_ok(dyn, obs, act, P, H, K, dyn_params, dyn_tr, dyn_act, dyn_flags, err_out)) return fail(MJX_ERR_ARG, "bad arguments");
  ChainShape ps; size_t wide_bytes = 0;
  const ModelRoutes r = model_routes(wide, env_flag("MJX_ROLLOUT_DISAGREE_MFMA", true), env_flag("MJX_ROLLOUT_DISAGREE_WIDE", true),
                                     wide_rows_shape(dyn, nullptr, wide_bytes), plan_shape(dyn, m, ps));
  if (P == 0 || H <= 1) return route_done(route_out, r.empty());
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = P * H, R = P * (H - 1);
  const int din = n + m;
  // one block serves every route: member means (K x R) on routes 1 and 2, [s, a] rows and predictions (R x din, K x R x n) on route 0
  float* scr = nullptr;
  if (int rc = dev_scratch(SITE_ROLLOUT_DISAGREE, stream, (size_t)R * (din + (size_t)K * n) * sizeof(float), &scr)) return rc;
  const RollDisArgs a{obs, act, dyn_params, dyn_tr, scr, rows, dyn.P, H, n, m, dyn.sz[1], dyn.sz[2], dyn_act, dyn_flags};
  int route;
  if (int rc = launch_routes(r, k_rollout_disagree_wide<RW_NS>, wide_bytes, 32 * RW_NS, roll_dis_kernel, ps, rows, K, true, a, st, route)) return rc;
  if (route) {                                              // the members' means lie in scratch: their maximum, in member order
    hipLaunchKernelGGL(k_rd_max, dim3(capped_grid(R, 256, 4096)), dim3(256), 0, st, scr, K, R, err_out);
    HIPCHK(hipGetLastError());
    return route_done(route_out, route);
  }
  // generic route: mjx_dyn_forward's kernel over the gathered [s, a] rows (shared by the members), then mjx_dyn_pred_error's arithmetic
  float* X = scr; float* pred = X + R * din;
  const size_t bytes = sizeof(float) * 3 * DYN_FT * (size_t)dyn.maxw;
  if (int rc = lds_limit((const void*)k_dyn_forward, bytes)) return rc;
  hipLaunchKernelGGL(k_rd_gather, dim3(capped_grid(R * din, 256, 4096)), dim3(256), 0, st, obs, act, R, H, n, m, X);
  DynFwdArgs fa{dyn, X, 0, R, dyn_params, dyn_tr, dyn_act, dyn_flags, pred};
  hipLaunchKernelGGL(k_dyn_forward, dim3((unsigned)((R + DYN_FT - 1) / DYN_FT), (unsigned)K), dim3(256), bytes, st, fa);
  hipLaunchKernelGGL(k_rd_reduce, dim3(capped_grid(R, 256, 4096)), dim3(256), 0, st, pred, obs, K, R, H, n, err_out);
  HIPCHK(hipGetLastError());
  return route_done(route_out, 0);
}
}  // namespace mjx

#endif  // __HIPCC__
