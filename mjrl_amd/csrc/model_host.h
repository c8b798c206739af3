// model_host.h -- host side of the learned-model kernels (dynamics.h, dyn_fit_ens.h, plan.h, path_reward.h, plan_wide.h, policy_rollout.h, policy_rollout_wide.h, rollout_batch.h, rows_wide.h): their shared
// argument checks, their routes as plain arithmetic, and the launches more than one entry makes.  Included by mjx.hip after fail / HIPCHK /
// lds_limit / capped_grid.
#pragma once
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
}  // namespace mjx
