// fit_host.h -- host side of the baseline and minibatch trainers (baseline.h, mlp_fit.h, mlp_fit_team.h, dynamics.h, dyn_fit_ens.h, dyn_fit_ens_team.h, policy_fit.h, policy_fit_wide.h):
// the feature-table cache, the routes of the ridge Gram, the MLP-baseline predict and fit and the policy minibatch fit as plain arithmetic, and
// what acts on a route -- the bodies of the predict and fit entries; mjx.hip checks arguments and forwards.  Included by mjx.hip after model_host.h
// (DynNet's helpers) and before update_host.h: the policy fit takes the pieces of mjx_ctx it uses as parameters.
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

// ---- MLP-baseline predict (baseline.h): the reference's default value network (128 x 128 ReLU) in one launch of k_mlp_predict128
// (MJX_MLP_PREDICT_FUSED=0, read per call: A/B); every other shape layer by layer, in chunks of 2^17 rows
inline bool mlp_predict_route(int d_in, const int* hidden, int n_hidden, const float* params) {
  return env_flag("MJX_MLP_PREDICT_FUSED", true) && n_hidden == 2 && hidden[0] == 128 && hidden[1] == 128 && d_in <= 64 &&
         (((uintptr_t)params) & 15) == 0 && mlp_predict_lds_bytes(d_in) <= LDS_MAX;
}
inline int mlp_predict(const float* feat, int64_t N, int d_in, const int* hidden, int n_hidden, const float* params, float* out, void* stream) {
  if (mlp_predict_route(d_in, hidden, n_hidden, params)) {
    const size_t bytes = mlp_predict_lds_bytes(d_in);
    if (int rc = lds_limit((const void*)k_mlp_predict128, bytes)) return rc;
    const int ncu = cu_count();
    const int64_t ntiles = (N + 31) / 32;
    const int64_t want = (ntiles + 7) / 8;
    MlpPredictArgs pa{feat, params, out, N, d_in};
    hipLaunchKernelGGL(k_mlp_predict128, dim3((unsigned)(want < ncu ? want : ncu)), dim3(512), bytes, (hipStream_t)stream, pa);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  MlpRegressor net; net.init(d_in, hidden, n_hidden);
  const int64_t CH = 1 << 17;
  size_t per_row = 0; for (int i = 0; i < n_hidden; ++i) per_row += hidden[i];
  // (the activation scratch is per stream: MLPBaseline.fit_async runs its before / after forwards on a side stream while the
  //  caller's stream may be predicting with another baseline -- one shared block would be written by both at once)
  float* sc = nullptr;
  if (int rc = dev_scratch(SITE_MLP_PREDICT, stream, (size_t)CH * (per_row ? per_row : 1) * sizeof(float), &sc)) return rc;
  std::vector<float*> acts(n_hidden);
  { float* q = sc; for (int i = 0; i < n_hidden; ++i) { acts[i] = q; q += (size_t)CH * hidden[i]; } }
  for (int64_t r0 = 0; r0 < N; r0 += CH) {
    int64_t rows = (N - r0 < CH) ? N - r0 : CH;
    net.forward(params, feat + r0 * d_in, rows, acts, out + r0, (hipStream_t)stream);
  }
  HIPCHK(lw_status());
  return MJX_OK;
}

// ---- MLP-baseline fit (mlp_fit.h): persistent trainers for the reference's default baseline shape, 128 x 128 at minibatches of 64 with at
// least one step and one epoch; every other shape, and every shape no trainer takes, runs the launch route.  HALVES: one workgroup, a step as
// two 32-sample halves, while the layout of d_in inputs fits LDS; ONEPASS: one workgroup, one pass over the 64 rows, up to 23 inputs,
// register-resident moments (REGMOM) only; WIDE: feature slices of MLPFIT_FS on up to MLPFIT_GMAX workgroups of the two-halves trainer.
// TEAM (mlp_fit_team.h): the same shape at minibatches of 128, 192 .. 512 rows, batch / 64 workgroups a step, while the two-halves layout
// of d_in inputs fits LDS, register-resident moments only.
enum { MLPFIT_LAUNCHES, MLPFIT_HALVES, MLPFIT_ONEPASS, MLPFIT_WIDE, MLPFIT_TEAM };
constexpr int MLPFIT_FS = 48, MLPFIT_GMAX = 16;
// the wide trainer's exchange block [2 parities][G][128 units][32 samples]; the larger of it and the team trainer's (mlp_fit_team.h)
constexpr size_t MLPFIT_WIDE_XBYTES = (size_t)2 * MLPFIT_GMAX * 128 * 32 * sizeof(float);
constexpr size_t MLPFIT_XBYTES = MLPFIT_WIDE_XBYTES > MLPFIT_TEAM_XBYTES ? MLPFIT_WIDE_XBYTES : MLPFIT_TEAM_XBYTES;
// the five switches, read per call: launch route for all / for the wide shapes, moments through L2 (so no one-pass and no team trainer), two
// halves for all, launch route for the larger minibatches
struct MlpFitSwitches { bool launches, wide, regmom, onepass, team; };
inline MlpFitSwitches mlp_fit_switches() {
  return {env_flag("MJX_MLP_FIT_LAUNCHES", false), env_flag("MJX_FIT_WIDE", true), env_flag("MJX_FIT_REGMOM", true), env_flag("MJX_FIT_ONEPASS", true),
          env_flag("MJX_FIT_TEAM", true)};
}
struct MlpFitRoute { int kind = MLPFIT_LAUNCHES, nf1 = 0, regmom = 0, G = 0; size_t bytes = 0; int site = SITE_MLP_FIT_LAUNCHES; };
inline MlpFitRoute mlp_fit_route(int d_in, const int* hidden, int n_hidden, int batch, int64_t N, int epochs, const MlpFitSwitches& sw) {
  if (sw.launches || n_hidden != 2 || hidden[0] != 128 || hidden[1] != 128 || N / batch - 1 <= 0 || epochs <= 0) return {};
  const int nf1 = d_in <= 31 ? 1 : 2, G = (d_in + MLPFIT_FS - 1) / MLPFIT_FS;
  if (batch != 64) {
    if (batch % 64 || batch < 128 || batch > 64 * MLPFIT_TEAM_GMAX || d_in > 63 || !sw.regmom || !sw.team) return {};
    const size_t bytes = MlpFitLayout<128>(d_in, nf1 == 2).bytes();
    return bytes <= LDS_MAX ? MlpFitRoute{MLPFIT_TEAM, nf1, 1, batch / 64, bytes, SITE_MLP_FIT_TEAM} : MlpFitRoute{};
  }
  const size_t halves = MlpFitLayout<128>(d_in, nf1 == 2).bytes(), onepass = MlpFit1pLayout<128>(d_in).bytes();
  if (d_in <= 63 && halves <= LDS_MAX) {
    if (d_in <= 23 && sw.regmom && sw.onepass && onepass <= LDS_MAX) return {MLPFIT_ONEPASS, nf1, 1, 1, onepass, SITE_MLP_FIT};
    return {MLPFIT_HALVES, nf1, sw.regmom, 1, halves, SITE_MLP_FIT};
  }
  if (sw.wide && d_in > 48 && G <= MLPFIT_GMAX) return {MLPFIT_WIDE, 2, sw.regmom, G, MlpFitLayout<128>(MLPFIT_FS, true).bytes(), SITE_MLP_FIT_WIDE};
  return {};
}
// the one table of the nine trainer instances, in the order they have in the code object: [REGMOM][NF1 - 1], the one-pass trainer, [REGMOM],
// the team trainer's [NF1 - 1]
typedef void (*MlpFitKernel)(MlpFitArgs);
inline MlpFitKernel mlp_fit_kernel(const MlpFitRoute& r) {
  static const MlpFitKernel halves[2][2] = {{k_mlp_fit<128, 1, false>, k_mlp_fit<128, 2, false>}, {k_mlp_fit<128, 1, true>, k_mlp_fit<128, 2, true>}};
  static const MlpFitKernel onepass = k_mlp_fit1p<128>, wide[2] = {k_mlp_fit<128, 2, false, true>, k_mlp_fit<128, 2, true, true>};
  static const MlpFitKernel team[2] = {k_mlp_fit_team<1>, k_mlp_fit_team<2>};
  return r.kind == MLPFIT_ONEPASS ? onepass : r.kind == MLPFIT_WIDE ? wide[r.regmom] : r.kind == MLPFIT_TEAM ? team[r.nf1 - 1] : halves[r.regmom][r.nf1 - 1];
}
// The exchange block of the WIDE and the TEAM trainer and, behind it, the arrival counter and the give-up word: UNCACHED device memory (stores
// are acknowledged by memory, loads bypass the per-XCD L2s -- the workgroups of one grid sit on different XCDs), allocated once per thread and
// device, never freed.  The 256 counter bytes are cleared on `st`; the block needs no clearing.  One block serves both trainers: the fits a
// thread puts on one stream follow each other (two streams of ONE thread would share it, as they shared each trainer's block: MLPBaseline
// never does that -- one side stream per device).
struct FitExchange { float* xch = nullptr; unsigned* bar = nullptr; };
inline int fit_exchange(hipStream_t st, FitExchange& x) {
  static thread_local PerDevice<char*> block_of;
  char*& block = block_of.here();
  if (!block) HIPCHK(hipExtMallocWithFlags((void**)&block, MLPFIT_XBYTES + 256, hipDeviceMallocUncached));
  HIPCHK(hipMemsetAsync(block + MLPFIT_XBYTES, 0, 256, st));
  x.xch = (float*)block; x.bar = (unsigned*)(block + MLPFIT_XBYTES);
  return MJX_OK;
}
// kinds 1 .. 4: every step of every epoch in ONE launch of the route's trainer; `a` as mlp_fit filled it
inline int mlp_fit_persistent(const MlpFitRoute& r, MlpFitArgs a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  a.G = r.G;
  if (r.G > 1) {                                                // WIDE and TEAM
    FitExchange x;
    if (int rc = fit_exchange(st, x)) return rc;
    a.xch = x.xch; a.bar = x.bar;
  }
  if (r.kind == MLPFIT_WIDE) {
    a.FS = MLPFIT_FS;
    const char* f = getenv("MJX_FIT_FAULT"); a.fault = (f && !strcmp(f, "straggler")) ? 1 : 0;      // (tests/test_gpu_lifecycle.py)
  }
  const MlpFitKernel k = mlp_fit_kernel(r);
  if (int rc = lds_limit((const void*)k, r.bytes)) return rc;
  hipLaunchKernelGGL(k, dim3(r.G), dim3(256), r.bytes, st, a);
  // a barrier wait that timed out (a workgroup without a CU) is recorded in a word of its own; this turns it into NaN epoch
  // losses AFTER every workgroup has left -- the last writer of epoch_loss no longer decides
  if (r.G > 1) hipLaunchKernelGGL(k_mlp_fit_verdict, dim3(1), dim3(64), 0, st, (const unsigned*)a.bar + 1, a.epoch_loss, a.epochs);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}
// kind 0: ~14 launches per step (gather, forward, MSE head, per layer weight gradient / bias gradient / delta, Adam)
inline int mlp_fit_launches(MlpRegressor& net, const MlpFitArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int L = net.nL(), nh = L - 1, bs = a.batch, d_in = a.d_in;
  size_t hsum = 0; for (int i = 0; i < nh; ++i) hsum += net.sizes[i + 1];
  // scratch: Xb, yb, yhat, d_out, acts (bs x h_l), deltas (bs x h_l), grads (P)
  size_t fl = (size_t)bs * d_in + 3 * (size_t)bs + 2 * (size_t)bs * hsum + (size_t)net.P;
  float* q = nullptr;
  if (int rc = dev_scratch(SITE_MLP_FIT_LAUNCHES, stream, fl * sizeof(float), &q)) return rc;
  float* Xb = q; q += (size_t)bs * d_in;
  float* yb = q; q += bs;
  float* yhat = q; q += bs;
  float* dout = q; q += bs;
  std::vector<float*> acts(nh), dl(nh);
  for (int i = 0; i < nh; ++i) { acts[i] = q; q += (size_t)bs * net.sizes[i + 1]; }
  for (int i = 0; i < nh; ++i) { dl[i] = q; q += (size_t)bs * net.sizes[i + 1]; }
  float* grads = q;
  int64_t t = a.step0;
  // the fp32-beta set (vecops.h: ADAM32_*), in 1 - beta and in the corrections too: the arithmetic of the persistent trainers
  // (mlp_fit.h), self-consistent -- the steps stay within 1e-6 lr of torch's, v itself is 1.3e-5 low (tests/test_gpu_fit_matrix.py)
  for (int ep = 0; ep < a.epochs; ++ep) {
    for (int64_t mb = 0; mb < a.steps; ++mb) {
      hipLaunchKernelGGL(k_gather_rows, dim3((bs * d_in + 255) / 256), dim3(256), 0, st, a.feat, a.y, a.perm + (int64_t)ep * a.N + mb * bs, bs, d_in, Xb, yb);
      net.forward(a.params, Xb, bs, acts, yhat, st);
      hipLaunchKernelGGL(k_mse_grad, dim3(1), dim3(256), 0, st, yhat, yb, bs, dout, a.epoch_loss + ep);
      const float* delta = dout;
      for (int l = L - 1; l >= 0; --l) {
        const int ho = net.sizes[l + 1], hi_ = net.sizes[l];
        const float* in = (l == 0) ? Xb : acts[l - 1];
        lw_launch_gemm(gemm_wgrad(bs, ho, hi_, delta, in, hi_, grads + net.oW[l]), 1, st);
        hipLaunchKernelGGL(k_colsum, dim3((ho + 63) / 64, 1), dim3(256), 0, st, delta, (int64_t)bs, ho, (int64_t)ho, grads + net.ob[l]);
        if (l > 0) {
          lw_launch_gemm(gemm_delta(bs, ho, hi_, delta, a.params + net.oW[l], false, dl[l - 1], acts[l - 1], EPI_BACK_RELU), 1, st);
          delta = dl[l - 1];
        }
      }
      const AdamBias bc = adam_bias(ADAM32_B1, ADAM32_B2, ++t);
      hipLaunchKernelGGL(k_adam, dim3((unsigned)((net.P + 255) / 256)), dim3(256), 0, st, a.params, grads, a.m, a.v, net.P, a.lr, a.wd, ADAM32_C1, ADAM32_B2, ADAM32_C2, ADAM_EPS, bc.bc1, bc.bc2s);
    }
  }
  HIPCHK(lw_status());
  return MJX_OK;
}
// mjx_mlp_fit_adam behind its argument check: the epoch losses cleared, the arguments every route takes, the route
inline int mlp_fit(const float* feat, const float* y, int64_t N, int d_in, const int* hidden, int n_hidden, float* params, float* m, float* v,
                   int64_t step0, const int32_t* perm, int epochs, int batch, float lr, float wd, double* epoch_loss_out, void* stream) {
  HIPCHK(hipMemsetAsync(epoch_loss_out, 0, sizeof(double) * (epochs > 0 ? epochs : 1), (hipStream_t)stream));
  MlpRegressor net; net.init(d_in, hidden, n_hidden);
  const MlpFitRoute r = mlp_fit_route(d_in, hidden, n_hidden, batch, N, epochs, mlp_fit_switches());
  MlpFitArgs a{};
  a.feat = feat; a.y = y; a.perm = perm; a.N = N; a.d_in = d_in; a.epochs = epochs;
  a.steps = N / batch - 1;                            // optimize_model.py:24
  a.params = params; a.m = m; a.v = v; a.step0 = step0; a.lr = lr; a.wd = wd; a.epoch_loss = epoch_loss_out; a.batch = batch;
  if (r.kind == MLPFIT_LAUNCHES) return mlp_fit_launches(net, a, stream);
  if (int rc = dev_scratch((ScratchSite)r.site, stream, (size_t)r.G * net.P * 2 * sizeof(float), &a.mv)) return rc;
  return mlp_fit_persistent(r, a, stream);
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
// the per-step route of both policy entries: gather, forward, loss head, backward and k_adam as launches of their own (`w`: the context's
// workspace; trn / tro: the transforms, never null)
inline int policy_fit_launches(int n, int m, int oS, int64_t d, MinibatchWS& w, int loss, const float* obs, const float* act, const float* adv,
                               const int32_t* idx, int64_t steps, int B, float* theta, const float* trn, const float* theta_old, const float* tro,
                               int old_tracks_new, float* adam_m, float* adam_v, int64_t step0, float lr, float clip, double* loss_trace,
                               hipStream_t st) {
  if (int rc = w.reserve(B)) return fail(rc, "minibatch workspace allocation failed");
  const int64_t cnt = (loss == 0) ? (int64_t)oS : d;             // MSE: log_std has no gradient -> untouched (like torch's grad None)
  const unsigned ggrid = capped_grid(B * (n > m ? n : m), 256, 1024);
  for (int64_t s = 0; s < steps; ++s) {
    const bool old_fwd = (loss == 2) && !old_tracks_new;
    if (int rc = w.grad_step(loss, obs, act, adv, idx + s * B, B, theta, trn, theta_old, tro, old_fwd, clip,
                             loss_trace ? loss_trace + s : (double*)nullptr, ggrid, st))
      return fail(MJX_ERR_STATE, "minibatch backward failed (%d)", rc);
    const AdamBias bc = adam_bias(ADAM_B1D, ADAM_B2D, step0 + s + 1);      // torch's constants, as k_policy_fit takes them (vecops.h)
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, theta, w.grad.p, adam_m, adam_v, cnt, lr, 0.f,
                       ADAM_C1, ADAM_B2, ADAM_C2, ADAM_EPS, bc.bc1, bc.bc2s);
  }
  HIPCHK(lw_status());
  return MJX_OK;
}
// mjx_policy_minibatch_adam behind its argument check, on the context's device: (n, m, hidden, ident_tr, oS, d) are the context's shape,
// its identity transform (for a null tr / tr_old), the offset of log_std and the parameter count; `w` is its launch route's workspace
inline int policy_fit(int n, int m, const std::vector<int>& hidden, const float* ident_tr, int oS, int64_t d, MinibatchWS& w, int loss,
                      const float* obs, const float* act, const float* adv, const int32_t* idx, int64_t steps, int B, float* theta,
                      const float* tr, const float* theta_old, const float* tr_old, int old_tracks_new, float* adam_m, float* adam_v,
                      int64_t step0, float lr, float clip, double* loss_trace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const float* trn = tr ? tr : ident_tr;
  const float* tro = tr_old ? tr_old : ident_tr;
  const PolicyFitRoute r = policy_fit_route(n, m, hidden, B, loss, old_tracks_new, env_flag("MJX_NO_POLICY_FIT", false));   // (read per call)
  if (r.H) {
    PolicyFitArgs a{obs, act, adv, idx, steps, B, n, m, theta, theta_old, trn, tro, loss, old_tracks_new, adam_m, adam_v,
                    step0, lr, clip, loss_trace, (int)(r.bytes / 4)};
    void (*k)(PolicyFitArgs) = (r.H == 64) ? k_policy_fit<64> : k_policy_fit<32>;
    if (int rc = lds_limit((const void*)k, r.bytes)) return rc;
    hipLaunchKernelGGL(k, dim3(1), dim3(PFIT_THREADS), r.bytes, st, a);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  return policy_fit_launches(n, m, oS, d, w, loss, obs, act, adv, idx, steps, B, theta, trn, theta_old, tro, old_tracks_new, adam_m, adam_v, step0, lr,
                             clip, loss_trace, st);
}

// ---- ... for the manipulation-sized policies (policy_fit_wide.h): H = 64 or 32 twice, up to 64 observations and 32 actions, the same
// minibatches; plain arithmetic over the kernel's own layout, H = 0: it does not serve (`off`: MJX_POLICY_FIT_WIDE=0 or MJX_NO_POLICY_FIT=1)
inline PolicyFitRoute policy_fit_wide_route(int n, int m, const std::vector<int>& hidden, int B, int loss, int old_tracks_new, bool off) {
  if (off || hidden.size() != 2 || hidden[0] != hidden[1] || (hidden[0] != 64 && hidden[0] != 32) || B % 4 || B < 8 || B > 64 || n < 1 ||
      n > 64 || m < 1 || m > 32)
    return {};
  const int H = hidden[0]; const bool old_net = loss == 2 && !old_tracks_new;
  const size_t bytes = 4 * (H == 64 ? PolicyFitWideLayout<64>(n, m).lds_floats(B, old_net) : PolicyFitWideLayout<32>(n, m).lds_floats(B, old_net));
  return bytes <= LDS_MAX ? PolicyFitRoute{H, bytes} : PolicyFitRoute{};
}
// The ladder of mjx_policy_minibatch_adam_wide as arithmetic: 1 = k_policy_fit where policy_fit_route serves (the measured kernel for its
// shapes), 2 = k_policy_fit_wide, 0 = per-step launches; `r`: H and bytes of route 1 or 2.  Both switches are read per call.
inline int policy_fit_ladder(int n, int m, const std::vector<int>& hidden, int B, int loss, int old_tracks_new, int from, PolicyFitRoute& r) {
  const bool no_fit = env_flag("MJX_NO_POLICY_FIT", false), wide_off = !env_flag("MJX_POLICY_FIT_WIDE", true);
  if (from <= 1 && (r = policy_fit_route(n, m, hidden, B, loss, old_tracks_new, no_fit)).H) return 1;
  if (from <= 2 && (r = policy_fit_wide_route(n, m, hidden, B, loss, old_tracks_new, no_fit || wide_off)).H) return 2;
  r = PolicyFitRoute{};
  return 0;
}
// mjx_policy_minibatch_adam_wide behind its argument check (parameters as policy_fit's): the ladder, where a route whose LDS request the
// device refuses falls through to the next (launch_chained, model_host.h); the route that ran goes to route_out
inline int policy_fit_wide(int n, int m, const std::vector<int>& hidden, const float* ident_tr, int oS, int64_t d, MinibatchWS& w, int loss,
                           const float* obs, const float* act, const float* adv, const int32_t* idx, int64_t steps, int B, float* theta,
                           const float* tr, const float* theta_old, const float* tr_old, int old_tracks_new, float* adam_m, float* adam_v,
                           int64_t step0, float lr, float clip, double* loss_trace, void* stream, int* route_out) {
  hipStream_t st = (hipStream_t)stream;
  const float* trn = tr ? tr : ident_tr;
  const float* tro = tr_old ? tr_old : ident_tr;
  PolicyFitRoute r;
  for (int from = 1; from <= 2; ++from) {
    const int route = policy_fit_ladder(n, m, hidden, B, loss, old_tracks_new, from, r);
    if (route == 0) break;
    const PolicyFitArgs a{obs, act, adv, idx, steps, B, n, m, theta, theta_old, trn, tro, loss, old_tracks_new, adam_m, adam_v,
                          step0, lr, clip, loss_trace, (int)(r.bytes / 4)};
    void (*k)(PolicyFitArgs) = route == 1 ? (r.H == 64 ? k_policy_fit<64> : k_policy_fit<32>) : (r.H == 64 ? k_policy_fit_wide<64> : k_policy_fit_wide<32>);
    bool launched = false;
    if (int rc = launch_chained(k, r.bytes, dim3(1), a, st, launched, dim3(PFIT_THREADS))) return rc;
    if (launched) { if (route_out) *route_out = route; return MJX_OK; }
    from = route;                                                // (refused: the next rung)
  }
  if (route_out) *route_out = 0;
  return policy_fit_launches(n, m, oS, d, w, loss, obs, act, adv, idx, steps, B, theta, trn, theta_old, tro, old_tracks_new, adam_m, adam_v, step0, lr,
                             clip, loss_trace, st);
}

// ---- dynamics fit of one member (dynamics.h) behind mjx_dyn_fit_adam's argument check, steps > 0: prep, then k_dyn_fit, the persistent
// trainer, where dyn_fit_shape / dyn_fit_persistent (model_host.h) allow, else launches per step
inline int dyn_fit_impl(const DynNet& net, const float* x, const float* y, int64_t N, const float* in_tr, const float* out_tr, int target_mode,
                        int act, float* params, float* m, float* v, int64_t step0, const int32_t* idx, int64_t steps, int batch, float lr,
                        float wd, float* loss_out, void* stream) {
  const int din = net.din(), dout = net.dout();
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  // scratch: normalised inputs + targets (prep), then the launch route's minibatch activations and deltas
  int wmax = 0; size_t hsum = 0;
  for (int l = 1; l <= net.nl; ++l) { wmax = net.sz[l] > wmax ? net.sz[l] : wmax; hsum += net.sz[l]; }
  const size_t prep = (size_t)N * (din + dout), mb = (size_t)batch * (din + dout + hsum + 2 * (size_t)wmax);
  float* xn = nullptr;
  if (int rc = dev_scratch(SITE_DYN_FIT, stream, (prep + mb) * sizeof(float), &xn)) return rc;
  float* tg = xn + (size_t)N * din;
  launch_dyn_prep(x, y, N, din, dout, in_tr, out_tr, target_mode, xn, tg, st);
  const float* oaff = target_mode == DYN_TGT_AFFINE ? out_tr : nullptr;
  const size_t fbytes = dyn_fit_lds_bytes(net, batch);
  if (dyn_fit_shape(net, batch, env_flag("MJX_DYN_FIT_LAUNCHES", false)) && dyn_fit_persistent(fbytes, static_lds((const void*)k_dyn_fit))) {
    if (int rc = lds_limit((const void*)k_dyn_fit, fbytes)) return rc;
    DynFitArgs a{net, xn, tg, idx, steps, batch, params, m, v, step0, lr, wd, act, oaff, loss_out};
    hipLaunchKernelGGL(k_dyn_fit, dim3(1), dim3(1024), fbytes, st, a);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  float* q = tg + (size_t)N * dout;
  std::vector<float*> A(net.nl + 1);
  for (int l = 0; l <= net.nl; ++l) { A[l] = q; q += (size_t)batch * net.sz[l]; }
  float* T = q; q += (size_t)batch * dout;
  float* D[2] = {q, q + (size_t)batch * wmax};
  auto blocks = [](int64_t e) { return dim3(capped_grid(e, 256, 2048)); };
  for (int64_t s = 0; s < steps; ++s) {
    hipLaunchKernelGGL(k_dl_gather, blocks((int64_t)batch * (din + dout)), dim3(256), 0, st, xn, tg, idx + s * batch, batch, din, dout, A[0], T);
    for (int l = 0; l < net.nl; ++l)
      hipLaunchKernelGGL(k_dl_fwd, blocks((int64_t)batch * net.sz[l + 1]), dim3(256), 0, st, A[l], batch, net.sz[l], params + net.oW[l],
                         params + net.ob[l], net.sz[l + 1], A[l + 1], l + 1 < net.nl ? act : -1);
    hipLaunchKernelGGL(k_dl_loss, dim3(1), dim3(1024), 0, st, A[net.nl], T, batch, dout, oaff, D[0], loss_out + s);
    int cur = 0;
    for (int l = net.nl - 1; l >= 0; --l) {
      const int di = net.sz[l], dj = net.sz[l + 1];
      if (l > 0)
        hipLaunchKernelGGL(k_dl_bwd, blocks((int64_t)batch * di), dim3(256), 0, st, D[cur], batch, di, params + net.oW[l], dj, A[l], act, D[cur ^ 1]);
      hipLaunchKernelGGL(k_dl_adam, blocks((int64_t)di * dj + dj), dim3(256), 0, st, D[cur], A[l], batch, di, dj, params, m, v, net.oW[l],
                         step0 + s + 1, lr, wd);
      cur ^= 1;
    }
  }
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

// ---- the fit of a whole ensemble (dyn_fit_ens.h, dyn_fit_ens_team.h).  What mjx_dyn_fit_ensemble, mjx_dyn_fit_ensemble_team and
// mjx_reward_fit_ensemble receive, after dyn_net has parsed the sizes: each entry fills one record, and everything below takes it
struct DfeCall {
  const float* x; int64_t x_stride; const float* y; int64_t y_stride; int64_t N; int K;
  DynNet net;
  const float* in_tr; const float* out_tr; int target_mode, act;
  float* params; float* m; float* v; const int64_t* step0;
  const int32_t* idx; int64_t steps; int batch; float lr, wd;
  float* loss_out; void* stream;
};
// what routes 1 and 2 share ahead of their launches: the scratch -- per member the normalised inputs and targets (every member has its own
// transforms) and, behind them, `xtiles` floats for the X tiles where the caller's LDS has no room --, the per-member prep, the kernel's arguments
inline int dfe_prepare(const DfeCall& c, size_t xtiles, DynFitEnsArgs& a) {
  const int din = c.net.din(), dout = c.net.dout();
  const size_t rows = (size_t)c.K * (size_t)c.N * (din + dout);
  float* scr = nullptr;
  if (int rc = dev_scratch(SITE_DYN_FIT_ENS, c.stream, (rows + (xtiles ? 4 + xtiles : 0)) * sizeof(float), &scr)) return rc;
  float* xn = scr; float* tg = xn + (size_t)c.K * c.N * din;
  for (int k = 0; k < c.K; ++k)
    launch_dyn_prep(c.x + k * c.x_stride, c.y + k * c.y_stride, c.N, din, dout, c.in_tr + (int64_t)k * 2 * din, c.out_tr + (int64_t)k * 2 * dout,
                    c.target_mode, xn + (size_t)k * c.N * din, tg + (size_t)k * c.N * dout, (hipStream_t)c.stream);
  a = DynFitEnsArgs{};
  a.din = din; a.h1 = c.net.sz[1]; a.h2 = c.net.sz[2]; a.dout = dout; a.B = c.batch; a.act = c.act;
  a.P = c.net.P; a.N = c.N; a.steps = c.steps; a.xn = xn; a.tg = tg; a.idx = c.idx; a.W = c.params; a.m = c.m; a.v = c.v; a.loss = c.loss_out;
  a.xscr = xtiles ? scr + ((rows + 3) & ~(size_t)3) : nullptr;
  a.lr = c.lr; a.wd = c.wd;
  return MJX_OK;
}
// the launches of a trainer over the members, `chunk` at a time (at most DFE_CHUNK: their step counts travel as kernel arguments), `wgs`
// workgroups a member; `a` is the DynFitEnsArgs inside `args`
template <class Args>
inline void dfe_launch_chunks(void (*kern)(Args), Args& args, DynFitEnsArgs& a, const DfeCall& c, int chunk, int wgs, size_t lds) {
  for (int k0 = 0; k0 < c.K; k0 += chunk) {
    const int kn = c.K - k0 < chunk ? c.K - k0 : chunk;
    a.k0 = k0;
    for (int q = 0; q < kn; ++q) a.step0[q] = c.step0[k0 + q];
    hipLaunchKernelGGL(kern, dim3((unsigned)(kn * wgs)), dim3(DFE_THREADS), lds, (hipStream_t)c.stream, args);
  }
}
// Route 1 of both ensemble entries: one k_dyn_fit_ens<RAG> launch per DFE_CHUNK members (one launch for K <= DFE_CHUNK)
template <bool RAG>
inline int dfe_run(const DfeCall& c) {
  MJX_DEVICE_ENTRY();
  const DfeLayout L(c.net, c.batch);
  DynFitEnsArgs a;
  if (int rc = dfe_prepare(c, L.x_in_lds ? 0 : (size_t)c.K * L.xtile, a)) return rc;
  if (int rc = lds_limit((const void*)k_dyn_fit_ens<RAG>, L.lds_bytes())) return rc;
  a.otr = RAG ? c.out_tr : nullptr;
  dfe_launch_chunks(k_dyn_fit_ens<RAG>, a, a, c, DFE_CHUNK, 1, L.lds_bytes());
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

// ---- ... with a team of G workgroups per member (dyn_fit_ens_team.h).  Route 2 of mjx_dyn_fit_ensemble_team.
// Its exchange block and, behind it, the members' [arrival counter, give-up word] pairs: uncached device memory as fit_exchange's, per thread
// and device.  The fits a thread puts on one stream follow each other, so one block serves them all; a call that needs more than the block
// holds gets a new one of at least twice the size and the old one STAYS (uncached memory a kernel has read is never freed): all blocks of a
// thread and device together stay under twice the largest call's need.
inline int fit_exchange_sized(size_t xbytes, size_t bar_bytes, FitExchange& x) {
  struct Block { char* p = nullptr; size_t xcap = 0, bcap = 0; };
  static thread_local PerDevice<Block> block_of;
  Block& b = block_of.here();
  if (!b.p || b.xcap < xbytes || b.bcap < bar_bytes) {
    auto grown = [](size_t need, size_t cap) { need = (need + 255) & ~(size_t)255; return need <= cap ? cap : need > 2 * cap ? need : 2 * cap; };
    const size_t xcap = grown(xbytes, b.xcap), bcap = grown(bar_bytes, b.bcap);
    char* p = nullptr;
    HIPCHK(hipExtMallocWithFlags((void**)&p, xcap + bcap, hipDeviceMallocUncached));
    b.p = p; b.xcap = xcap; b.bcap = bcap;
  }
  x.xch = (float*)b.p; x.bar = (unsigned*)(b.p + b.xcap);
  return MJX_OK;
}
// dfe_run's prep, then per launch at most floor(CUs / G) teams, each workgroup with LDS that leaves no room for a second one on its CU --
// every team of a launch is co-resident on an idle device; the give-up path covers a busy one -- and behind the launches the verdict.  The
// caller has asked dfe_team_serves.
inline int dfe_team_run(const DfeCall& c) {
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)c.stream;
  const DfeTeamLayout L(c.net, c.batch);
  const int cap = cu_count() / L.G, chunk = cap < DFE_CHUNK ? cap : DFE_CHUNK;
  if (chunk < 1) return fail(MJX_ERR_UNSUPPORTED, "a team of %d workgroups needs %d CUs", L.G, L.G);
  DynFitTeamArgs t{};
  if (int rc = dfe_prepare(c, 0, t.e)) return rc;
  FitExchange ex;
  if (int rc = fit_exchange_sized((size_t)(c.K < chunk ? c.K : chunk) * L.slot * sizeof(float), (size_t)c.K * 2 * sizeof(unsigned), ex)) return rc;
  hipLaunchKernelGGL(k_dfe_team_clear, dim3(capped_grid(2 * (int64_t)c.K, 256, 64)), dim3(256), 0, st, ex.bar, 2 * (int64_t)c.K);
  if (int rc = lds_limit((const void*)k_dyn_fit_ens_team, L.lds_bytes())) return rc;
  t.G = L.G; t.xch = ex.xch; t.bar = ex.bar; t.xslot = (int64_t)L.slot;
  dfe_launch_chunks(k_dyn_fit_ens_team, t, t.e, c, chunk, L.G, L.lds_bytes());
  hipLaunchKernelGGL(k_dfe_team_verdict, dim3((unsigned)c.K), dim3(64), 0, st, (const unsigned*)ex.bar, c.loss_out, c.steps);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

// what both ensemble entries and the team entry ask of their arguments, after the sizes are parsed
inline bool dfe_args_ok(const DfeCall& c) {
  if (!c.x || !c.y || !c.in_tr || !c.out_tr || !c.params || !c.m || !c.v || !c.step0 || (c.steps > 0 && (!c.idx || !c.loss_out)) || c.N <= 0 ||
      c.x_stride < 0 || c.y_stride < 0 || c.batch <= 0 || c.batch > c.N || c.steps < 0 || !dyn_args_ok(c.net, c.K, c.act, c.target_mode))
    return false;
  for (int k = 0; k < c.K; ++k) if (c.step0[k] < 0) return false;
  return true;
}
// the body of both ensemble entries, after the sizes are parsed: the argument check, the route (the entry's switch, read per call -- the
// tests and tools/bench_dyn_fit.py compare the two routes in one process -- and what its shape predicate answered) written to route_out,
// then route 0, member by member on the routes of dyn_fit_impl (the check above covers every member's), or route 1, dfe_run<RAG>
template <bool RAG>
inline int dfe_entry(const DfeCall& c, const char* switch_name, bool shape_served, int* route_out) {
  const int din = c.net.din(), dout = c.net.dout();
  if (!dfe_args_ok(c)) return fail(MJX_ERR_ARG, "bad arguments");
  const int route = env_flag(switch_name, true) && shape_served ? 1 : 0;
  if (route_out) *route_out = route;
  if (c.steps == 0) return MJX_OK;
  if (route == 0) {
    for (int k = 0; k < c.K; ++k)
      if (int rc = dyn_fit_impl(c.net, c.x + k * c.x_stride, c.y + k * c.y_stride, c.N, c.in_tr + (int64_t)k * 2 * din, c.out_tr + (int64_t)k * 2 * dout,
                                c.target_mode, c.act, c.params + k * c.net.P, c.m + k * c.net.P, c.v + k * c.net.P, c.step0[k],
                                c.idx + (int64_t)k * c.steps * c.batch, c.steps, c.batch, c.lr, c.wd, c.loss_out + (int64_t)k * c.steps, c.stream))
        return rc;
    return MJX_OK;
  }
  return dfe_run<RAG>(c);
}

}  // namespace mjx
