// mjx.hip -- C ABI (include/mjx.h) over the gfx950 kernels.  Host side only orchestrates:
// it owns the workspace, picks the kernel instance and enqueues launches on the caller's
// stream.  No host<->device synchronisation happens here unless an entry point says so.
#include "../../include/mjx.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <pthread.h>
#include <unistd.h>
#include <atomic>
#include <string>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "baseline.h"
#include "dynamics.h"
#include "dyn_fit_ens.h"
#include "fused_policy.h"
#include "policy_fit.h"
#include "rccl_dyn.h"
#include "launch_state.h"
#include "layerwise.h"
#include "mlp_fit.h"
#include "path_reward.h"
#include "plan.h"
#include "plan_wide.h"
#include "policy_rollout.h"
#include "policy_rollout_wide.h"
#include "rollout_batch.h"
#include "rows_wide.h"
#include "vecops.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) return fail((int)e_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// launch_state.h's answers as entry results: the dynamic-LDS limit of `kern` on the current device before a launch with `bytes`,
// and a scratch block of the calling thread on (site, current device, stream)
int lds_limit(const void* kern, size_t bytes) {
  const int e = mjx::dyn_lds(kern, bytes);
  if (e == mjx::LDS_OVER) return fail(MJX_ERR_UNSUPPORTED, "needs %zu + %zu static bytes of LDS (> 160 KiB)", bytes, mjx::static_lds(kern));
  if (e) return fail(e, "dynamic LDS limit of %zu bytes: %s", bytes, hipGetErrorString((hipError_t)e));
  return MJX_OK;
}
enum ScratchSite { SITE_GRAM, SITE_MLP_PREDICT, SITE_MLP_FIT, SITE_MLP_FIT_WIDE, SITE_MLP_FIT_LAUNCHES, SITE_DYN_FIT, SITE_SUM_STATS, SITE_PLAN_ROLLOUT, SITE_PLAN_SCORE, SITE_DYN_FIT_ENS, SITE_PATH_REWARDS, SITE_POLICY_ROLLOUT, SITE_ROLLOUT_DISAGREE };
template <class T>
int dev_scratch(ScratchSite site, void* stream, size_t bytes, T** out) {
  HIPCHK(mjx::scratch(site, (hipStream_t)stream, bytes, (void**)out));
  return MJX_OK;
}
// blocks of `per` elements that cover `elems` > 0, at most `cap` (grid-stride kernels)
unsigned capped_grid(int64_t elems, int per, int cap) { const int64_t g = (elems + per - 1) / per; return (unsigned)(g < cap ? g : cap); }

// ---- fork guard.  Sampler workers are FORKED from the training process (mjrl/samplers/core.py:189-210: mp.Pool under a parent
// that holds an mjx_ctx, page-locked staging blocks and libmjx's gather threads).  None of that survives a fork in a usable
// state, so a forked child of a process that touched the device through this library may not touch it again: every entry that
// creates device state refuses there, loudly, instead of hanging inside the HIP runtime.  mjx_process_state() lets a test (or
// a worker) prove that it never tried.
std::atomic<long long> g_device_calls{0};     // entries that reach the HIP runtime, made by THIS process (zeroed in a forked child)
std::atomic<int> g_forked_child{0};           // 1: this process was forked from one whose g_device_calls was > 0
void atfork_child() {
  if (g_device_calls.load() > 0) g_forked_child.store(1);
  g_device_calls.store(0);
}
struct ForkGuardInit { ForkGuardInit() { pthread_atfork(nullptr, nullptr, atfork_child); } } g_fork_guard_init;

#define MJX_DEVICE_ENTRY()                                                                                                          \
  do {                                                                                                                              \
    if (g_forked_child.load())                                                                                                      \
      return fail(MJX_ERR_STATE, "libmjx: this process was forked from one that holds HIP state; device work belongs to the "      \
                                 "training process (sampler workers stay on the host, mjrl/samplers/core.py)");                     \
    g_device_calls.fetch_add(1);                                                                                                    \
  } while (0)

}  // namespace

#include "fused_host.h"
#include "model_host.h"
#include "fit_host.h"
#include "update_host.h"     // (defines mjx_ctx)

namespace {

using namespace mjx;

const float* tr_new_or_ident(const mjx_ctx* c) { return c->tr_new ? c->tr_new : c->ident_tr; }
const float* tr_old_or_ident(const mjx_ctx* c) { return c->tr_old ? c->tr_old : c->ident_tr; }

// the bound inputs as the fused kernels take them; FusedWS adds its own part (fused_host.h complete())
FusedArgs bound_args(const mjx_ctx* c, const float* thetaB) {
  FusedArgs a{};
  a.obs = c->obs; a.act = c->act; a.adv = c->adv; a.N = c->N_local;
  a.inv_N = (float)(1.0 / (double)c->N_global);
  a.thetaA = c->theta_new; a.thetaB = thetaB; a.trA = tr_new_or_ident(c); a.trB = tr_old_or_ident(c);
  a.old_is_new = c->old_is_new;
  a.dbg = c->dbg; a.clk = c->clk;
  a.n = c->n; a.m = c->m;
  return a;
}

int check_bound(mjx_ctx* c, bool need_act) {
  if (!c) return fail(MJX_ERR_ARG, "null context");
  if (!c->batch_bound || c->N_local < 0 || c->N_global <= 0) return fail(MJX_ERR_STATE, "mjx_bind_batch has not been called");
  if (need_act && c->N_local > 0 && (!c->act || !c->adv)) return fail(MJX_ERR_STATE, "actions / advantages not bound");
  if (!c->theta_new || !c->theta_old) return fail(MJX_ERR_STATE, "mjx_bind_policy has not been called");
  return MJX_OK;
}

}  // namespace

extern "C" {

const char* mjx_last_error(void) { return g_err.c_str(); }
int mjx_version(void) { return 1; }

int mjx_process_state(int64_t* out2) {
  if (!out2) return fail(MJX_ERR_ARG, "null output");
  out2[0] = (int64_t)g_device_calls.load();
  out2[1] = (int64_t)g_forked_child.load();
  return MJX_OK;
}

int mjx_device_count(void) {
  if (g_forked_child.load()) return 0;            // (never fails: a forked child simply sees no device through this library)
  g_device_calls.fetch_add(1);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

int mjx_create(mjx_ctx** out, int device, int n, int m, const int* hidden, int n_hidden) {
  if (!out || n <= 0 || m <= 0 || n_hidden < 0 || (n_hidden > 0 && !hidden)) return fail(MJX_ERR_ARG, "bad arguments");
  MJX_DEVICE_ENTRY();
  if (mjx_device_count() <= device) return fail(MJX_ERR_NOGPU, "HIP device %d not available", device);
  HIPCHK(hipSetDevice(device));
  struct Guard { mjx_ctx* c; ~Guard() { mjx_destroy(c); } } built{new mjx_ctx()};     // any failure below takes back what was built so far
  mjx_ctx* c = built.c;
  c->device = device; c->n = n; c->m = m;
  c->hidden.assign(hidden, hidden + n_hidden);
  int prev = n; int64_t d = 0;
  for (int h : c->hidden) { if (h <= 0) return fail(MJX_ERR_ARG, "bad hidden size"); d += (int64_t)prev * h + h; prev = h; }
  d += (int64_t)prev * m + m;
  c->oS = (int)d;
  d += m;
  c->d = d;
  if (int rc = c->fz.init(n, m, d, c->oS, c->hidden, cu_count(), env_flag("MJX_FORCE_LAYERWISE", false))) return rc;
  if (int rc = c->cg.alloc(d)) return rc;
  c->tp.init(device, d, c->cg.ticket);
  std::vector<float> id(tr_len(n, m), 0.f);
  for (int i = 0; i < n; ++i) id[n + i] = 1.f;
  for (int i = 0; i < m; ++i) id[2 * n + m + i] = 1.f;
  HIPCHK(hipMalloc(&c->ident_tr, id.size() * 4));
  HIPCHK(hipMemcpy(c->ident_tr, id.data(), id.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(c->fz.spartials, 0, c->fz.spartials_bytes()));
  c->lw.init(n, m, c->hidden);
  c->lwmb.lw.init(n, m, c->hidden);
  built.c = nullptr;
  *out = c;
  return MJX_OK;
}

// (a half-built context too: every owner releases what it has, null pointers included)
void mjx_destroy(mjx_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->tp.detach();
  c->lw.release();
  c->lwmb.release();
  c->prof.release();
  c->fz.release();
  hipFree(c->ident_tr);
  c->cg.release();
  delete c;
}

int64_t mjx_num_params(const mjx_ctx* c) { return c ? c->d : -1; }
int mjx_uses_fused_path(const mjx_ctx* c) { return c ? (c->fz.variant != 0) : 0; }
int mjx_fused_info(const mjx_ctx* c, int32_t* out) {
  if (!c || !out) return fail(MJX_ERR_ARG, "bad arguments");
  c->fz.info(out);
  return MJX_OK;
}
int mjx_fused_route(int n, int m, const int* hidden, int n_hidden, int32_t* out4) {
  if (!out4 || n <= 0 || m <= 0 || n_hidden < 0 || (n_hidden > 0 && !hidden)) return fail(MJX_ERR_ARG, "bad arguments");
  for (int i = 0; i < n_hidden; ++i) if (hidden[i] <= 0) return fail(MJX_ERR_ARG, "bad hidden size");
  const FusedRoute r = fused_route(n, m, std::vector<int>(hidden, hidden + n_hidden));
  out4[0] = r.variant; out4[1] = r.npc; out4[2] = r.raw_dr; out4[3] = (int32_t)r.bytes;
  return MJX_OK;
}

int mjx_malloc(void** p, int64_t bytes) {
  MJX_DEVICE_ENTRY();
  if (!p || bytes < 0) return fail(MJX_ERR_ARG, "bad arguments");
  HIPCHK(hipMalloc(p, (size_t)bytes + 16));      // + one 16-byte granule: the tail reads of mjx_bind_batch's observation block stay inside
  return MJX_OK;
}
int mjx_free(void* p) { HIPCHK(hipFree(p)); return MJX_OK; }
int mjx_memcpy_h2d(void* dst, const void* src, int64_t bytes, void* stream) {
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream)); return MJX_OK; }
int mjx_memcpy_d2h(void* dst, const void* src, int64_t bytes, void* stream) {
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream)); return MJX_OK; }
int mjx_stream_sync(void* stream) { HIPCHK(hipStreamSynchronize((hipStream_t)stream)); return MJX_OK; }

int mjx_bind_batch(mjx_ctx* c, const float* obs, const float* act, const float* adv, int64_t N_local, int64_t N_global) {
  if (!c || (!obs && N_local > 0) || N_local < 0 || N_global < N_local || N_global <= 0) return fail(MJX_ERR_ARG, "bad batch");
  if (((uintptr_t)obs & 15) != 0) return fail(MJX_ERR_ARG, "obs must be 16-byte aligned");
  c->obs = obs; c->act = act; c->adv = adv; c->N_local = N_local; c->N_global = N_global;
  c->batch_bound = true;
  c->rows_bound = N_local;
  c->fz.on_batch();                             // a new batch: nothing cached from earlier calls applies
  c->lw.invalidate();
  c->lw_old_ok = false;
  if (!c->fz.variant) {
    // the layer-wise launches put one 128-row tile per grid row: gridDim.y <= 65 535 -> 8 388 480 rows per context (BASELINE
    // configs[4] at its full 8M + demonstrations fits; beyond that, shard the batch -- element and byte offsets are 64-bit throughout)
    if (N_local > (int64_t)65535 * 128) return fail(MJX_ERR_ARG, "layer-wise path: at most %lld rows per context (got %lld): bind the batch in shards", (long long)65535 * 128, (long long)N_local);
    int rc = c->lw.reserve(N_local); if (rc) return fail(rc, "layer-wise workspace allocation failed");
  }
  return MJX_OK;
}

int mjx_bind_rows(mjx_ctx* c, int64_t N_local, int64_t N_global, const float* adv) {
  if (!c || !c->batch_bound) return fail(MJX_ERR_STATE, "mjx_bind_batch has not been called");
  if (N_local < 0 || N_local > c->rows_bound || N_global < N_local || N_global <= 0) return fail(MJX_ERR_ARG, "bad row count");
  c->N_local = N_local; c->N_global = N_global;
  if (adv) c->adv = adv;
  c->lw.narrow(N_local);                        // (a prefix of the bound rows keeps the activations cached for it -- DAPG's on-policy prefix;
                                                //  the fused caches are valid for any prefix of the rows they were filled for)
  return MJX_OK;
}

}  // extern "C"
namespace {
// keep_old_outputs: the one-call updates re-bind (stepped parameters, the SAME old parameters) between their K1 and their
// evaluations -- the old policy's cached outputs stay usable; a caller's own binding may come with new contents under the same pointers
int bind_policy_impl(mjx_ctx* c, const float* theta_new, const float* theta_old, const float* tr_new, const float* tr_old, int old_is_new,
                     bool keep_old_outputs) {
  if (!c || !theta_new || !theta_old) return fail(MJX_ERR_ARG, "bad policy");
  if (c && !(keep_old_outputs && theta_old == c->theta_old && tr_old == c->tr_old && tr_new == c->tr_new)) c->lw_old_ok = false;
  if ((((uintptr_t)theta_new) | ((uintptr_t)theta_old)) & 15) return fail(MJX_ERR_ARG, "parameter vectors must be 16-byte aligned");
  c->theta_new = theta_new; c->theta_old = theta_old; c->tr_new = tr_new; c->tr_old = tr_old;
  c->old_is_new = old_is_new ? 1 : 0;
  c->lw.invalidate();
  c->fz.on_policy();
  return MJX_OK;
}
}  // namespace
extern "C" {

int mjx_bind_policy(mjx_ctx* c, const float* theta_new, const float* theta_old, const float* tr_new, const float* tr_old, int old_is_new) {
  return bind_policy_impl(c, theta_new, theta_old, tr_new, tr_old, old_is_new, false);
}

// ---------------------------------------------------------------------------- K6 baselines (host side: csrc/fit_host.h)
int mjx_bl_num_features(int kind, int n) { return (kind < 0 || kind > 2 || n <= 0) ? -1 : bl_num_features(kind, n); }

int mjx_bl_features_f32(const double* obs, const int32_t* tpos, int64_t N, int n, float* out, void* stream) {
  if (!obs || !tpos || !out || N < 0 || n <= 0) return fail(MJX_ERR_ARG, "bad arguments");
  if (N == 0) return MJX_OK;
  hipLaunchKernelGGL(k_bl_features_f32, dim3(ew_grid(N * (n + 4))), dim3(256), 0, (hipStream_t)stream, obs, tpos, N, n, out);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_bl_gram_route(int kind, int n, int64_t N, int32_t* out6) {
  if (!out6 || kind < 0 || kind > 2 || n <= 0 || n > 4096 || N <= 0) return fail(MJX_ERR_ARG, "bad arguments");     // (get_feat_table's limits)
  const GramRoute r = gram_route(bl_num_features(kind, n), n, N, env_flag("MJX_GRAM_FMA", false));
  out6[0] = r.arm; out6[1] = r.Z; out6[2] = r.nblk; out6[3] = r.gx; out6[4] = r.blk; out6[5] = (int32_t)r.lds;
  return MJX_OK;
}

int mjx_bl_gram(int kind, const double* obs, const int32_t* tpos, const double* y, int64_t N, int n, double* G, void* stream) {
  if (!obs || !tpos || !y || !G || N <= 0) return fail(MJX_ERR_ARG, "bad arguments");
  FeatTableCache* ft;
  if (int rc = get_feat_table(kind, n, &ft)) return rc;
  const int F = ft->F, FA = F + 1;
  const GramRoute r = gram_route(F, n, N, env_flag("MJX_GRAM_FMA", false));
  const size_t pbytes = (size_t)r.Z * FA * FA * sizeof(double);
  double* part = nullptr;
  if (int rc = dev_scratch(SITE_GRAM, stream, pbytes, &part)) return rc;
  const bool blk = r.arm == GRAM_MFMA_BLK;                 // that arm writes every partial it owns (tests/test_gpu_ridge_matrix.py: after a call with y x 1e6) and may take LDS beyond the default
  if (!blk) HIPCHK(hipMemsetAsync(part, 0, pbytes, (hipStream_t)stream));
  if (!blk && r.lds > LDS_DEFAULT) return fail(MJX_ERR_UNSUPPORTED, "obs dim too large for the Gram kernel's LDS staging");
  auto launch = [&](auto kern, dim3 grid, auto... lead) {
    if (int rc = lds_limit((const void*)kern, r.lds)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), r.lds, (hipStream_t)stream, lead..., ft->dev, F, n, obs, tpos, y, N, part);
    return (int)MJX_OK;
  };
  if (int rc = r.arm == GRAM_MFMA ? launch(k_bl_gram_mfma, dim3(r.Z)) : launch(blk ? k_bl_gram_mfma_blk : k_bl_gram, dim3(r.gx, r.Z), r.nblk)) return rc;
  hipLaunchKernelGGL(k_bl_gram_reduce, dim3(ew_grid((int64_t)FA * FA)), dim3(256), 0, (hipStream_t)stream, (const double*)part, r.Z, FA, G, r.blk);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_bl_predict(int kind, const double* obs, const int32_t* tpos, int64_t N, int n, const double* coef, double* out, void* stream) {
  if (!obs || !tpos || !coef || !out || N < 0) return fail(MJX_ERR_ARG, "bad arguments");
  if (N == 0) return MJX_OK;
  FeatTableCache* ft;
  if (int rc = get_feat_table(kind, n, &ft)) return rc;
  int nth = 256;                                          // one observation row per thread in LDS: fewer threads for wide observations
  while (nth > 64 && (size_t)nth * n * sizeof(double) > LDS_DEFAULT) nth >>= 1;
  size_t lds = (size_t)nth * n * sizeof(double);
  if (lds > LDS_DEFAULT) return fail(MJX_ERR_UNSUPPORTED, "obs dim too large for the predict kernel's LDS staging");
  if (int rc = lds_limit((const void*)k_bl_predict, lds)) return rc;
  hipLaunchKernelGGL(k_bl_predict, dim3(capped_grid(N, nth, 8192)), dim3(nth), lds, (hipStream_t)stream, ft->dev, ft->F, n, obs, tpos, coef, N, out);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_mlp_predict(const float* feat, int64_t N, int d_in, const int* hidden, int n_hidden, const float* params, float* out, void* stream) {
  if (!feat || !params || !out || N < 0 || d_in <= 0 || n_hidden < 0 || (n_hidden && !hidden)) return fail(MJX_ERR_ARG, "bad arguments");
  if (N == 0) return MJX_OK;
  {
    // the reference's default value network (128 x 128 ReLU) in one launch: csrc/baseline.h k_mlp_predict128 (MJX_MLP_PREDICT_FUSED=0: A/B)
    const size_t bytes = mlp_predict_lds_bytes(d_in);
    if (env_flag("MJX_MLP_PREDICT_FUSED", true) && n_hidden == 2 && hidden[0] == 128 && hidden[1] == 128 && d_in <= 64 &&
        (((uintptr_t)params) & 15) == 0 && bytes <= LDS_MAX) {
      if (int rc = lds_limit((const void*)k_mlp_predict128, bytes)) return rc;
      const int ncu = cu_count();
      const int64_t ntiles = (N + 31) / 32;
      const int64_t want = (ntiles + 7) / 8;
      MlpPredictArgs pa{feat, params, out, N, d_in};
      hipLaunchKernelGGL(k_mlp_predict128, dim3((unsigned)(want < ncu ? want : ncu)), dim3(512), bytes, (hipStream_t)stream, pa);
      HIPCHK(hipGetLastError());
      return MJX_OK;
    }
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

int mjx_mlp_fit_route(int d_in, const int* hidden, int n_hidden, int batch, int64_t N, int epochs, int32_t* out6) {
  if (!out6 || d_in <= 0 || n_hidden < 0 || (n_hidden && !hidden) || batch <= 0 || N <= 0 || epochs < 0) return fail(MJX_ERR_ARG, "bad arguments");
  for (int i = 0; i < n_hidden; ++i) if (hidden[i] <= 0) return fail(MJX_ERR_ARG, "bad hidden size");
  const MlpFitRoute r = mlp_fit_route(d_in, hidden, n_hidden, batch, N, epochs, mlp_fit_switches());
  out6[0] = r.kind; out6[1] = r.nf1; out6[2] = r.regmom; out6[3] = r.G; out6[4] = (int32_t)r.bytes; out6[5] = r.site;
  return MJX_OK;
}

int mjx_mlp_fit_adam(const float* feat, const float* y, int64_t N, int d_in, const int* hidden, int n_hidden, float* params,
                     float* m, float* v, int64_t step0, const int32_t* perm, int epochs, int batch, float lr, float wd,
                     double* epoch_loss_out, void* stream) {
  if (!feat || !y || !params || !m || !v || !perm || !epoch_loss_out || N <= 0 || batch <= 0 || epochs < 0 || n_hidden < 0)
    return fail(MJX_ERR_ARG, "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(epoch_loss_out, 0, sizeof(double) * (epochs > 0 ? epochs : 1), st));
  MlpRegressor net; net.init(d_in, hidden, n_hidden);
  const MlpFitRoute r = mlp_fit_route(d_in, hidden, n_hidden, batch, N, epochs, mlp_fit_switches());
  if (r.kind != MLPFIT_LAUNCHES) {
    const bool wide = r.kind == MLPFIT_WIDE;
    float* mvws = nullptr;
    if (int rc = dev_scratch((ScratchSite)r.site, stream, (size_t)r.G * net.P * 2 * sizeof(float), &mvws)) return rc;
    MlpFitArgs a{feat, y, perm, N, d_in, epochs, N / batch - 1, params, m, v, mvws, step0, lr, wd, epoch_loss_out};
    if (wide) {
      // the exchange block and the arrival counter: UNCACHED device memory (stores are acknowledged by memory, loads bypass the
      // per-XCD L2s -- the workgroups of one grid sit on different XCDs), allocated once per thread and device
      static thread_local PerDevice<char*> xch_of;
      char*& xch = xch_of.here();
      const size_t xbytes = (size_t)2 * MLPFIT_GMAX * 128 * 32 * sizeof(float);
      if (!xch) HIPCHK(hipExtMallocWithFlags((void**)&xch, xbytes + 256, hipDeviceMallocUncached));
      HIPCHK(hipMemsetAsync(xch + xbytes, 0, 256, st));                       // the counter (the exchange block needs no clearing)
      a.xch = (float*)xch; a.bar = (unsigned*)(xch + xbytes); a.G = r.G; a.FS = MLPFIT_FS;
      { const char* f = getenv("MJX_FIT_FAULT"); a.fault = (f && !strcmp(f, "straggler")) ? 1 : 0; }      // (tests/test_gpu_lifecycle.py)
    }
    const MlpFitKernel k = mlp_fit_kernel(r);
    if (int rc = lds_limit((const void*)k, r.bytes)) return rc;
    hipLaunchKernelGGL(k, dim3(r.G), dim3(256), r.bytes, st, a);
    // a barrier wait that timed out (a workgroup without a CU) is recorded in a word of its own; this turns it into NaN epoch
    // losses AFTER every workgroup has left -- the last writer of epoch_loss no longer decides
    if (wide) hipLaunchKernelGGL(k_mlp_fit_verdict, dim3(1), dim3(64), 0, st, (const unsigned*)a.bar + 1, epoch_loss_out, epochs);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  const int L = net.nL(), bs = batch;
  size_t hsum = 0; for (int i = 0; i < n_hidden; ++i) hsum += hidden[i];
  // scratch: Xb, yb, yhat, d_out, acts (bs x h_l), deltas (bs x h_l), grads (P)
  size_t fl = (size_t)bs * d_in + 3 * (size_t)bs + 2 * (size_t)bs * hsum + (size_t)net.P;
  float* q = nullptr;
  if (int rc = dev_scratch(SITE_MLP_FIT_LAUNCHES, stream, fl * sizeof(float), &q)) return rc;
  float* Xb = q; q += (size_t)bs * d_in;
  float* yb = q; q += bs;
  float* yhat = q; q += bs;
  float* dout = q; q += bs;
  std::vector<float*> acts(n_hidden), dl(n_hidden);
  for (int i = 0; i < n_hidden; ++i) { acts[i] = q; q += (size_t)bs * hidden[i]; }
  for (int i = 0; i < n_hidden; ++i) { dl[i] = q; q += (size_t)bs * hidden[i]; }
  float* grads = q;
  const int64_t steps = N / bs - 1;                 // optimize_model.py:24
  int64_t t = step0;
  // the fp32-beta set (vecops.h: ADAM32_*), in 1 - beta and in the corrections too: the arithmetic of the persistent trainers
  // (mlp_fit.h), self-consistent -- the steps stay within 1e-6 lr of torch's, v itself is 1.3e-5 low (tests/test_gpu_fit_matrix.py)
  for (int ep = 0; ep < epochs; ++ep) {
    for (int64_t mb = 0; mb < steps; ++mb) {
      hipLaunchKernelGGL(k_gather_rows, dim3((bs * d_in + 255) / 256), dim3(256), 0, st, feat, y, perm + (int64_t)ep * N + mb * bs, bs, d_in, Xb, yb);
      net.forward(params, Xb, bs, acts, yhat, st);
      hipLaunchKernelGGL(k_mse_grad, dim3(1), dim3(256), 0, st, yhat, yb, bs, dout, epoch_loss_out + ep);
      const float* delta = dout;
      for (int l = L - 1; l >= 0; --l) {
        const int ho = net.sizes[l + 1], hi_ = net.sizes[l];
        const float* in = (l == 0) ? Xb : acts[l - 1];
        lw_launch_gemm(gemm_wgrad(bs, ho, hi_, delta, in, hi_, grads + net.oW[l]), 1, st);
        hipLaunchKernelGGL(k_colsum, dim3((ho + 63) / 64, 1), dim3(256), 0, st, delta, (int64_t)bs, ho, (int64_t)ho, grads + net.ob[l]);
        if (l > 0) {
          lw_launch_gemm(gemm_delta(bs, ho, hi_, delta, params + net.oW[l], false, dl[l - 1], acts[l - 1], EPI_BACK_RELU), 1, st);
          delta = dl[l - 1];
        }
      }
      const AdamBias bc = adam_bias(ADAM32_B1, ADAM32_B2, ++t);
      hipLaunchKernelGGL(k_adam, dim3((unsigned)((net.P + 255) / 256)), dim3(256), 0, st, params, grads, m, v, net.P, lr, wd, ADAM32_C1, ADAM32_B2, ADAM32_C2, ADAM_EPS, bc.bc1, bc.bc2s);
    }
  }
  HIPCHK(lw_status());
  return MJX_OK;
}

// ---------------------------------------------------------------------------- model-based NPG (csrc/dynamics.h; host side: csrc/model_host.h)
int mjx_dyn_forward(const float* x, int64_t x_stride, int64_t rows, int K, const int* sizes, int n_sizes, const float* params,
                    const float* tr, int act, int flags, float* out, void* stream) {
  DynNet net;
  if (int rc = dyn_net(sizes, n_sizes, net)) return rc;
  if (!x || !params || !tr || !out || rows < 0 || !dyn_args_ok(net, K, act, DYN_TGT_PLAIN, flags & DYN_RESIDUAL)) return fail(MJX_ERR_ARG, "bad arguments");
  if (rows == 0) return MJX_OK;
  MJX_DEVICE_ENTRY();
  const size_t bytes = sizeof(float) * 3 * DYN_FT * (size_t)net.maxw;
  if (int rc = lds_limit((const void*)k_dyn_forward, bytes)) return rc;
  DynFwdArgs a{net, x, x_stride, rows, params, tr, act, flags, out};
  hipLaunchKernelGGL(k_dyn_forward, dim3((unsigned)((rows + DYN_FT - 1) / DYN_FT), (unsigned)K), dim3(256), bytes, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_model_rollout(const float* s0, int64_t N, int H, int K, const int* pol_sizes, int pol_n_sizes, const float* pol_params,
                      const float* pol_tr, const float* noise, const float* actions, const int* dyn_sizes, int dyn_n_sizes,
                      const float* dyn_params, const float* dyn_tr, int act, int flags, const float* a_min, const float* a_max,
                      const float* s_min, const float* s_max, float* obs_out, float* act_out, void* stream) {
  RolloutArgs a{};
  if (int rc = dyn_net(dyn_sizes, dyn_n_sizes, a.dyn)) return rc;
  const int n = a.dyn.dout(), m = a.dyn.din() - n;
  if (!s0 || !dyn_params || !dyn_tr || !obs_out || !act_out || N < 0 || H < 0 || m <= 0 || !dyn_args_ok(a.dyn, K, act) ||
      (!a_min) != (!a_max) || (!s_min) != (!s_max))
    return fail(MJX_ERR_ARG, "bad arguments");
  if (actions) {
    if (pol_sizes || noise) return fail(MJX_ERR_ARG, "given actions: no policy, no noise");
  } else {
    if (int rc = dyn_net(pol_sizes, pol_n_sizes, a.pol)) return rc;
    if (!pol_params || !pol_tr || a.pol.din() != n || a.pol.dout() != m) return fail(MJX_ERR_ARG, "policy does not match the state / action dims");
  }
  if (N == 0 || H == 0) return MJX_OK;
  MJX_DEVICE_ENTRY();
  a.pol_P = pol_params; a.pol_tr = pol_tr; a.noise = noise; a.a_lo = a_min; a.a_hi = a_max; a.s_lo = s_min; a.s_hi = s_max;
  return launch_model_rollout(a, s0, N, H, K, actions, dyn_params, dyn_tr, act, flags, obs_out, act_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------- MPC planning on learned models (csrc/plan.h, csrc/plan_wide.h;
// the entries with a wide route and their route queries: csrc/model_host.h)
int mjx_plan_route(const int* dyn_sizes, int dyn_n_sizes, int act_dim) { return plan_route(false, dyn_sizes, dyn_n_sizes, act_dim); }
int mjx_plan_rollout_wide_route(const int* dyn_sizes, int dyn_n_sizes, int act_dim) { return plan_route(true, dyn_sizes, dyn_n_sizes, act_dim); }
int mjx_plan_rollout(const float* s0, int64_t s0_stride, int64_t N, int H, int K, const float* actions, const int* dyn_sizes,
                     int dyn_n_sizes, const float* dyn_params, const float* dyn_tr, int act, int flags, float* obs_out, void* stream) {
  return plan_rollout(false, s0, s0_stride, N, H, K, actions, dyn_sizes, dyn_n_sizes, dyn_params, dyn_tr, act, flags, obs_out, nullptr, stream);
}
int mjx_plan_rollout_wide(const float* s0, int64_t s0_stride, int64_t N, int H, int K, const float* actions, const int* dyn_sizes,
                          int dyn_n_sizes, const float* dyn_params, const float* dyn_tr, int act, int flags, float* obs_out, int* route_out,
                          void* stream) {
  return plan_rollout(true, s0, s0_stride, N, H, K, actions, dyn_sizes, dyn_n_sizes, dyn_params, dyn_tr, act, flags, obs_out, route_out, stream);
}

int mjx_plan_score(const float* obs, const double* rewards, const double* actions, int K, int64_t N, int H, int n, int m, double kappa,
                   double gamma, double omega, int idx_mode, double* R_out, double* S_out, double* seq_out, void* stream) {
  if (!rewards || !actions || !R_out || !S_out || !seq_out || K <= 0 || K > 65535 || N <= 0 || H <= 0 || n <= 0 || m <= 0 ||
      (idx_mode != PLAN_IDX_REFERENCE && idx_mode != PLAN_IDX_TRAJECTORY))
    return fail(MJX_ERR_ARG, "bad arguments");
  if (obs && idx_mode == PLAN_IDX_REFERENCE && K > N)
    return fail(MJX_ERR_ARG, "the reference's index reads disagreement[member]: needs K <= N (model_learning_mpc.py:95)");
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  double* scr = nullptr;
  if (int rc = dev_scratch(SITE_PLAN_SCORE, stream, (size_t)(N + 1) * sizeof(double), &scr)) return rc;
  double* dis = scr + 1;
  if (obs) {
    const int64_t need = idx_mode == PLAN_IDX_REFERENCE ? K : N;         // (the reference reads entries 0 .. K-1 only)
    hipLaunchKernelGGL(k_plan_disagree, dim3((unsigned)need), dim3(64), 0, st, obs, K, N, (int64_t)H * n, dis);
  }
  const int64_t T = K * N;
  hipLaunchKernelGGL(k_plan_returns, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, rewards, obs ? dis : nullptr, K, N, H, gamma, omega,
                     idx_mode, R_out);
  hipLaunchKernelGGL(k_plan_softmax, dim3(1), dim3(1024), 0, st, R_out, T, kappa, S_out, scr);
  hipLaunchKernelGGL(k_plan_sequence, dim3((unsigned)(H * m)), dim3(256), 0, st, S_out, scr, actions, K, N, (int64_t)H * m, seq_out);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

// ---------------------------------------------------------------------------- learned path rewards (csrc/path_reward.h, csrc/rows_wide.h)
int mjx_rows_wide_tile_rows(void) { return 32 * RW_NS; }
int mjx_path_rewards_route(const int* dyn_sizes, int dyn_n_sizes, const int* rew_sizes, int rew_n_sizes) {
  return path_rewards_route(false, dyn_sizes, dyn_n_sizes, rew_sizes, rew_n_sizes);
}
int mjx_path_rewards_wide_route(const int* dyn_sizes, int dyn_n_sizes, const int* rew_sizes, int rew_n_sizes) {
  return path_rewards_route(true, dyn_sizes, dyn_n_sizes, rew_sizes, rew_n_sizes);
}
int mjx_path_rewards(const float* obs, const float* act, int64_t act_stride, int64_t rows, int K, const int* dyn_sizes, int dyn_n_sizes,
                     const float* dyn_params, const float* dyn_tr, int dyn_act, int dyn_flags, const int* rew_sizes, int rew_n_sizes,
                     const float* rew_params, const float* rew_tr, int rew_act, float* r32_out, double* r64_out, int* route_out,
                     void* stream) {
  return path_rewards(false, obs, act, act_stride, rows, K, dyn_sizes, dyn_n_sizes, dyn_params, dyn_tr, dyn_act, dyn_flags, rew_sizes, rew_n_sizes,
                      rew_params, rew_tr, rew_act, r32_out, r64_out, route_out, stream);
}
int mjx_path_rewards_wide(const float* obs, const float* act, int64_t act_stride, int64_t rows, int K, const int* dyn_sizes, int dyn_n_sizes,
                          const float* dyn_params, const float* dyn_tr, int dyn_act, int dyn_flags, const int* rew_sizes, int rew_n_sizes,
                          const float* rew_params, const float* rew_tr, int rew_act, float* r32_out, double* r64_out, int* route_out,
                          void* stream) {
  return path_rewards(true, obs, act, act_stride, rows, K, dyn_sizes, dyn_n_sizes, dyn_params, dyn_tr, dyn_act, dyn_flags, rew_sizes, rew_n_sizes,
                      rew_params, rew_tr, rew_act, r32_out, r64_out, route_out, stream);
}

// ---------------------------------------------------------------------------- policy rollout on learned models (csrc/policy_rollout.h, csrc/policy_rollout_wide.h)
int mjx_policy_rollout_route(const int* pol_sizes, int pol_n_sizes, const int* dyn_sizes, int dyn_n_sizes) {
  return policy_rollout_route(false, pol_sizes, pol_n_sizes, dyn_sizes, dyn_n_sizes);
}
int mjx_policy_rollout_wide_route(const int* pol_sizes, int pol_n_sizes, const int* dyn_sizes, int dyn_n_sizes) {
  return policy_rollout_route(true, pol_sizes, pol_n_sizes, dyn_sizes, dyn_n_sizes);
}
int mjx_policy_rollout(const float* s0, int64_t s0_stride, int64_t N, int H, int K, const int* pol_sizes, int pol_n_sizes,
                       const float* pol_params, const float* pol_tr, const float* noise, int64_t noise_stride, const int* dyn_sizes,
                       int dyn_n_sizes, const float* dyn_params, const float* dyn_tr, int act, int flags, const float* a_min,
                       const float* a_max, const float* s_min, const float* s_max, float* obs_out, float* act_out, int* route_out,
                       void* stream) {
  return policy_rollout(false, s0, s0_stride, N, H, K, pol_sizes, pol_n_sizes, pol_params, pol_tr, noise, noise_stride, dyn_sizes, dyn_n_sizes,
                        dyn_params, dyn_tr, act, flags, a_min, a_max, s_min, s_max, obs_out, act_out, route_out, stream);
}
int mjx_policy_rollout_wide(const float* s0, int64_t s0_stride, int64_t N, int H, int K, const int* pol_sizes, int pol_n_sizes,
                            const float* pol_params, const float* pol_tr, const float* noise, int64_t noise_stride, const int* dyn_sizes,
                            int dyn_n_sizes, const float* dyn_params, const float* dyn_tr, int act, int flags, const float* a_min,
                            const float* a_max, const float* s_min, const float* s_max, float* obs_out, float* act_out, int* route_out,
                            void* stream) {
  return policy_rollout(true, s0, s0_stride, N, H, K, pol_sizes, pol_n_sizes, pol_params, pol_tr, noise, noise_stride, dyn_sizes, dyn_n_sizes,
                        dyn_params, dyn_tr, act, flags, a_min, a_max, s_min, s_max, obs_out, act_out, route_out, stream);
}

// ---------------------------------------------------------------------------- device-resident model rollouts (csrc/rollout_batch.h, csrc/rows_wide.h)
int mjx_rollout_disagreement_route(const int* dyn_sizes, int dyn_n_sizes) { return rollout_disagreement_route(false, dyn_sizes, dyn_n_sizes); }
int mjx_rollout_disagreement_wide_route(const int* dyn_sizes, int dyn_n_sizes) { return rollout_disagreement_route(true, dyn_sizes, dyn_n_sizes); }
int mjx_rollout_disagreement(const float* obs, const float* act, int64_t P, int H, int K, const int* dyn_sizes, int dyn_n_sizes,
                             const float* dyn_params, const float* dyn_tr, int dyn_act, int dyn_flags, float* err_out, int* route_out,
                             void* stream) {
  return rollout_disagreement(false, obs, act, P, H, K, dyn_sizes, dyn_n_sizes, dyn_params, dyn_tr, dyn_act, dyn_flags, err_out, route_out, stream);
}
int mjx_rollout_disagreement_wide(const float* obs, const float* act, int64_t P, int H, int K, const int* dyn_sizes, int dyn_n_sizes,
                                  const float* dyn_params, const float* dyn_tr, int dyn_act, int dyn_flags, float* err_out, int* route_out,
                                  void* stream) {
  return rollout_disagreement(true, obs, act, P, H, K, dyn_sizes, dyn_n_sizes, dyn_params, dyn_tr, dyn_act, dyn_flags, err_out, route_out, stream);
}

int mjx_rollout_pack(const float* obs, const float* act, const float* rew32, const double* rew64, const float* err, int64_t P, int H, int n,
                     int m, double lim, int min_len, double truncate_reward, int64_t* off_out, int32_t* first_out, uint8_t* term_out,
                     float* obs_out, float* act_out, double* rew_out, double* obs64_out, int32_t* tpos_out, void* stream) {
  if (!obs || !act || (!rew32) == (!rew64) || P < 0 || H < 1 || n <= 0 || m <= 0 || min_len < 1 || lim != lim || !off_out || !first_out ||
      !term_out || !obs_out || !act_out || !rew_out)
    return fail(MJX_ERR_ARG, "bad arguments");
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  if (P > 0) hipLaunchKernelGGL(k_rp_first, dim3(capped_grid(P, 256, 4096)), dim3(256), 0, st, err, P, H, lim, min_len, off_out, first_out, term_out);
  hipLaunchKernelGGL(k_rp_scan, dim3(1), dim3(1024), 0, st, P, off_out);
  if (P > 0) {
    const RollPackArgs a{obs, act, rew32, rew64, off_out, first_out, obs_out, act_out, rew_out, obs64_out, tpos_out, P, H, n, m, truncate_reward};
    hipLaunchKernelGGL(k_rp_rows, dim3(capped_grid(P * H * (n + m + 1), 256, 8192)), dim3(256), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_cast_f32_f64(const float* src, int64_t count, double* dst, void* stream) {
  if (count < 0 || (count > 0 && (!src || !dst))) return fail(MJX_ERR_ARG, "bad arguments");
  if (count == 0) return MJX_OK;
  MJX_DEVICE_ENTRY();
  hipLaunchKernelGGL(k_pr_widen, dim3(capped_grid(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, src, count, dst);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_dyn_fit_adam(const float* x, const float* y, int64_t N, const int* sizes, int n_sizes, const float* in_tr, const float* out_tr,
                     int target_mode, int act, float* params, float* m, float* v, int64_t step0, const int32_t* idx, int64_t steps,
                     int batch, float lr, float wd, float* loss_out, void* stream) {
  DynNet net;
  if (int rc = dyn_net(sizes, n_sizes, net)) return rc;
  const int din = net.din(), dout = net.dout();
  if (!x || !y || !in_tr || !out_tr || !params || !m || !v || (steps > 0 && (!idx || !loss_out)) || N <= 0 || batch <= 0 || batch > N ||
      steps < 0 || step0 < 0 || !dyn_args_ok(net, 1, act, target_mode))
    return fail(MJX_ERR_ARG, "bad arguments");
  if (steps == 0) return MJX_OK;
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

// route 1 of both ensemble entries: per-member prep into scratch, then one k_dyn_fit_ens<RAG> launch per DFE_CHUNK members
extern "C++" {
template <bool RAG>
static int dfe_run(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int64_t N, int K, const DynNet& net, const float* in_tr,
                   const float* out_tr, int target_mode, int act, float* params, float* m, float* v, const int64_t* step0,
                   const int32_t* idx, int64_t steps, int batch, float lr, float wd, float* loss_out, void* stream) {
  const int din = net.din(), dout = net.dout();
  MJX_DEVICE_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  const DfeLayout L(net, batch);
  // scratch, per member: normalised inputs and targets (every member has its own transforms), and the X tile where LDS has no room
  const size_t xt = L.x_in_lds ? 0 : L.xtile;
  float* scr = nullptr;
  if (int rc = dev_scratch(SITE_DYN_FIT_ENS, stream, ((size_t)K * (size_t)N * (din + dout) + 4 + (size_t)K * xt) * sizeof(float), &scr)) return rc;
  float* xn = scr; float* tg = xn + (size_t)K * N * din;
  float* xscr = xt ? scr + (((size_t)K * N * (din + dout) + 3) & ~(size_t)3) : nullptr;
  for (int k = 0; k < K; ++k)
    launch_dyn_prep(x + k * x_stride, y + k * y_stride, N, din, dout, in_tr + (int64_t)k * 2 * din, out_tr + (int64_t)k * 2 * dout, target_mode,
                    xn + (size_t)k * N * din, tg + (size_t)k * N * dout, st);
  if (int rc = lds_limit((const void*)k_dyn_fit_ens<RAG>, L.lds_bytes())) return rc;
  DynFitEnsArgs a{};
  a.din = din; a.h1 = net.sz[1]; a.h2 = net.sz[2]; a.dout = dout; a.B = batch; a.act = act;
  a.P = net.P; a.N = N; a.steps = steps; a.xn = xn; a.tg = tg; a.idx = idx; a.W = params; a.m = m; a.v = v; a.loss = loss_out; a.xscr = xscr;
  a.lr = lr; a.wd = wd; a.otr = RAG ? out_tr : nullptr;
  for (int k0 = 0; k0 < K; k0 += DFE_CHUNK) {               // one launch for K <= DFE_CHUNK members
    const int kn = K - k0 < DFE_CHUNK ? K - k0 : DFE_CHUNK;
    a.k0 = k0;
    for (int q = 0; q < kn; ++q) a.step0[q] = step0[k0 + q];
    hipLaunchKernelGGL(k_dyn_fit_ens<RAG>, dim3((unsigned)kn), dim3(DFE_THREADS), L.lds_bytes(), st, a);
  }
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

// the body of both ensemble entries, after the sizes are parsed: the argument check, the route (the entry's switch, read per call -- the
// tests and tools/bench_dyn_fit.py compare the two routes in one process -- and what its shape predicate answered) written to route_out,
// then route 0, member by member on the routes of mjx_dyn_fit_adam, or route 1, dfe_run<RAG>
template <bool RAG>
static int dfe_entry(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int64_t N, int K, const int* sizes, int n_sizes,
                     const DynNet& net, const float* in_tr, const float* out_tr, int target_mode, int act, float* params, float* m, float* v,
                     const int64_t* step0, const int32_t* idx, int64_t steps, int batch, float lr, float wd, float* loss_out,
                     const char* switch_name, bool shape_served, int* route_out, void* stream) {
  const int din = net.din(), dout = net.dout();
  if (!x || !y || !in_tr || !out_tr || !params || !m || !v || !step0 || (steps > 0 && (!idx || !loss_out)) || N <= 0 ||
      x_stride < 0 || y_stride < 0 || batch <= 0 || batch > N || steps < 0 || !dyn_args_ok(net, K, act, target_mode))
    return fail(MJX_ERR_ARG, "bad arguments");
  for (int k = 0; k < K; ++k) if (step0[k] < 0) return fail(MJX_ERR_ARG, "bad arguments");
  const int route = env_flag(switch_name, true) && shape_served ? 1 : 0;
  if (route_out) *route_out = route;
  if (steps == 0) return MJX_OK;
  if (route == 0) {
    for (int k = 0; k < K; ++k)
      if (int rc = mjx_dyn_fit_adam(x + k * x_stride, y + k * y_stride, N, sizes, n_sizes, in_tr + (int64_t)k * 2 * din, out_tr + (int64_t)k * 2 * dout,
                                    target_mode, act, params + k * net.P, m + k * net.P, v + k * net.P, step0[k],
                                    idx + (int64_t)k * steps * batch, steps, batch, lr, wd, loss_out + (int64_t)k * steps, stream))
        return rc;
    return MJX_OK;
  }
  return dfe_run<RAG>(x, x_stride, y, y_stride, N, K, net, in_tr, out_tr, target_mode, act, params, m, v, step0, idx, steps, batch, lr, wd,
                      loss_out, stream);
}
}  // extern "C++"

// ---- the whole ensemble's fit (csrc/dyn_fit_ens.h)
int mjx_dyn_fit_route(const int* sizes, int n_sizes, int batch, int target_mode) {
  DynNet net;
  if (int rc = dyn_net(sizes, n_sizes, net)) return rc;
  if (batch <= 0 || target_mode < DYN_TGT_AFFINE || target_mode > DYN_TGT_RESIDUAL) return fail(MJX_ERR_ARG, "bad batch or target mode");
  return dfe_serves(net, batch, target_mode) ? 1 : 0;
}

int mjx_dyn_fit_ensemble(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int64_t N, int K, const int* sizes, int n_sizes,
                         const float* in_tr, const float* out_tr, int target_mode, int act, float* params, float* m, float* v,
                         const int64_t* step0, const int32_t* idx, int64_t steps, int batch, float lr, float wd, float* loss_out,
                         int* route_out, void* stream) {
  DynNet net;
  if (int rc = dyn_net(sizes, n_sizes, net)) return rc;
  return dfe_entry<false>(x, x_stride, y, y_stride, N, K, sizes, n_sizes, net, in_tr, out_tr, target_mode, act, params, m, v, step0, idx, steps,
                          batch, lr, wd, loss_out, "MJX_DYN_FIT_ENS", dfe_serves(net, batch, target_mode), route_out, stream);
}

// ---- the reward nets of the whole ensemble (target mode 0: the loss runs through the output affine on raw r)
int mjx_reward_fit_route(const int* sizes, int n_sizes, int batch) {
  DynNet net;
  if (int rc = dyn_net(sizes, n_sizes, net)) return rc;
  if (batch <= 0) return fail(MJX_ERR_ARG, "bad batch");
  return reward_fit_serves(net, batch) ? 1 : 0;
}

int mjx_dyn_fit_ens_layout(const int* sizes, int n_sizes, int batch, int64_t* info) {
  DynNet net;
  if (int rc = dyn_net(sizes, n_sizes, net)) return rc;
  if (!info || batch <= 0 || !reward_fit_serves(net, batch)) return fail(MJX_ERR_ARG, "not a shape of the ensemble kernel");
  const DfeLayout L(net, batch);
  info[0] = (int64_t)L.lds_bytes(); info[1] = L.x_in_lds ? 1 : 0; info[2] = L.ST; info[3] = (int64_t)L.xtile;
  return MJX_OK;
}

int mjx_reward_fit_ensemble(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int64_t N, int K, const int* sizes,
                            int n_sizes, const float* in_tr, const float* out_tr, int act, float* params, float* m, float* v,
                            const int64_t* step0, const int32_t* idx, int64_t steps, int batch, float lr, float wd, float* loss_out,
                            int* route_out, void* stream) {
  DynNet net;
  if (int rc = dyn_net(sizes, n_sizes, net)) return rc;
  return dfe_entry<true>(x, x_stride, y, y_stride, N, K, sizes, n_sizes, net, in_tr, out_tr, DYN_TGT_AFFINE, act, params, m, v, step0, idx, steps,
                         batch, lr, wd, loss_out, "MJX_REWARD_FIT_ENS", reward_fit_serves(net, batch), route_out, stream);
}

int mjx_dyn_pred_error(const float* pred, int K, int64_t rows, int n, const float* s_next, const int64_t* seg_off, int nseg, double lim,
                       float* err_out, int32_t* first_out, void* stream) {
  if (!pred || !s_next || !seg_off || !err_out || !first_out || K <= 0 || rows < 0 || n <= 0 || nseg < 0) return fail(MJX_ERR_ARG, "bad arguments");
  if (nseg == 0) return MJX_OK;
  MJX_DEVICE_ENTRY();
  hipLaunchKernelGGL(k_dyn_pred_err, dim3((unsigned)nseg), dim3(256), 0, (hipStream_t)stream, pred, K, rows, n, s_next, seg_off, lim, err_out, first_out);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_profile_enable(mjx_ctx* c, int on) {
  if (!c) return fail(MJX_ERR_ARG, "null context");
  HIPCHK(hipSetDevice(c->device));
  return c->prof.enable(on);
}

int mjx_profile_read(mjx_ctx* c, double* out) {
  if (!c || !out) return fail(MJX_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(c->device));
  double tot = 0.0, ms = 0.0;
  for (size_t i = 0; i < c->prof.used; ++i) {
    if (int rc = c->prof.elapsed(i, &ms)) return rc;
    tot += ms;
  }
  out[0] = tot; out[1] = (double)c->prof.used;
  return MJX_OK;
}

int mjx_profile_samples(mjx_ctx* c, double* ms_out_host, int cap, int* count_out) {
  if (!c || !count_out || (cap > 0 && !ms_out_host)) return fail(MJX_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(c->device));
  for (size_t i = 0; i < c->prof.used && (int64_t)i < cap; ++i)
    if (int rc = c->prof.elapsed(i, ms_out_host + i)) return rc;
  *count_out = (int)c->prof.used;
  return MJX_OK;
}

int mjx_set_debug_buffer(mjx_ctx* c, float* dbg, int64_t floats) {
  if (!c || (dbg && floats < 2048 * 8)) return fail(MJX_ERR_ARG, "debug buffer too small");
  c->dbg = dbg;
#ifdef MJX_PHASE_CLOCK
  // timing build: a buffer of at least LW_CLK_SLOTS slots also receives the per-workgroup stamps of the next k_gemm launches
  lw_clk_buf() = (dbg && floats >= 2 * (int64_t)LW_CLK_SLOT * LW_CLK_SLOTS) ? (long long*)dbg : nullptr;
  lw_clk_slot() = 0;
#endif
  return MJX_OK;
}

int mjx_set_clock_buffer(mjx_ctx* c, int64_t* clk) {
  if (!c) return fail(MJX_ERR_ARG, "null context");
  c->clk = (long long*)clk;
  return MJX_OK;
}

}  // extern "C"
namespace {
// K1, the Fisher-vector product and K3 on the bound inputs, declared in update_host.h for the solve and the updates.
// pp (peer exchange): the gradient's reduction kernel writes this rank's slot (grad_out IS that slot) into every peer's buffer,
// K1's 4 sums travel with it at byte scal_off of the slot (scal_out: that place in the own slot), one arrival flag for both
int surr_vpg_impl(mjx_ctx* c, float* grad_out, double* scal_out, void* stream, const PeerPush* pp, int scal_off) {
  if (int rc = check_bound(c, true)) return rc;
  if (!grad_out || !scal_out) return fail(MJX_ERR_ARG, "null output");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(c->device));
  if (c->N_local == 0) {                       // a rank without trajectories contributes zeros
    HIPCHK(hipMemsetAsync(grad_out, 0, c->d * sizeof(float), st));
    HIPCHK(hipMemsetAsync(scal_out, 0, 4 * sizeof(double), st));
    return MJX_OK;
  }
  if (c->fz.variant) return c->fz.surr_vpg(bound_args(c, c->theta_old), grad_out, scal_out, pp, scal_off, st, &c->lw_old_ok);
  if (c->lw.surr_vpg(c->obs, c->act, c->adv, c->N_local, c->N_global, c->theta_new, c->theta_old, tr_new_or_ident(c), tr_old_or_ident(c),
                     c->old_is_new, grad_out, scal_out, st)) return fail(MJX_ERR_STATE, "layer-wise surr_vpg failed");
  c->lw_old_ok = c->old_is_new != 0;            // its output block now holds the old policy's means for the bound rows
  return MJX_OK;
}

// pp: peer exchange folded into the reduction kernel (fused kernels with d % 4 == 0 only; `out` is then this rank's slot)
int fvp_impl(mjx_ctx* c, const float* v, float* out, void* stream, const PeerPush* pp) {
  if (int rc = check_bound(c, false)) return rc;
  if (!v || !out) return fail(MJX_ERR_ARG, "null vector");
  if (c->fz.variant && (((uintptr_t)v) & 15)) return fail(MJX_ERR_ARG, "v must be 16-byte aligned (fused path)");   // (the layer-wise path takes any 4-byte aligned v)
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(c->device));
  if (c->N_local == 0) { HIPCHK(hipMemsetAsync(out, 0, c->d * sizeof(float), st)); return MJX_OK; }
  if (!c->old_is_new) {
    // general position (e.g. input_normalization, npg_cg.py:101-107): exact Pearlmutter product on the layer-wise path
    if (int rc = c->lw.ensure_rows(c->N_local)) return fail(rc, "layer-wise workspace allocation failed");
    int rc = c->lw.hvp_general(c->obs, c->N_local, c->N_global, c->theta_new, c->theta_old, tr_new_or_ident(c), tr_old_or_ident(c), v, out, st);
    return rc ? fail(MJX_ERR_STATE, "general Hessian-vector product failed (%d)", rc) : MJX_OK;
  }
  int pair;
  if (int rc = c->prof.begin(ProfPick::PRODUCT, false, st, &pair)) return rc;
  // (the bracket closes behind the product itself: the fused path's reduction of the partials stays outside it)
  auto prof_end = [&]() -> int { return c->prof.end(pair, st); };
  if (c->fz.variant) return c->fz.fvp(bound_args(c, v), out, (float)((double)c->N_local / (double)c->N_global), pp, st, prof_end);
  const int rc = c->lw.fvp(c->obs, c->N_local, c->N_global, c->theta_new, tr_new_or_ident(c), v, out, st);
  if (int e = prof_end()) return e;
  return rc ? fail(MJX_ERR_STATE, "layer-wise fvp failed") : MJX_OK;
}

// pp (peer exchange): the reduction of K3's sums writes them into slot `rank` of every buffer (scal_out IS the own slot) and raises
// the flags; the caller launches the consumer (k_peer_sum<double>)
int eval_impl(mjx_ctx* c, double* scal_out, void* stream, const PeerPush* pp, bool old_ok) {
  if (int rc = check_bound(c, true)) return rc;
  if (!scal_out) return fail(MJX_ERR_ARG, "null output");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(c->device));
  if (c->N_local == 0) { HIPCHK(hipMemsetAsync(scal_out, 0, 4 * sizeof(double), st)); return MJX_OK; }
  if (c->fz.variant) return c->fz.eval(bound_args(c, c->theta_old), scal_out, pp, old_ok && c->lw_old_ok, st);
  return c->lw.eval(c->obs, c->act, c->adv, c->N_local, c->theta_new, c->theta_old, tr_new_or_ident(c), tr_old_or_ident(c), scal_out, st,
                    old_ok && c->lw_old_ok, c->old_is_new != 0)
             ? fail(MJX_ERR_STATE, "layer-wise eval failed") : MJX_OK;
}
}  // namespace
extern "C" {

int mjx_surr_vpg(mjx_ctx* c, float* grad_out, double* scal_out, void* stream) { return surr_vpg_impl(c, grad_out, scal_out, stream, nullptr, -1); }
int mjx_fvp(mjx_ctx* c, const float* v, float* out, void* stream) { return fvp_impl(c, v, out, stream, nullptr); }
int mjx_eval_surr_kl(mjx_ctx* c, double* scal_out, void* stream) { return eval_impl(c, scal_out, stream, nullptr, false); }

// ---------------------------------------------------------------------------- the solve, call by call and whole (csrc/update_host.h: CgWS, cg_solve_impl)
int mjx_cg_init(mjx_ctx* c, const float* b, void* stream) {
  if (!c || !b) return fail(MJX_ERR_ARG, "bad arguments");
  c->fz.on_solve();
  return c->cg.init(b, (hipStream_t)stream);
}
const float* mjx_cg_p(mjx_ctx* c) { return c ? c->cg.p : nullptr; }
int mjx_cg_step(mjx_ctx* c, const float* Ap, float damping, double tol, void* stream) {
  if (!c || !Ap) return fail(MJX_ERR_ARG, "bad arguments");
  return c->cg.step(Ap, nullptr, CgFin{}, damping, tol, (hipStream_t)stream);
}
int mjx_cg_finish(mjx_ctx* c, const float* b, float* x_out, double* bdotx_out, void* stream) {
  if (!c || !b) return fail(MJX_ERR_ARG, "bad arguments");
  return c->cg.finish(b, x_out, bdotx_out, (hipStream_t)stream);
}
int mjx_cg_solve(mjx_ctx* c, const float* b, int iters, float damping, double tol, float* x_out, double* bdotx_out,
                 mjx_allreduce_fn allreduce, void* user, void* stream) {
  if (!c || !b || iters < 0) return fail(MJX_ERR_ARG, "bad arguments");
  SolveReq q{const_cast<float*>(b), iters, damping, tol, x_out, bdotx_out, fin_only(), stream};
  q.allreduce = allreduce; q.user = user;
  return cg_solve_impl(c, q);
}

// ---------------------------------------------------------------------------- multi-rank: RCCL (bound at run time), the hook, the peer exchange (csrc/update_host.h: Transport)
int mjx_comm_unique_id(char* id_out) {
  if (!id_out) return fail(MJX_ERR_ARG, "null id buffer");
  RcclApi& r = rccl();
  if (!r.load()) return fail(MJX_ERR_UNSUPPORTED, "%s", r.error.c_str());
  RcclApi::UniqueId id;
  if (int rc = r.GetUniqueId(&id)) return fail(1000 + rc, "ncclGetUniqueId: %s", r.GetErrorString(rc));
  memcpy(id_out, id.internal, MJX_COMM_ID_BYTES);
  return MJX_OK;
}
int mjx_comm_init(mjx_ctx* c, int rank, int world, const char* id_host) {
  if (!c || !id_host || world < 1 || rank < 0 || rank >= world) return fail(MJX_ERR_ARG, "bad arguments");
  return c->tp.attach_rccl(rank, world, id_host);
}
int mjx_comm_destroy(mjx_ctx* c) {
  if (!c) return fail(MJX_ERR_ARG, "null context");
  c->tp.detach();
  return MJX_OK;
}
int mjx_comm_world(const mjx_ctx* c) { return c ? c->tp.world() : 0; }
int mjx_peer_export(mjx_ctx* c, int rank, int world, char* handle_out) {
  if (!c || !handle_out || world < 2 || world > PEER_MAX_WORLD || rank < 0 || rank >= world) return fail(MJX_ERR_ARG, "bad arguments (2 <= world <= 16)");
  return c->tp.peer_export(rank, world, handle_out);
}
int mjx_peer_connect(mjx_ctx* c, const char* handles) {
  if (!c) return fail(MJX_ERR_ARG, "null context");
  return c->tp.peer_connect(handles);
}
int mjx_peer_status(mjx_ctx* c, int* timeouts_out) {
  if (!c || !timeouts_out) return fail(MJX_ERR_ARG, "bad arguments");
  return c->tp.peer_status(timeouts_out);
}
int mjx_comm_set_callback(mjx_ctx* c, mjx_reduce_fn fn, void* user, int world) {
  if (!c || (fn && world < 1)) return fail(MJX_ERR_ARG, "bad arguments");
  return c->tp.attach_hook(fn, user, world);
}
int mjx_comm_allreduce(mjx_ctx* c, void* buf, int64_t count, int dtype, void* stream) {
  if (!c || !buf || count < 0 || (dtype != 0 && dtype != 1)) return fail(MJX_ERR_ARG, "bad arguments");
  return c->tp.allreduce(buf, count, dtype, stream);
}

// ---------------------------------------------------------------------------- the one-call updates (csrc/update_host.h)
int mjx_npg_update(mjx_ctx* c, int iters, float damping, double tol, double step_size, double const_alpha, float min_log_std,
                   float* grad_out, float* x_out, float* theta_out, double* results, void* stream) {
  if (int rc = update_prologue(c, "mjx_npg_update", grad_out && x_out && theta_out && results && iters >= 0, true, theta_out)) return rc;
  const float* base = c->theta_old;               // == theta_new in value; theta_out may be the theta_new buffer itself
  // (theta_out == theta_new: the stepped parameters are written by the solve's LAST kernel, after every product has read theta)
  if (int rc = vpg_then_solve(c, iters, damping, tol, grad_out, x_out, results,
                              fin_step(base, theta_out, results + 9, step_size, const_alpha, min_log_std), stream)) return rc;
  if (int rc = bind_policy_impl(c, theta_out, c->theta_old, c->tr_new, c->tr_old, 0, true)) return rc;
  return eval_and_rank_sum(c, results, stream);
}

int mjx_trpo_update(mjx_ctx* c, int iters, float damping, double tol, double step_size, double kl_dist, int n_trials, int first,
                    float min_log_std, float* grad_out, float* x_out, float* theta_out, double* results, void* stream) {
  if (int rc = update_prologue(c, "mjx_trpo_update", grad_out && x_out && theta_out && results && iters >= 0 && n_trials >= 1 && n_trials <= 24,
                               false, theta_out)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (first) {
    if (!c->old_is_new) return fail(MJX_ERR_STATE, "mjx_trpo_update starts from theta_new == theta_old (mjx_bind_policy with old_is_new)");
    if (int rc = vpg_then_solve(c, iters, damping, tol, grad_out, x_out, results, fin_only(), stream)) return rc;
  }
  for (int t = 0; t < n_trials; ++t) {
    hipLaunchKernelGGL(k_trpo_try, dim3((c->d + 255) / 256), dim3(256), 0, st, c->theta_old, x_out, results, step_size,
                       (first && t == 0) ? 1 : 0, min_log_std, theta_out, (int)c->d, c->oS);
    HIPCHK(hipGetLastError());
    if (first && t == 0) { if (int rc = bind_policy_impl(c, theta_out, c->theta_old, c->tr_new, c->tr_old, 0, true)) return rc; }
    if (int rc = eval_and_rank_sum(c, results, stream)) return rc;
    hipLaunchKernelGGL(k_trpo_check, dim3(1), dim3(64), 0, st, results, kl_dist, (double)c->N_global);
    HIPCHK(hipGetLastError());
  }
  return MJX_OK;
}

// (its own sequence: the gradient is scaled between its rank sum and the solve, so that exchange is never folded into the solve)
int mjx_dapg_update(mjx_ctx* c, int iters, float damping, double tol, double step_size, float min_log_std, int64_t rows_on,
                    int64_t N_on_global, const float* adv_on, float* grad_out, float* x_out, float* theta_out, double* results,
                    void* stream) {
  if (int rc = update_prologue(c, "mjx_dapg_update", grad_out && x_out && theta_out && results && (adv_on || rows_on <= 0) && iters >= 0,   // (a rank without on-policy rows has no advantages)
                               true, theta_out)) return rc;
  if (rows_on < 0 || rows_on > c->N_local || N_on_global <= 0 || N_on_global > c->N_global) return fail(MJX_ERR_ARG, "bad on-policy row counts");
  hipStream_t st = (hipStream_t)stream;
  // the vanilla gradient over [on-policy ; demonstrations] (mean over N_all), then x N_all / N_on (dapg.py:97-98)
  const float coef = (float)((double)c->N_global / (double)N_on_global);
  if (int rc = surr_vpg_impl(c, grad_out, results + 4, stream, nullptr, -1)) return rc;
  if (c->tp.attached()) if (int rc = c->tp.allreduce(grad_out, c->d, 0, stream)) return rc;
  hipLaunchKernelGGL(k_scale_f32, dim3((c->d + 255) / 256), dim3(256), 0, st, grad_out, coef, (int)c->d);
  HIPCHK(hipGetLastError());
  // Fisher metric, surrogate and KL: the on-policy prefix with its own advantages, means over the on-policy count (:92, :103)
  if (int rc = mjx_bind_rows(c, rows_on, N_on_global, adv_on)) return rc;
  if (int rc = eval_and_rank_sum(c, results + 4, stream)) return rc;                   // surr_before (theta_new == theta_old)
  if (int rc = cg_solve_impl(c, SolveReq{grad_out, iters, damping, tol, x_out, results + 8,
                                         fin_step(c->theta_old, theta_out, results + 9, step_size, std::nan(""), min_log_std), stream})) return rc;
  if (int rc = bind_policy_impl(c, theta_out, c->theta_old, c->tr_new, c->tr_old, 0, true)) return rc;
  return eval_and_rank_sum(c, results, stream);
}

int mjx_apply_step(mjx_ctx* c, const float* theta, const float* x, float alpha, float min_log_std, float* theta_out, void* stream) {
  if (!c || !theta || !x || !theta_out) return fail(MJX_ERR_ARG, "bad arguments");
  hipLaunchKernelGGL(k_apply_step, dim3((c->d + 255) / 256), dim3(256), 0, (hipStream_t)stream, theta, x, alpha, min_log_std,
                     theta_out, (int)c->d, c->oS);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_apply_npg_step(mjx_ctx* c, const float* theta, const float* x, const double* gdotx, double step_size, float min_log_std,
                       float* theta_out, double* alpha_out, void* stream) {
  if (!c || !theta || !x || !gdotx || !theta_out) return fail(MJX_ERR_ARG, "bad arguments");
  hipLaunchKernelGGL(k_apply_npg_step, dim3((c->d + 255) / 256), dim3(256), 0, (hipStream_t)stream, theta, x, gdotx, step_size,
                     min_log_std, theta_out, alpha_out, (int)c->d, c->oS);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_discount_scan(const double* x, const int64_t* offsets, int64_t n_traj, double gamma, double* y, void* stream) {
  if (n_traj == 0) return MJX_OK;
  if (!x || !offsets || !y || n_traj < 0) return fail(MJX_ERR_ARG, "bad arguments");
  hipLaunchKernelGGL(k_traj_scan<0>, dim3((unsigned)n_traj), dim3(256), 0, (hipStream_t)stream, x, (const double*)nullptr,
                     offsets, (const uint8_t*)nullptr, gamma, gamma, y);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_time_index(const int64_t* offsets, int64_t n_traj, int32_t* tpos, void* stream) {
  if (n_traj == 0) return MJX_OK;
  if (!offsets || !tpos || n_traj < 0) return fail(MJX_ERR_ARG, "bad arguments");
  hipLaunchKernelGGL(k_time_index, dim3((unsigned)n_traj), dim3(256), 0, (hipStream_t)stream, offsets, tpos);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_gae(const double* rewards, const double* baseline, const int64_t* offsets, const uint8_t* terminated,
            int64_t n_traj, double gamma, double lam, double* adv, void* stream) {
  if (n_traj == 0) return MJX_OK;
  if (!rewards || !baseline || !offsets || !adv || n_traj < 0) return fail(MJX_ERR_ARG, "bad arguments");
  if (lam < 0.0 || lam > 1.0 || std::isnan(lam))
    hipLaunchKernelGGL(k_traj_scan<2>, dim3((unsigned)n_traj), dim3(256), 0, (hipStream_t)stream, rewards, baseline, offsets,
                       terminated, gamma, 0.0, adv);
  else
    hipLaunchKernelGGL(k_traj_scan<1>, dim3((unsigned)n_traj), dim3(256), 0, (hipStream_t)stream, rewards, baseline, offsets,
                       terminated, gamma, gamma * lam, adv);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_sum_stats(const double* x, int64_t N, double shift, double* stats_out, void* stream) {
  if (!x || !stats_out || N < 0) return fail(MJX_ERR_ARG, "bad arguments");
  const int G = 512;
  double* part = nullptr;
  if (int rc = dev_scratch(SITE_SUM_STATS, stream, G * 2 * sizeof(double), &part)) return rc;
  hipLaunchKernelGGL(k_sum_stats_partial, dim3(G), dim3(256), 0, (hipStream_t)stream, x, N, shift, part);
  hipLaunchKernelGGL(k_sum_stats_final, dim3(1), dim3(256), 0, (hipStream_t)stream, part, G, N, stats_out);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_whiten_cast(const double* adv, int64_t N, double mean, double std, double eps, float* out32, void* stream) {
  if (!adv || !out32 || N < 0) return fail(MJX_ERR_ARG, "bad arguments");
  if (N == 0) return MJX_OK;
  hipLaunchKernelGGL(k_whiten_cast, dim3(capped_grid(N, 256, 4096)), dim3(256), 0, (hipStream_t)stream, adv, N, mean, std + eps, out32);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

int mjx_policy_forward(mjx_ctx* c, const float* obs, int64_t N, const float* theta, const float* tr, float* mean_out, void* stream) {
  if (!c || N < 0 || (N > 0 && (!obs || !theta || !mean_out))) return fail(MJX_ERR_ARG, "bad arguments");
  if (N == 0) return MJX_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = c->lw.ensure_rows(N)) return fail(rc, "layer-wise workspace allocation failed");
  HIPCHK(c->lw.forward_scratch(theta, tr ? tr : c->ident_tr, obs, N, mean_out, (hipStream_t)stream));
  return MJX_OK;
}

int mjx_policy_fit_route(int n, int m, const int* hidden, int n_hidden, int B, int loss, int old_tracks_new, int32_t* out2) {
  if (!out2 || n <= 0 || m <= 0 || n_hidden < 0 || (n_hidden && !hidden) || B <= 0 || loss < 0 || loss > 2) return fail(MJX_ERR_ARG, "bad arguments");
  for (int i = 0; i < n_hidden; ++i) if (hidden[i] <= 0) return fail(MJX_ERR_ARG, "bad hidden size");
  const PolicyFitRoute r = policy_fit_route(n, m, std::vector<int>(hidden, hidden + n_hidden), B, loss, old_tracks_new, env_flag("MJX_NO_POLICY_FIT", false));
  out2[0] = r.H; out2[1] = (int32_t)r.bytes;
  return MJX_OK;
}

int mjx_policy_minibatch_adam(mjx_ctx* c, int loss, const float* obs, const float* act, const float* adv, const int32_t* idx,
                              int64_t steps, int B, float* theta, const float* tr, const float* theta_old, const float* tr_old,
                              int old_tracks_new, float* adam_m, float* adam_v, int64_t step0, float lr, float clip,
                              double* loss_trace, void* stream) {
  if (!c || loss < 0 || loss > 2 || steps < 0 || B <= 0 || step0 < 0) return fail(MJX_ERR_ARG, "bad arguments");
  if (steps == 0) return MJX_OK;
  if (!obs || !act || !idx || !theta || !adam_m || !adam_v) return fail(MJX_ERR_ARG, "null buffer");
  if (loss == 2 && (!adv || !theta_old)) return fail(MJX_ERR_ARG, "PPO needs advantages and the old parameters");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(c->device));
  const float* trn0 = tr ? tr : c->ident_tr;
  const float* tro0 = tr_old ? tr_old : c->ident_tr;
  const PolicyFitRoute r = policy_fit_route(c->n, c->m, c->hidden, B, loss, old_tracks_new, env_flag("MJX_NO_POLICY_FIT", false));   // (read per call)
  if (r.H) {
    PolicyFitArgs a{obs, act, adv, idx, steps, B, c->n, c->m, theta, theta_old, trn0, tro0, loss, old_tracks_new, adam_m, adam_v,
                    step0, lr, clip, loss_trace, (int)(r.bytes / 4)};
    void (*k)(PolicyFitArgs) = (r.H == 64) ? k_policy_fit<64> : k_policy_fit<32>;
    if (int rc = lds_limit((const void*)k, r.bytes)) return rc;
    hipLaunchKernelGGL(k, dim3(1), dim3(PFIT_THREADS), r.bytes, st, a);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  MinibatchWS& w = c->lwmb;
  if (int rc = w.reserve(B)) return fail(rc, "minibatch workspace allocation failed");
  const float *trn = trn0, *tro = tro0;
  const int64_t cnt = (loss == 0) ? (int64_t)c->oS : c->d;       // MSE: log_std has no gradient -> untouched (like torch's grad None)
  const unsigned ggrid = capped_grid(B * (c->n > c->m ? c->n : c->m), 256, 1024);
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

}  // extern "C"

// ---- host side of rollout ingestion: csrc/host_ingest.h (plain C++; also built under ASan / TSan by tests/c/host_san.cpp)
namespace {
inline bool mjx_hi_set_device(int idx) { return hipSetDevice(idx) == hipSuccess; }
inline int mjx_hi_h2d_async(void* dst, const void* src, size_t bytes, void* stream, const char** what) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) { *what = hipGetErrorString(e); return (int)e; }
  return 0;
}
}  // namespace
extern "C" int mjx_cast_f64_f32(const double* x, int64_t count, float* out32, void* stream);
namespace {
// reads a page-locked HOST block (device-mapped) and writes it to the device twice: as it is, and as fp32 (host_ingest.h: small raw blocks)
__global__ void k_pull_f64(const double* __restrict__ host, int64_t n, double* __restrict__ raw, float* __restrict__ o32) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = host[i];
    raw[i] = v; o32[i] = (float)v;
  }
}
inline int mjx_hi_pull_f64(const double* host, int64_t n, double* raw, float* o32, void* stream) {
  if (n <= 0) return MJX_OK;
  hipLaunchKernelGGL(k_pull_f64, dim3(capped_grid(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, host, n, raw, o32);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}
}  // namespace
#define MJX_HI_PULL_F64(x, n, r, o, st) mjx_hi_pull_f64(x, n, r, o, st)
#define MJX_HI_SET_DEVICE(i) mjx_hi_set_device(i)
#define MJX_HI_H2D_ASYNC(d, s_, b, st, w) mjx_hi_h2d_async(d, s_, b, st, w)
#define MJX_HI_CAST_F64_F32(x, n, o, st) mjx_cast_f64_f32(x, n, o, st)
#include "host_ingest.h"

extern "C" {

int mjx_cast_f64_f32(const double* x, int64_t count, float* out32, void* stream) {
  if (!x || !out32 || count < 0) return fail(MJX_ERR_ARG, "bad arguments");
  if (count == 0) return MJX_OK;
  hipLaunchKernelGGL(k_cast_f64_f32, dim3(capped_grid(count, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, count, out32);
  HIPCHK(hipGetLastError());
  return MJX_OK;
}

}  // extern "C"
