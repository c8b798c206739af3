// update_host.h -- host side of the update path: K1, the CG solve, the step and K3 as mjx_npg_update / mjx_trpo_update /
// mjx_dapg_update enqueue them.  Four owners: Transport (who sums over the ranks: none, RCCL, the hook or the peer exchange),
// CgWS (the solve's vectors and every launch of its kernels), ProfBrackets (the event pairs of mjx_profile_*), and the solve
// and the one-call updates themselves.  The rules that decide a route -- cg_route, peer_folds, ProfPick -- are plain C++ on top
// (tests/c/update_host.cpp checks them against a table without a GPU; the peer buffer's layout: peer_layout.h); the rest needs
// the HIP compiler and is included by mjx.hip beside fused_host.h, after fail / HIPCHK.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "peer_layout.h"

namespace mjx {

// ---- routes
// The CG vector update (vecops.h): up to CG_REG_MAX parameters one workgroup holds every element in registers (k_cg_step_reg<8>:
// 8 elements per thread x 1024 threads) -- the only arm that can take the Fisher-vector product as one slot per rank and fold
// what follows the solve into its last launch; beyond, three launches of CGM_G workgroups, or (MJX_CG_MULTI=0) the looping
// single-workgroup kernel.
constexpr int64_t CG_REG_MAX = 8 * 1024;
enum CgRoute { CG_REG, CG_MULTI, CG_LOOP };
inline CgRoute cg_route(int64_t d, bool multi) { return d <= CG_REG_MAX ? CG_REG : multi ? CG_MULTI : CG_LOOP; }

enum TransportKind { TP_NONE, TP_RCCL, TP_HOOK, TP_PEER };
// d-float vectors the peer exchange folds into the loop's own kernels (k_reduce_partials4 / k_cg_step_reg<8, W>): the producer
// side needs the fused path's vectorised reduction (d % 4 == 0), the consumer side the register-resident vector update.  Every
// rank of a job answers alike: the condition depends on the architecture and the transport only.
inline bool peer_folds(TransportKind kind, bool fused, int64_t d) { return kind == TP_PEER && fused && (d & 3) == 0 && d <= CG_REG_MAX; }

// ---- which launches mjx_profile_enable brackets.  enable(k): every k-th Fisher-vector PRODUCT (the bracket closes behind the
// product itself: the fused path's reduction of the partials stays outside it); enable(-k): every k-th CG ITERATION as a whole
// (product, reduction / exchange, vector update) -- except a solve's last one, whose kernel may carry the step; enable(0): off,
// what was recorded stays readable.  PAIRS brackets at the most; any enable(+-k) starts over.
struct ProfPick {
  static constexpr size_t PAIRS = 2048;
  enum Kind { PRODUCT, ITERATION };
  bool on = false, iter = false;
  size_t stride = 1, seen = 0, used = 0;       // launches of the enabled kind that came by; pairs recorded
  void enable(int k) {
    on = k != 0; iter = k < 0;
    if (k) { used = seen = 0; stride = (size_t)(k < 0 ? -(int64_t)k : k); }
  }
  // the pair that brackets this launch, or -1; close() after its second event is recorded
  int pick(Kind kind, bool last_iteration) {
    if (!on || iter != (kind == ITERATION) || (kind == ITERATION && last_iteration)) return -1;
    if (seen++ % stride != 0 || used >= PAIRS) return -1;
    return (int)used;
  }
  void close() { ++used; }
};

}  // namespace mjx

#ifdef __HIPCC__

namespace mjx {

// f(integral_constant<W>) with the compile-time rank count of the folded kernels that covers `world`: 2, 4, 8 or 16
template <class F>
void with_world_width(int world, F&& f) {
  if (world <= 2) f(std::integral_constant<int, 2>{}); else if (world <= 4) f(std::integral_constant<int, 4>{});
  else if (world <= 8) f(std::integral_constant<int, 8>{}); else f(std::integral_constant<int, 16>{});
}

// ---------------------------------------------------------------------------- Transport
// the next exchange: its number, this rank's slot in the own buffer, the producer's and the consumer's view of it
struct PeerRound { uint32_t seq; char* own; PeerPush push; PeerSlots slots; };

// Who sums a buffer over the ranks.  The entries attach one at a time (engine.py tears one down before it tries the next); where
// more than one is present, kind() names the one that serves: the peer exchange once connected, else RCCL, else the hook.
struct Transport {
  int device = 0; int64_t d = 0;
  unsigned* ticket = nullptr;        // the producer kernels' workgroup ticket (CgWS owns it)
  void* comm = nullptr;              // RCCL communicator (one process per GPU)
  mjx_reduce_fn hook = nullptr; void* hook_user = nullptr;   // transport hook in its place (tests)
  // peer exchange (mjx_peer_*): one uncached device buffer per rank (PeerLayout), the peers' mapped through HIP IPC
  struct Peer {
    bool on = false, loopback = false; int rank = 0, world = 0;
    char* buf = nullptr; char* map[PEER_MAX_WORLD] = {nullptr};
    uint32_t seq = 0;
    unsigned long long timeout_ticks = 500000000ull;   // 100 MHz ticks a consumer waits for a peer (MJX_PEER_TIMEOUT_MS; default 5 s)
    int fault = 0;                                     // MJX_PEER_FAULT (tests): 1 = "slot", 2 = "flag" (peer_layout.h peer_push_view)
  } peer;
  int world_ = 0;                    // of the transport attached last (the peer exchange's rank: peer.rank)

  void init(int device_, int64_t d_, unsigned* ticket_) { device = device_; d = d_; ticket = ticket_; }
  TransportKind kind() const { return peer.on ? TP_PEER : comm ? TP_RCCL : hook ? TP_HOOK : TP_NONE; }
  bool attached() const { return kind() != TP_NONE; }
  int world() const { return attached() ? world_ : 0; }
  PeerLayout layout() const { return PeerLayout{d, peer.world}; }
  int scal_off() const { return (int)layout().scal_off(); }   // where the 4 doubles that travel with a gradient sit in a slot

  int attach_rccl(int rank, int world, const char* id_host) {
    if (comm) return fail(MJX_ERR_STATE, "a communicator is already attached");
    RcclApi& r = rccl();
    if (!r.load()) return fail(MJX_ERR_UNSUPPORTED, "%s", r.error.c_str());
    HIPCHK(hipSetDevice(device));
    RcclApi::UniqueId id;
    memcpy(id.internal, id_host, MJX_COMM_ID_BYTES);
    RcclApi::Comm cm = nullptr;
    if (int rc = r.CommInitRank(&cm, world, id, rank)) return fail(1000 + rc, "ncclCommInitRank: %s", r.GetErrorString(rc));
    comm = cm; world_ = world;
    return MJX_OK;
  }
  int attach_hook(mjx_reduce_fn fn, void* user, int world) {     // fn == NULL: detach it
    if (comm) return fail(MJX_ERR_STATE, "an RCCL communicator is attached");
    hook = fn; hook_user = user; world_ = fn ? world : 0;
    return MJX_OK;
  }
  // MJX_PEER_FAULT, MJX_PEER_FAULT_RANK and MJX_PEER_TIMEOUT_MS are read here, once per exported buffer
  int peer_export(int rank, int world, char* handle_out) {
    if (comm || hook || peer.buf) return fail(MJX_ERR_STATE, "a transport is already attached");
    HIPCHK(hipSetDevice(device));
    const size_t total = PeerLayout{d, world}.total_bytes();
    void* p = nullptr;
    HIPCHK(hipExtMallocWithFlags(&p, total, hipDeviceMallocUncached));
    struct Guard { void* p; ~Guard() { if (p) (void)hipFree(p); } } g{p};
    HIPCHK(hipMemset(p, 0, total));
    HIPCHK(hipDeviceSynchronize());
    hipIpcMemHandle_t h;
    { hipError_t e = hipIpcGetMemHandle(&h, p); if (e != hipSuccess) return fail((int)e, "hipIpcGetMemHandle: %s", hipGetErrorString(e)); }
    static_assert(sizeof(hipIpcMemHandle_t) == MJX_PEER_HANDLE_BYTES, "handle size");
    memcpy(handle_out, &h, sizeof h);
    g.p = nullptr;
    peer.buf = (char*)p; peer.rank = rank; peer.world = world; peer.seq = 0;
    if (const char* f = getenv("MJX_PEER_FAULT")) {
      const char* only = getenv("MJX_PEER_FAULT_RANK");               // (default: every rank misbehaves)
      if (!only || atoi(only) == rank) peer.fault = !strcmp(f, "slot") ? 1 : !strcmp(f, "flag") ? 2 : 0;
    }
    if (const char* ms = getenv("MJX_PEER_TIMEOUT_MS")) {             // how long a consumer kernel waits for a peer's vector
      const double v = atof(ms);
      if (v > 0.0) peer.timeout_ticks = (unsigned long long)(v * 1e5);
    }
    return MJX_OK;
  }
  int peer_connect(const char* handles) {                             // handles == NULL: loop-back rehearsal, every peer is the own buffer
    if (!peer.buf || peer.on) return fail(MJX_ERR_STATE, "call mjx_peer_export first (once)");
    HIPCHK(hipSetDevice(device));
    for (int r = 0; r < peer.world; ++r) {
      if (r == peer.rank || !handles) { peer.map[r] = peer.buf; continue; }
      hipIpcMemHandle_t h;
      memcpy(&h, handles + (size_t)r * MJX_PEER_HANDLE_BYTES, sizeof h);
      void* q = nullptr;
      hipError_t e = hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) return fail((int)e, "hipIpcOpenMemHandle (rank %d): %s", r, hipGetErrorString(e));
      peer.map[r] = (char*)q;
    }
    peer.on = true; peer.loopback = (handles == nullptr);
    world_ = peer.world;
    return MJX_OK;
  }
  // timed-out waits of this rank's consumers since the last call (synchronises: read after the update's own read-back)
  int peer_status(int* timeouts_out) {
    *timeouts_out = 0;
    if (!peer.on) return MJX_OK;
    HIPCHK(hipSetDevice(device));
    unsigned* word = layout().flags(peer.buf) + PeerLayout::TIMEOUTS;
    unsigned n = 0;
    HIPCHK(hipMemcpy(&n, word, sizeof n, hipMemcpyDeviceToHost));
    if (n) HIPCHK(hipMemset(word, 0, sizeof n));
    *timeouts_out = (int)n;
    return MJX_OK;
  }
  // the peer exchange and the communicator go (a half-attached exchange too); the hook is detached by attach_hook(NULL)
  void detach() {
    if (peer.buf) {
      (void)hipSetDevice(device);
      (void)hipDeviceSynchronize();
      for (int r = 0; r < peer.world; ++r)
        if (r != peer.rank && peer.map[r] && peer.map[r] != peer.buf) (void)hipIpcCloseMemHandle(peer.map[r]);
      (void)hipFree(peer.buf);
      peer = Peer{};
      world_ = 0;
    }
    if (comm) {
      (void)hipSetDevice(device);
      (void)hipDeviceSynchronize();
      (void)rccl().CommDestroy(comm);
      comm = nullptr; world_ = 0;
    }
  }

  PeerRound next_round() {
    const PeerLayout L = layout();
    const PeerRoundNo n = peer_next_round(&peer.seq);
    return PeerRound{n.seq, L.slot(peer.buf, n.par, peer.rank),
                     peer_push_view(L, peer.map, peer.rank, n.par, n.seq, peer.loopback, peer.fault, ticket),
                     peer_slots_view(L, peer.buf, peer.rank, n.par, n.seq, peer.timeout_ticks)};
  }
  // buf[0, count) summed over the ranks in place, on the stream (dtype 0: float, 1: double)
  int allreduce(void* buf, int64_t count, int dtype, void* stream) {
    if (count == 0) return MJX_OK;
    switch (kind()) {
      case TP_PEER: {
        hipStream_t st = (hipStream_t)stream;
        const size_t bytes = (size_t)count * (dtype ? 8 : 4), slot = layout().slot_bytes();
        if (bytes > slot) return fail(MJX_ERR_ARG, "peer all-reduce of %zu bytes exceeds the slot (%zu)", bytes, slot);
        const PeerRound r = next_round();
        const unsigned grid = (unsigned)((count + 255) / 256);
        if (dtype) hipLaunchKernelGGL(k_peer_push<double>, dim3(grid), dim3(256), 0, st, (const double*)buf, r.push, count);
        else hipLaunchKernelGGL(k_peer_push<float>, dim3(grid), dim3(256), 0, st, (const float*)buf, r.push, count);
        HIPCHK(hipGetLastError());
        if (dtype) hipLaunchKernelGGL(k_peer_sum<double>, dim3(grid), dim3(256), 0, st, r.slots, (double*)buf, count);
        else hipLaunchKernelGGL(k_peer_sum<float>, dim3(grid), dim3(256), 0, st, r.slots, (float*)buf, count);
        HIPCHK(hipGetLastError());
        return MJX_OK;
      }
      case TP_RCCL: {
        RcclApi& r = rccl();
        if (int rc = r.AllReduce(buf, buf, (size_t)count, dtype ? RcclApi::kFloat64 : RcclApi::kFloat32, RcclApi::kSum, comm, stream))
          return fail(1000 + rc, "ncclAllReduce: %s", r.GetErrorString(rc));
        return MJX_OK;
      }
      case TP_HOOK:
        if (int rc = hook(hook_user, buf, count, dtype, stream)) return fail(rc, "transport hook failed (%d)", rc);
        return MJX_OK;
      case TP_NONE: break;
    }
    return fail(MJX_ERR_STATE, "no communicator attached (mjx_comm_init)");
  }
};

// ---------------------------------------------------------------------------- CgWS
// The solve's state on the device -- x, r, p, z, Ap, the 8 doubles of its scalars (vecops.h) -- and the only launches of
// k_cg_* / k_cgm_*.  The public call-by-call entries (mjx_cg_init / _step / _finish) and the solve below use the same four.
static_assert(CG_REG_MAX >= 4 * CGM_G, "k_cgm_*'s 2 x CGM_G fp64 partials live in z: d floats must hold them wherever that arm runs");
struct CgWS {
  int64_t d = 0;
  float *x = nullptr, *r = nullptr, *p = nullptr, *z = nullptr, *Ap = nullptr;
  double* scal = nullptr;
  unsigned* ticket = nullptr;        // workgroup ticket of the producer kernels (ordinary device memory, zero between launches)

  int alloc(int64_t d_) {
    d = d_;
    HIPCHK(hipMalloc(&x, d * 4)); HIPCHK(hipMalloc(&r, d * 4)); HIPCHK(hipMalloc(&p, d * 4));
    HIPCHK(hipMalloc(&z, d * 4)); HIPCHK(hipMalloc(&Ap, d * 4));
    HIPCHK(hipMalloc((void**)&ticket, 256)); HIPCHK(hipMemset(ticket, 0, 256));
    HIPCHK(hipMalloc(&scal, 8 * sizeof(double)));
    return MJX_OK;
  }
  void release() { hipFree(x); hipFree(r); hipFree(p); hipFree(z); hipFree(Ap); hipFree(ticket); hipFree(scal); }
  static bool multi_on() { static const bool on = env_flag("MJX_CG_MULTI", true); return on; }   // read once per process, by the first step beyond CG_REG_MAX

  int init(const float* b, hipStream_t st) {
    hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(1024), 0, st, b, x, r, p, scal, (int)d);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  // the right-hand side arrives as one slot per rank (the gradient's peer exchange, K1's 4 sums riding along at scal_off): one
  // kernel waits, sums, leaves the summed gradient in `b` and the sums in s4_out, and starts the solve
  int init_from_slots(const PeerSlots& slots, int scal_off, float* b, double* s4_out, hipStream_t st) {
    with_world_width(slots.world, [&](auto w) {
      hipLaunchKernelGGL((k_cg_init_w<decltype(w)::value>), dim3(1), dim3(1024), 0, st, slots, scal_off, b, s4_out, x, r, p, scal, (int)d);
    });
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  // one vector update with the product in Ap_, or (slots, CG_REG only) in one slot per rank, waited for and summed by the
  // kernel; fin (CG_REG only): what follows a solve's last update, in the same launch
  int step(const float* Ap_, const PeerSlots* slots, const CgFin& fin, float damping, double tol, hipStream_t st) {
    if (slots) {
      with_world_width(slots->world, [&](auto w) {
        hipLaunchKernelGGL((k_cg_step_reg<8, decltype(w)::value>), dim3(1), dim3(1024), 0, st, (const float*)nullptr, damping, tol, x, r, p, scal, (int)d, *slots, fin);
      });
    } else if (d <= CG_REG_MAX) {
      hipLaunchKernelGGL(k_cg_step_reg<8>, dim3(1), dim3(1024), 0, st, Ap_, damping, tol, x, r, p, scal, (int)d, PeerSlots{}, fin);
    } else if (cg_route(d, multi_on()) == CG_MULTI) {
      double* part = (double*)z;       // 2 x CGM_G fp64 partials
      hipLaunchKernelGGL(k_cgm_pz, dim3(CGM_G), dim3(CGM_T), 0, st, Ap_, (const float*)p, damping, (const double*)scal, part, (int)d);
      hipLaunchKernelGGL(k_cgm_xr, dim3(CGM_G), dim3(CGM_T), 0, st, Ap_, (const float*)p, damping, x, r, scal, part, (int)d);
      hipLaunchKernelGGL(k_cgm_p, dim3(CGM_G), dim3(CGM_T), 0, st, (const float*)r, p, tol, scal, (const double*)part, (int)d);
    } else {
      hipLaunchKernelGGL(k_cg_step, dim3(1), dim3(1024), 0, st, Ap_, damping, tol, x, r, p, z, scal, (int)d);
    }
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  int finish(const float* b, float* x_out, double* bdotx_out, hipStream_t st) {
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(1024), 0, st, b, x, x_out, bdotx_out, (int)d);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
};

// ---------------------------------------------------------------------------- ProfBrackets
// ProfPick's brackets as HIP event pairs on the caller's stream (pair i: events 2i, 2i + 1)
struct ProfBrackets : ProfPick {
  std::vector<hipEvent_t> ev;
  int enable(int k) {
    if (k && ev.empty()) {
      ev.resize(2 * PAIRS);
      for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    }
    ProfPick::enable(k);
    return MJX_OK;
  }
  void release() { for (auto& e : ev) hipEventDestroy(e); ev.clear(); }
  // *pair = the bracket opened in front of this launch, or -1 (end(-1) does nothing)
  int begin(Kind kind, bool last_iteration, hipStream_t st, int* pair) {
    *pair = pick(kind, last_iteration);
    if (*pair >= 0) HIPCHK(hipEventRecord(ev[2 * *pair], st));
    return MJX_OK;
  }
  int end(int pair, hipStream_t st) {
    if (pair < 0) return MJX_OK;
    HIPCHK(hipEventRecord(ev[2 * pair + 1], st));
    close();
    return MJX_OK;
  }
  int elapsed(size_t i, double* ms_out) {            // waits for bracket i < used to close on the device
    HIPCHK(hipEventSynchronize(ev[2 * i + 1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
    *ms_out = (double)ms;
    return MJX_OK;
  }
};

}  // namespace mjx

// ---------------------------------------------------------------------------- the context
// The shape, the bound inputs and the owners.  (Defined here and not in mjx.hip because the solve and the updates below need it.)
struct mjx_ctx {
  int device = 0;
  int n = 0, m = 0;
  std::vector<int> hidden;
  int64_t d = 0;
  int oS = 0;                      // offset of log_std in the flat vector
  // bound inputs
  const float *obs = nullptr, *act = nullptr, *adv = nullptr;
  int64_t N_local = 0, N_global = 0;
  const float *theta_new = nullptr, *theta_old = nullptr, *tr_new = nullptr, *tr_old = nullptr;
  int old_is_new = 1;
  bool batch_bound = false;
  int64_t rows_bound = 0;                             // rows handed to the last mjx_bind_batch
  float* ident_tr = nullptr;       // identity transforms (device)
  float* dbg = nullptr;
  long long* clk = nullptr;        // launch clock stamps (mjx_set_clock_buffer)
  bool lw_old_ok = false;          // K1's outputs are the OLD policy's (old == new at K1; theta_old, its transform and the batch untouched since by this
                                   // library): set by mjx_surr_vpg, cleared by the public binding calls, consumed by the one-call updates' evaluations
                                   // (layer-wise path: reuse of the output block; fused path: the snapshot compare of K3's prologue is skipped)
  mjx::FusedWS fz;                 // fused path workspace (fz.variant != 0: it serves this context)
  mjx::LayerwiseWS lw;             // layer-wise path workspace
  mjx::MinibatchWS lwmb;           // launch-based minibatch trainer's workspace (mjx_policy_minibatch_adam)
  mjx::CgWS cg;                    // the solve's vectors and launches
  mjx::Transport tp;               // rank sums
  mjx::ProfBrackets prof;          // mjx_profile_*
};

namespace {

using namespace mjx;

// the kernel launches and the binding of mjx.hip that the solve and the updates drive.  pp (peer exchange): the launch's reduction
// kernel writes this rank's slot into every peer's buffer and raises the flags; the output pointer IS the own slot then.
int check_bound(mjx_ctx* c, bool need_act);
int surr_vpg_impl(mjx_ctx* c, float* grad_out, double* scal_out, void* stream, const PeerPush* pp, int scal_off);
int fvp_impl(mjx_ctx* c, const float* v, float* out, void* stream, const PeerPush* pp);
int eval_impl(mjx_ctx* c, double* scal_out, void* stream, const PeerPush* pp, bool old_ok);
int bind_policy_impl(mjx_ctx* c, const float* theta_new, const float* theta_old, const float* tr_new, const float* tr_old, int old_is_new,
                     bool keep_old_outputs);

// ---------------------------------------------------------------------------- the solve
// b: the right-hand side, or (b_slots) where its rank sum is left, with K1's summed scalars to s4_out.  allreduce / user:
// mjx_cg_solve's caller-supplied rank sum in place of the context's transport.  fin: what follows the last vector update
// (fin_only / fin_step); the solve fills in b, x_out, bdotx and oS.
struct SolveReq {
  float* b; int iters; float damping; double tol; float* x_out; double* bdotx_out;
  CgFin fin; void* stream;
  mjx_allreduce_fn allreduce = nullptr; void* user = nullptr;
  const PeerSlots* b_slots = nullptr; double* s4_out = nullptr;
};
CgFin fin_only() { CgFin f; f.mode = 1; return f; }
CgFin fin_step(const float* theta, float* theta_out, double* alpha_out, double step_size, double const_alpha, float min_log_std) {
  CgFin f;
  f.mode = std::isnan(const_alpha) ? 2 : 3;
  f.theta = theta; f.theta_out = theta_out; f.alpha_out = alpha_out; f.step_size = step_size;
  f.const_alpha = std::isnan(const_alpha) ? 0.f : (float)const_alpha; f.min_log_std = min_log_std;
  return f;
}

// One iteration: product, rank sum, vector update (with `f` in its launch).  fold: the peer exchange rides on the loop's own
// kernels -- the product's reduction kernel writes this rank's vector into slot `rank` of EVERY rank's buffer and raises its
// arrival flags, the vector-update kernel waits on the own flags and sums its local slots (rank order): exactly the launches of
// the one-rank loop, no host round trip.  (A rank on another route -- empty shard -- runs the same exchange through allreduce.)
int cg_iteration(mjx_ctx* c, const SolveReq& q, bool fold, const CgFin& f) {
  hipStream_t st = (hipStream_t)q.stream;
  if (fold) {
    const PeerRound r = c->tp.next_round();
    if (int rc = fvp_impl(c, c->cg.p, (float*)r.own, q.stream, &r.push)) return rc;
    return c->cg.step(nullptr, &r.slots, f, q.damping, q.tol, st);
  }
  if (int rc = fvp_impl(c, c->cg.p, c->cg.Ap, q.stream, nullptr)) return rc;
  if (q.allreduce) { if (int rc = q.allreduce(q.user, c->cg.Ap, c->d, q.stream)) return fail(rc, "allreduce callback failed (%d)", rc); }
  else if (c->tp.attached()) { if (int rc = c->tp.allreduce(c->cg.Ap, c->d, 0, q.stream)) return rc; }
  return c->cg.step(c->cg.Ap, nullptr, f, q.damping, q.tol, st);
}

// The solve, with (r06) what precedes and follows it folded into its own launches when the shapes allow: the gradient's rank sum
// into its first kernel (b_slots), and after the LAST vector update b.x, x_out and (fin mode 2 / 3) the stepped parameters in that
// update's kernel -- k_cg_finish and k_apply_*_step are not launched (CG_REG and at least one iteration; otherwise they are).
int cg_solve_impl(mjx_ctx* c, const SolveReq& q) {
  hipStream_t st = (hipStream_t)q.stream;
  c->fz.on_solve();
  if (int rc = q.b_slots ? c->cg.init_from_slots(*q.b_slots, c->tp.scal_off(), q.b, q.s4_out, st) : c->cg.init(q.b, st)) return rc;
  const bool reg = cg_route(c->d, false) == CG_REG;
  const bool fold = !q.allreduce && peer_folds(c->tp.kind(), c->fz.variant != 0, c->d) && c->old_is_new && c->N_local > 0;
  CgFin fin = q.fin;
  fin.b = q.b; fin.x_out = q.x_out; fin.bdotx = q.bdotx_out; fin.oS = c->oS;
  bool fin_done = false;
  for (int i = 0; i < q.iters; ++i) {
    const bool last = i == q.iters - 1;
    const CgFin f = (reg && last) ? fin : CgFin{};
    int pair;
    if (int rc = c->prof.begin(ProfPick::ITERATION, last, st, &pair)) return rc;
    const int rc = cg_iteration(c, q, fold, f);
    (void)c->prof.end(pair, st);
    if (rc) return rc;
    fin_done = f.mode != 0;
  }
  if (fin_done) return MJX_OK;
  if (int rc = c->cg.finish(q.b, q.x_out, q.bdotx_out, st)) return rc;
  if (fin.mode == 2) return mjx_apply_npg_step(c, fin.theta, q.x_out, q.bdotx_out, fin.step_size, fin.min_log_std, fin.theta_out, fin.alpha_out, q.stream);
  if (fin.mode == 3) return mjx_apply_step(c, fin.theta, q.x_out, fin.const_alpha, fin.min_log_std, fin.theta_out, q.stream);
  return MJX_OK;
}

// ---------------------------------------------------------------------------- the updates
// K1 and the rank sums of its outputs, up to the point where the solve starts.  *folded: the gradient's sum is left to the
// solve's first kernel, *slots_out is what it reads (peer exchange, folded: ONE exchange carries the gradient and K1's sums)
int vpg_and_rank_sums(mjx_ctx* c, float* grad_out, double* s4, void* stream, PeerSlots* slots_out, bool* folded) {
  *folded = false;
  hipStream_t st = (hipStream_t)stream;
  if (peer_folds(c->tp.kind(), c->fz.variant != 0, c->d)) {
    const PeerRound r = c->tp.next_round();
    const int off = c->tp.scal_off();
    if (c->N_local > 0) {
      if (int rc = surr_vpg_impl(c, (float*)r.own, (double*)(r.own + off), stream, &r.push, off)) return rc;
    } else {                                     // a rank without samples: zeros, through the same exchange
      HIPCHK(hipMemsetAsync(grad_out, 0, c->d * sizeof(float), st));
      HIPCHK(hipMemsetAsync(s4, 0, 4 * sizeof(double), st));
      hipLaunchKernelGGL(k_peer_push_vs, dim3((unsigned)((c->d + 255) / 256)), dim3(256), 0, st, (const float*)grad_out, (const double*)s4, r.push, (int)c->d, off);
      HIPCHK(hipGetLastError());
    }
    *slots_out = r.slots;
    *folded = true;
    return MJX_OK;
  }
  if (int rc = surr_vpg_impl(c, grad_out, s4, stream, nullptr, -1)) return rc;
  if (c->tp.kind() == TP_RCCL) {
    RcclApi& r = rccl();
    (void)r.GroupStart();                       // one launch for the gradient and its scalars
    int rc = c->tp.allreduce(grad_out, c->d, 0, stream);
    if (!rc) rc = c->tp.allreduce(s4, 4, 1, stream);
    const int ge = r.GroupEnd();
    if (rc) return rc;
    if (ge) return fail(1000 + ge, "ncclGroupEnd: %s", r.GetErrorString(ge));
  } else if (c->tp.attached()) {
    if (int rc = c->tp.allreduce(grad_out, c->d, 0, stream)) return rc;
    if (int rc = c->tp.allreduce(s4, 4, 1, stream)) return rc;
  }
  return MJX_OK;
}

// K3 and the rank sum of its 4 doubles (peer exchange: the push rides on the reduction kernel).  The evaluations of the one-call
// updates may use the old policy's outputs K1 left -- nothing outside the library ran in between.
int eval_and_rank_sum(mjx_ctx* c, double* res4, void* stream) {
  if (c->tp.kind() == TP_PEER && c->fz.variant && c->N_local > 0) {
    const PeerRound r = c->tp.next_round();
    if (int rc = eval_impl(c, (double*)r.own, stream, &r.push, true)) return rc;
    hipLaunchKernelGGL(k_peer_sum<double>, dim3(1), dim3(256), 0, (hipStream_t)stream, r.slots, res4, (int64_t)4);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  if (int rc = eval_impl(c, res4, stream, nullptr, true)) return rc;
  if (c->tp.attached()) if (int rc = c->tp.allreduce(res4, 4, 1, stream)) return rc;
  return MJX_OK;
}

// the checks the three one-call updates share, in their order, with the entry's own name in the text
int update_prologue(mjx_ctx* c, const char* entry, bool args_ok, bool from_old_is_new, const float* theta_out) {
  if (int rc = check_bound(c, true)) return rc;
  if (!args_ok) return fail(MJX_ERR_ARG, "bad arguments");
  if (from_old_is_new && !c->old_is_new) return fail(MJX_ERR_STATE, "%s starts from theta_new == theta_old (mjx_bind_policy with old_is_new)", entry);
  if (theta_out == c->theta_old) return fail(MJX_ERR_ARG, "theta_out must not alias theta_old");
  return MJX_OK;
}

// K1, the rank sums and the solve of NPG and of TRPO's first call: the gradient to grad_out, K1's sums to results[4..8), the
// solution to x_out, b.x to results[8]
int vpg_then_solve(mjx_ctx* c, int iters, float damping, double tol, float* grad_out, float* x_out, double* results, const CgFin& fin, void* stream) {
  PeerSlots gs{};
  bool folded = false;
  if (int rc = vpg_and_rank_sums(c, grad_out, results + 4, stream, &gs, &folded)) return rc;
  SolveReq q{grad_out, iters, damping, tol, x_out, results + 8, fin, stream};
  if (folded) { q.b_slots = &gs; q.s4_out = results + 4; }
  return cg_solve_impl(c, q);
}

}  // namespace

#endif  // __HIPCC__
