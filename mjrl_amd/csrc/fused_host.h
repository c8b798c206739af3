// fused_host.h -- host side of the fused policy kernels (fused_policy.h): the table of their instances and FusedWS, the owner of the fused
// path's buffers, caches and validity flags (the counterpart of LayerwiseWS, layerwise.h).  Included by mjx.hip after fail / HIPCHK / lds_limit
// and after fused_policy.h (FusedWS::launch takes the address of k_fused); everything else it shares with the kernel is fused_layout.h.
#pragma once
#include "fused_layout.h"

namespace mjx {

// ---- the instances, in pick order: X(variant id, H1, H2, NT1, MP, NPC).  H1 x H2 = hidden widths, NT1 = 32-column blocks of the
// first layer, MP = padded action count, NPC = compile-time feature count (observations + the ones column, padded to 4; 0 = any,
// read at run time).  Variant 6 is the Adroit class: 39-46 observations, 24-30 actions, 32 x 32 (hand_dapg).  The NPC entries
// specialise variant 1 (first layer fully unrolled): 20 = 16..19 observations (HalfCheetah 17), 12 = 8..11 (Hopper 11, Reacher 11,
// Swimmer 8), 8 = 4..7 (InvertedPendulum 4, point_mass 6).  A debug instance (k_fused<..., DBG = true>) exists for the generic
// variant 1 only, and not in the timing build (MJX_PHASE_CLOCK), whose stamps go to the debug buffer of the production kernels:
// that build differs here and nowhere else.
#define MJX_FUSED_INSTANCES(X)                                                                                                     \
  X(1, 64, 64, 1, 8, 0) X(2, 32, 32, 1, 8, 0) X(3, 64, 64, 1, 16, 0) X(4, 32, 32, 1, 16, 0) X(5, 32, 32, 2, 8, 0) X(6, 32, 32, 2, 32, 0) \
  X(1, 64, 64, 1, 8, 20) X(1, 64, 64, 1, 8, 12) X(1, 64, 64, 1, 8, 8)
#ifdef MJX_PHASE_CLOCK
constexpr bool FUSED_HAS_DBG = false;
#else
constexpr bool FUSED_HAS_DBG = true;
#endif

template <int ID, int H1_, int H2_, int NT1_, int MP_, int NPC_>
struct FusedInst {
  static constexpr int id = ID, H1 = H1_, H2 = H2_, NT1 = NT1_, MP = MP_, NPC = NPC_;
  static constexpr bool has_dbg = FUSED_HAS_DBG && ID == 1 && NPC_ == 0;
  using Layout = FusedLayout<H1_, H2_, NT1_, MP_>;
  using Slab = RawSlab<H1_, H2_, NT1_, MP_, NPC_>;
};
struct FusedKey { int variant, npc, mp; };
#define MJX_X(id, h1, h2, nt1, mp, npc) {id, npc, mp},
constexpr FusedKey FUSED_KEYS[] = {MJX_FUSED_INSTANCES(MJX_X)};
#undef MJX_X
constexpr int fused_max_mp() { int mp = 0; for (const FusedKey& k : FUSED_KEYS) mp = k.mp > mp ? k.mp : mp; return mp; }

// the only switch over the table: f(FusedInst<...>{}) for the instance (variant, npc); false: the table has no such instance
template <class F>
bool with_fused_instance(int variant, int npc, F&& f) {
  switch (variant * 64 + npc) {
#define MJX_X(id, h1, h2, nt1, mp, npc) case id * 64 + npc: f(FusedInst<id, h1, h2, nt1, mp, npc>{}); return true;
    MJX_FUSED_INSTANCES(MJX_X)
#undef MJX_X
  }
  return false;
}

// the end-of-kernel reduction region: four copies of `cols` partial columns + 64 floats, inside a layout of `bytes`
inline bool reduction_fits(int64_t cols, size_t bytes) { return (size_t)(4 * cols + 64) * 4 <= bytes; }

// What serves a shape (arithmetic only): variant 0 = the layer-wise path.  The first generic entry whose layout fits LDS with the
// reduction region of the d parameters; its NPC specialisation where the table has one for this feature count; that instance's
// accumulator-order slab (RawSlab: raw_dr columns, perm = column -> flat index) -- or raw_dr 0, the flat-order epilogue, on any
// doubt about it (a table that does not hit every flat index exactly once, no room for its four copies in LDS).
struct FusedRoute { int variant = 0, npc = 0, raw_dr = 0; size_t bytes = 0; std::vector<int> perm; };
inline FusedRoute fused_route(int n, int m, const std::vector<int>& hid) {
  FusedRoute r;
  if (hid.size() != 2) return r;
  for (const FusedKey& k : FUSED_KEYS) {
    if (k.npc || r.variant) continue;
    with_fused_instance(k.variant, 0, [&](auto inst) {
      using I = decltype(inst);
      if (hid[0] != I::H1 || hid[1] != I::H2 || m > I::MP || n + 1 > 32 * I::NT1) return;
      const size_t bytes = typename I::Layout(n).bytes();
      if (bytes > LDS_MAX || !reduction_fits(FlatOff(n, m, I::H1, I::H2).d, bytes)) return;
      r.variant = I::id; r.bytes = bytes;
    });
  }
  const int NPr = (n + 1 + 3) & ~3;
  for (const FusedKey& k : FUSED_KEYS) if (r.variant && k.variant == r.variant && k.npc == NPr) r.npc = NPr;
  with_fused_instance(r.variant, r.npc, [&](auto inst) {
    using RS = typename decltype(inst)::Slab;
    r.perm.assign(RS::DR, -1);
    if (RS::fill_perm(r.perm.data(), n, m) && reduction_fits(RS::DR, r.bytes)) r.raw_dr = RS::DR;
  });
  return r;
}

// the cached 64 x 64 product on bf16x3 MFMAs and, within it, its W2 gradient (R9); =0: the fp32 kernels (read once per process)
inline bool fvp_bf16x3_on() { static const bool on = env_flag("MJX_FVP_BF16X3", true); return on; }
inline bool fvp_bf16x3_r9_on() { static const bool on = env_flag("MJX_FVP_BF16X3_R9", true); return on; }

struct FusedWS {
  int variant = 0, npc = 0;        // the instance that serves this context (variant 0: none, the layer-wise path does)
  int grid = 256;                  // workgroups per launch: one per CU (K3 with up to 8 actions: two)
  int n = 0, m = 0, oS = 0; int64_t d = 0;
  float* partials = nullptr;       // [grid][max(d, raw_dr)]
  double* spartials = nullptr;     // [2 * grid][4]
  int raw_dr = 0; int* raw_perm = nullptr;   // > 0: workgroup partials in accumulator order + the column -> flat index table (RawSlab)
  // What K1 at old == new leaves for the rest of the update.  Two rules keep it honest:
  //   on_batch():  a new batch drops all three -- activations, observation image, old-policy outputs;
  //   on_policy(): new parameters drop the activations; the image (K3 checks its transform against the snapshot) and the
  //                old policy's outputs (K3 compares the snapshot, or the caller vouches for it) stay.
  int use_hcache = 1;              // MJX_NO_HCACHE=1: no caches at all
  float* hcache = nullptr; size_t hcache_bytes = 0, hc_tile = 0;   // per 32-sample tile (hc_tile floats): h1, h2 | normalised observations
  bool acts_ok = false, ximg_ok = false; const float* hcache_obs = nullptr; int64_t hcache_rows = 0;
  float* ocache = nullptr; size_t ocache_bytes = 0;                // old-policy outputs of the batch (K1 -> K3) ...
  float* snap = nullptr; size_t snap_bytes = 0;                    // ... and the parameters + transforms they were computed with
  bool ocache_ok = false; int64_t ocache_rows = 0;
  unsigned fvp_seq = 0;            // products since the cache was filled / the last solve began: alternate sweep direction

  // MJX_NO_HCACHE and MJX_RAW_SLAB (=0: flat-order partials, A/B) are read here, once per context
  int init(int n_, int m_, int64_t d_, int oS_, const std::vector<int>& hidden, int n_cu, bool layerwise_only) {
    n = n_; m = m_; d = d_; oS = oS_; grid = n_cu;
    const FusedRoute r = fused_route(n, m, hidden);
    if (!layerwise_only) { variant = r.variant; npc = r.npc; }
    if (env_flag("MJX_NO_HCACHE", false)) use_hcache = 0;
    with_fused_instance(variant, npc, [&](auto inst) {
      using L = typename decltype(inst)::Layout;
      hc_tile = (size_t)L::hc_tile(L(n).NP);
    });
    if (variant && r.raw_dr > 0 && env_flag("MJX_RAW_SLAB", true)) {
      HIPCHK(hipMalloc((void**)&raw_perm, (size_t)r.raw_dr * sizeof(int)));
      HIPCHK(hipMemcpy(raw_perm, r.perm.data(), (size_t)r.raw_dr * sizeof(int), hipMemcpyHostToDevice));
      raw_dr = r.raw_dr;
    }
    HIPCHK(hipMalloc(&partials, (size_t)grid * (size_t)(raw_dr > d ? raw_dr : d) * sizeof(float)));
    HIPCHK(hipMalloc(&spartials, spartials_bytes()));
    return MJX_OK;
  }
  size_t spartials_bytes() const { return (size_t)2 * grid * 4 * sizeof(double); }
  void release() { hipFree(hcache); hipFree(ocache); hipFree(snap); hipFree(partials); hipFree(spartials); hipFree(raw_perm); }
  void on_batch() { acts_ok = ximg_ok = ocache_ok = false; }
  void on_policy() { acts_ok = false; }
  void on_solve() { fvp_seq = 0; }   // every solve walks the cache in the same sequence of directions (reproducible bits)
  void info(int32_t* out4) const { out4[0] = variant; out4[1] = variant ? npc : 0; out4[2] = variant ? raw_dr : 0; out4[3] = variant ? grid : 0; }

  // ---- a debug buffer selects the generic instance of the variant (the only one with a debug build), whose accumulator order is
  // not the picked instance's: flat-order partials then.  The debug build covers K1 and the recompute product; a cached product
  // under a debug buffer runs as a recompute one, K3 runs the production kernel of the generic instance.
  static bool dbg_generic(const FusedArgs& a) { return FUSED_HAS_DBG && a.dbg != nullptr; }
  // the caller's bound inputs (mjx.hip bound_args) + this workspace
  FusedArgs complete(FusedArgs a) const { a.partials = partials; a.spartials = spartials; a.raw_dr = dbg_generic(a) ? 0 : raw_dr; return a; }
  template <class I, bool DBG>
  int launch(int mode, const FusedArgs& a, hipStream_t st) const {
    constexpr int H1 = I::H1, H2 = I::H2, NT1 = I::NT1, MP = I::MP, NPC = I::NPC;
    using L = typename I::Layout;
    const int nf = NPC ? NPC - 1 : a.n;                // (the layout depends on the run-time observation count: NPC = 0 serves many)
    const bool ev2 = (mode == MODE_EVAL) && MP <= 8;   // small layout, two workgroups per CU (fused_policy.h)
    const bool cached = (mode == MODE_FVP) && a.hcache != nullptr && !DBG;
    // bf16x3: 64 x 64 with up to 8 actions, and only while its layout -- two 24 KB piece images -- fits 160 KB: up to 23 observations
    constexpr bool BF3_OK = H1 == 64 && H2 == 64 && MP == 8;
    const bool bf3 = BF3_OK && cached && fvp_bf16x3_on() && L(nf, false, true).bytes() <= LDS_MAX;
    const size_t bytes = L(nf, ev2, bf3).bytes();
    void (*k)(FusedArgs) = nullptr;
    if (mode == MODE_VPG) k = k_fused<H1, H2, NT1, MP, MODE_VPG, DBG, NPC>;
    else if (mode == MODE_FVP) k = cached ? k_fused<H1, H2, NT1, MP, MODE_FVP, false, NPC, true> : k_fused<H1, H2, NT1, MP, MODE_FVP, DBG, NPC>;
    else k = k_fused<H1, H2, NT1, MP, MODE_EVAL, false, NPC>;
    if constexpr (BF3_OK) {
      if (bf3) k = fvp_bf16x3_r9_on() ? k_fused<H1, H2, NT1, MP, MODE_FVP, false, NPC, true, true, true> : k_fused<H1, H2, NT1, MP, MODE_FVP, false, NPC, true, true>;
    }
    if (int rc = lds_limit((const void*)k, bytes)) return rc;
    hipLaunchKernelGGL(k, dim3(ev2 ? 2 * grid : grid), dim3(256), bytes, st, a);
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  int dispatch(int mode, const FusedArgs& a, hipStream_t st) const {
    const bool dbg = dbg_generic(a);
    int rc = MJX_OK;
    const bool found = with_fused_instance(variant, dbg ? 0 : npc, [&](auto inst) {
      using I = decltype(inst);
      if constexpr (I::has_dbg) { if (dbg) { rc = launch<I, true>(mode, a, st); return; } }
      rc = launch<I, false>(mode, a, st);
    });
    return found ? rc : fail(MJX_ERR_STATE, "no fused variant");
  }
  // the workgroup partials summed into out (product: + the damping-free tail on theta / v / frac); scal_out: K1's 4 sums too, on one
  // extra workgroup of the vector reduction where that kernel serves (d % 4 == 0 or an accumulator-order slab)
  int reduce(const FusedArgs& a, float* out, const float* theta, const float* v, float frac, const PeerPush* pp, double* scal_out,
              int scal_off, hipStream_t st) const {
    if ((d & 3) == 0 || a.raw_dr > 0) {
      const int cols = a.raw_dr > 0 ? a.raw_dr : (int)d;
      hipLaunchKernelGGL(k_reduce_partials4, dim3((cols + 31) / 32 + (scal_out ? 1 : 0)), dim3(256), 0, st, partials, grid, cols, out, theta, v,
                         oS, frac, pp ? *pp : PeerPush{}, scal_out ? ScalTail{spartials, grid, scal_out, scal_off} : ScalTail{nullptr, 0, nullptr, -1},
                         a.raw_dr > 0 ? (const int*)raw_perm : (const int*)nullptr);
    } else {
      hipLaunchKernelGGL(k_reduce_partials, dim3((d + 15) / 16), dim3(256), 0, st, partials, grid, (int)d, out, theta, v, oS, frac);
      if (scal_out) hipLaunchKernelGGL(k_reduce_scalars, dim3(1), dim3(256), 0, st, spartials, grid, scal_out, PeerPush{});
    }
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
  // the caches are optional (the kernels recompute): grow the block to `need` bytes, or drop it where the allocation fails
  template <class T>
  static void grow_or_drop(T** p, size_t* have, size_t need) {
    if (need <= *have) return;
    if (*p) hipFree(*p);
    *p = nullptr; *have = 0;
    if (hipMalloc(p, need) == hipSuccess) *have = need; else (void)hipGetLastError();
  }

  // K1.  At old == new it keeps h1 / h2 and the normalised observations of every sample for the products of this update (theta is
  // fixed during CG), and the old policy's means / log-likelihoods with a snapshot of their parameters for K3 (the kernel writes
  // the snapshot itself).  *old_kept: the ocache now holds the old policy's outputs of the bound rows.
  int surr_vpg(FusedArgs a, float* grad_out, double* scal_out, const PeerPush* pp, int scal_off, hipStream_t st, bool* old_kept) {
    a = complete(a);
    acts_ok = ximg_ok = false; fvp_seq = 0;
    if (use_hcache && a.old_is_new) {
      const size_t tiles = (size_t)((a.N + 31) / 32);
      grow_or_drop(&hcache, &hcache_bytes, tiles * hc_tile * sizeof(float));
      if (hcache) { a.hcache = hcache; acts_ok = ximg_ok = true; hcache_obs = a.obs; hcache_rows = a.N; }
      grow_or_drop(&ocache, &ocache_bytes, tiles * oc_tile(fused_max_mp()) * sizeof(float));     // any instance
      grow_or_drop(&snap, &snap_bytes, (size_t)snap_len(d, n, m) * sizeof(float));
      ocache_ok = false;
      if (ocache && snap) { a.snap_out = snap; a.ocache = ocache; ocache_ok = true; ocache_rows = a.N; }
    }
    *old_kept = a.old_is_new != 0 && a.ocache != nullptr;
    if (int rc = dispatch(MODE_VPG, a, st)) return rc;
    return reduce(a, grad_out, nullptr, nullptr, 0.f, pp, scal_out, scal_off, st);
  }
  // The Fisher-vector product (a.thetaB = v); after_product() runs between the product and its reduction (profiling events).  K1 filled
  // the cache front to back, so the first product of a solve starts at the back, the next at the front, ...: the lines the previous sweep
  // touched last are the ones the memory-side cache most likely still holds (the 592 MB image does not fit).  MJX_FVP_SWEEP: read per launch.
  template <class F>
  int fvp(FusedArgs a, float* out, float frac, const PeerPush* pp, hipStream_t st, F&& after_product) {
    a = complete(a);
    if (acts_ok && a.N <= hcache_rows) a.hcache = hcache;
    const bool sweep_on = env_flag("MJX_FVP_SWEEP", true);
    a.reverse = (a.hcache && sweep_on) ? (int)((fvp_seq++ & 1u) ^ 1u) : 0;
    if (int rc = dispatch(MODE_FVP, a, st)) return rc;
    if (int rc = after_product()) return rc;
    return reduce(a, out, a.thetaA, a.thetaB, frac, pp, nullptr, -1, st);
  }
  // K3.  old_trusted: the caller vouches that the snapshot still holds (the compare in the kernel's prologue is skipped).  K1's
  // normalised-observation image of this batch (same rows, same observations; the kernel checks the input transform against the
  // snapshot before it trusts it) spares K3 the staging and normalisation of the raw observations.  MJX_K3_XIMG: read per launch.
  int eval(FusedArgs a, double* scal_out, const PeerPush* pp, bool old_trusted, hipStream_t st) {
    a = complete(a);
    if (ocache_ok && a.N <= ocache_rows) { a.ocache = ocache; a.snap = snap; a.snap_trusted = old_trusted ? 1 : 0; }
    const bool ximg_on = env_flag("MJX_K3_XIMG", true);
    if (ximg_on && a.ocache && ximg_ok && hcache && a.N <= hcache_rows && a.obs == hcache_obs) a.hcache = hcache;
    if (int rc = dispatch(MODE_EVAL, a, st)) return rc;
    hipLaunchKernelGGL(k_reduce_scalars, dim3(1), dim3(256), 0, st, spartials, 2 * grid, scal_out, pp ? *pp : PeerPush{});
    HIPCHK(hipGetLastError());
    return MJX_OK;
  }
};

}  // namespace mjx
