// lw_launch.h -- the only code that turns a plan of the layer-wise path (lw_plan.h) into kernel launches: the per-device ticket
// ring of the persistent kernel, the dynamic-LDS limits, the one status check per operation, the slots of the timing build, and
// ONE switch from a plan's (BN, NTH) / (LB, EPI) to the template instances.  Callers inside and outside the path use
// lw_launch_gemm and lw_reduce_split.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <utility>

#include "launch_state.h"
#include "lw_gemm.h"
#include "lw_gemm_p.h"
#include "lw_plan.h"

namespace mjx {

// Per-DEVICE state of the layer-wise launchers lives in launch_state.h (function-static flags configured only the
// device that happened to be current at first use -- a second context on another GPU of the same process launched > 64 KB-LDS
// kernels without the attribute and read a foreign device's ticket counter).
inline int* lw_ticket_ring() {                                               // 256 ticket counters (+ leaver counts) on the current device; nullptr if the allocation fails
  static std::mutex mu;
  static PerDevice<std::pair<bool, int*>> rings;                             // (tried, [256 tickets][256 leaver counts], zero between launches)
  std::lock_guard<std::mutex> lk(mu);
  auto& r = rings.here();
  if (!r.first) {
    r.first = true;
    if (hipMalloc(&r.second, 512 * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); r.second = nullptr; }
    else if (hipMemset(r.second, 0, 512 * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(r.second); r.second = nullptr; }
  }
  return r.second;
}
// The GEMM launchers below return nothing; every operation built from them ends with ONE status check, lw_status().  A
// dynamic-LDS limit that could not be set keeps its kernel from being launched and is kept for that check.
inline hipError_t& lw_refused() { static thread_local hipError_t e = hipSuccess; return e; }
inline bool lw_dyn_lds(const void* kern, size_t bytes) {
  const int e = dyn_lds(kern, bytes);
  if (e != 0 && lw_refused() == hipSuccess) lw_refused() = e == LDS_OVER ? hipErrorInvalidValue : (hipError_t)e;
  return e == 0;
}
inline hipError_t lw_status() {                                              // the first refusal since the last check, else the runtime's last error
  const hipError_t refused = lw_refused(), last = hipGetLastError();
  lw_refused() = hipSuccess;
  return refused != hipSuccess ? refused : last;
}

#ifdef MJX_PHASE_CLOCK
// timing build (-DMJX_PHASE_CLOCK, LW_STAMP in lw_gemm.h): mjx_set_debug_buffer hands the buffer over and resets the slot
// counter, each GEMM launch takes the next slot of LW_CLK_SLOT int64
constexpr int LW_CLK_SLOT = 8 + 8 * 16384, LW_CLK_SLOTS = 24;
inline long long*& lw_clk_buf() { static long long* p = nullptr; return p; }
inline int& lw_clk_slot() { static int s = 0; return s; }
inline void lw_clk_take(GemmArgs& h, int64_t workgroups) {
  if (lw_clk_buf() && !h.clk && lw_clk_slot() < LW_CLK_SLOTS && workgroups <= 16384) h.clk = lw_clk_buf() + (int64_t)(lw_clk_slot()++) * LW_CLK_SLOT;
}
#else
inline void lw_clk_take(GemmArgs&, int64_t) {}
#endif

// the instance tables: (BN, NTH) of a tile step, (LB, EPI) of a persistent step
typedef void (*LwTileKernel)(GemmArgs);
typedef void (*LwPersistentKernel)(GemmArgs, int, int, int*);
inline LwTileKernel lw_tile_kernel(int BN, int NTH) {
  switch (BN) {
    case 32: return k_gemm<128, 32, 256>;
    case 64: return k_gemm<128, 64, 256>;
    case 256: return k_gemm<128, 256, 512>;
    default: return NTH == 256 ? k_gemm<128, 128, 256> : k_gemm<128, 128, 512>;
  }
}
inline LwPersistentKernel lw_persistent_kernel(int LB, int epi) {
  if (epi == EPI_BIAS_TANH) return LB ? k_gemm_p<1, EPI_BIAS_TANH, GemmArgs> : k_gemm_p<0, EPI_BIAS_TANH, GemmArgs>;
  if (epi == EPI_TANGENT) return LB ? k_gemm_p<1, EPI_TANGENT, GemmArgs> : k_gemm_p<0, EPI_TANGENT, GemmArgs>;
  return LB ? k_gemm_p<1, EPI_BACK, GemmArgs> : k_gemm_p<0, EPI_BACK, GemmArgs>;
}

// product g over `splits` sample splits (blockIdx.z; the contraction of a weight gradient runs over samples)
// (r04, measured and dropped: handing the row blocks of the last, partial ticket round -- 67 of 3 907 tiles at the configs[3]
//  shard -- to the general kernel as 128 x 128 tiles in a second launch, to halve the tail: 4.39 -> 4.45 ms; the ticket scheme
//  already spreads the remainder, a kernel boundary costs more than the half tile it saves.  profiles/r04_lw/ab_tail_launch.log)
inline void lw_launch_gemm(const GemmArgs& g, int splits, hipStream_t st, const LwSwitches& sw = LwSwitches::read()) {
  // the ticket ring is made at the first product that could run persistent
  const bool has_ring = sw.persist && g.N > 32 && lw_ticket_ring() != nullptr;
  const LwPlan pl = lw_plan_gemm(g, splits, sw, cu_count(), has_ring);
  if (pl.ntile == 0) {
    const LwPersistentKernel kern = lw_persistent_kernel(pl.LB, pl.epi);
    if (!lw_dyn_lds((const void*)kern, pl.lds)) return;
    GemmArgs h = g;
    if (!h.cs_ld) h.cs_ld = h.N;
    // (a ring of counters per device, one per launch in turn: launches on different streams do not share one)
    static std::atomic<unsigned> turn{0};
    int* ticket = lw_ticket_ring() + (turn.fetch_add(1) & 255u);            // (zero: the kernel's last workgroup leaves it so)
    lw_clk_take(h, 0);
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(GP_NTH), pl.lds, st, h, pl.row_tiles, pl.col_blocks, ticket);
    return;
  }
  for (int i = 0; i < pl.ntile; ++i) {
    const LwTileStep& t = pl.tile[i];
    const LwTileKernel kern = lw_tile_kernel(t.BN, t.NTH);
    if (!lw_dyn_lds((const void*)kern, t.lds)) continue;                   // double-buffered operand tiles: dynamic LDS beyond the 64 KB default
    GemmArgs h = lw_col_slice(g, t.j0, t.ncols);
    h.fast = sw.fast ? 1 : 0;
    lw_clk_take(h, (int64_t)t.gx * t.gy);
    hipLaunchKernelGGL(kern, dim3(t.gx, t.gy, t.gz), dim3(t.NTH), t.lds, st, h);
  }
}

// sum of `splits` partial slabs of cnt floats (fixed order, fp64 accumulation)
inline void lw_reduce_split(const float* part, int splits, int64_t cnt, float* out, hipStream_t st, const LwSwitches& sw = LwSwitches::read()) {
  if ((cnt & 3) == 0 && (((uintptr_t)part | (uintptr_t)out) & 15) == 0 && sw.tiles != 0)
    hipLaunchKernelGGL(k_reduce_split4, dim3((unsigned)((cnt / 4 + 63) / 64)), dim3(256), 0, st, part, splits, cnt / 4, out);
  else
    hipLaunchKernelGGL(k_reduce_split, dim3(ew_grid(cnt)), dim3(256), 0, st, part, splits, cnt, out);
}

}  // namespace mjx
