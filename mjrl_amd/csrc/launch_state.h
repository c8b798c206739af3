// launch_state.h -- what the host keeps between kernel launches, in one place: the LDS limits, the dynamic-LDS attribute of
// each kernel, the CU count, and scratch blocks of device memory.  Plain host C++ over the HIP runtime API (no kernels), so that
// tests/c/launch_state_san.cpp can run it against a fake runtime with two devices, under the sanitizers.
//
// What is keyed by what:
//   per DEVICE, process-wide (mutex):  the dynamic-LDS attribute of a kernel (a property of the loaded code object on that
//                                      device, shared by all threads), the CU count, anything held in a locked PerDevice<T>
//   per kernel, process-wide:          its static LDS (the same code object everywhere)
//   per THREAD, then (site, device, stream): scratch blocks.  A block belongs to the thread that fetched it (another thread may
//                                      not grow, i.e. free, it between that thread's fetch and its launch), lies on the device
//                                      that was current, and is used by one stream (two streams never share one block)
// Every function acts on the CURRENT device (hipGetDevice); callers with a context make theirs current first.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace mjx {

// LDS one workgroup can get on gfx950: static + dynamic bytes together; beyond LDS_DEFAULT only after the kernel's
// hipFuncAttributeMaxDynamicSharedMemorySize has been raised on the device it is launched on (dyn_lds)
constexpr size_t LDS_MAX = 160 * 1024, LDS_DEFAULT = 64 * 1024;

// An on / off switch of the environment: "0" turns a default-on switch off, "1" turns a default-off switch on, anything else
// is the default.  WHEN a switch is read (per launch, per call, once per process behind a `static const`) is the caller's choice.
inline bool env_flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e ? (dflt ? e[0] != '0' : e[0] == '1') : dflt;
}

inline int current_device() { int dev = 0; (void)hipGetDevice(&dev); return dev; }

// One T per device, value-initialised at first use on that device.  No lock of its own: a process-wide instance lives beside a
// mutex, a thread_local one needs none.  The reference is good until the next here().
template <class T>
struct PerDevice {
  std::vector<std::pair<int, T>> slots;
  T& here() {
    const int dev = current_device();
    for (auto& s : slots) if (s.first == dev) return s.second;
    slots.emplace_back(dev, T{});
    return slots.back().second;
  }
};

inline int cu_count() {                                    // compute units of the current device
  static std::mutex mu;
  static PerDevice<int> count;
  std::lock_guard<std::mutex> lk(mu);
  int& c = count.here();
  if (c == 0 && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, current_device()) != hipSuccess) { (void)hipGetLastError(); return 256; }
  return c;
}

// ---- dynamic LDS
struct LdsState {
  std::mutex mu;
  std::map<const void*, size_t> static_bytes;                         // kernel -> its __shared__ arrays
  std::map<std::pair<int, const void*>, size_t> configured;           // (device, kernel) -> largest dynamic size the attribute was set to
  hipError_t static_of(const void* kern, size_t* bytes) {            // (mu held)
    auto it = static_bytes.find(kern);
    if (it == static_bytes.end()) {
      hipFuncAttributes fa{};
      if (hipError_t e = hipFuncGetAttributes(&fa, kern)) return e;
      it = static_bytes.emplace(kern, fa.sharedSizeBytes).first;
    }
    *bytes = it->second;
    return hipSuccess;
  }
};
inline LdsState& lds_state() { static LdsState* s = new LdsState(); return *s; }     // (leaked: launches may outlive static destructors)

constexpr int LDS_OVER = -1;                                // dyn_lds: static + dynamic bytes exceed LDS_MAX (not a runtime error)
// Static LDS of a kernel (its host-side stub address), 0 if the runtime cannot tell.
inline size_t static_lds(const void* kern) {
  LdsState& s = lds_state();
  std::lock_guard<std::mutex> lk(s.mu);
  size_t st = 0;
  if (s.static_of(kern, &st) != hipSuccess) (void)hipGetLastError();
  return st;
}
// Would `bytes` of dynamic LDS fit beside the kernel's static LDS?  Touches no attribute: for route choices.  (If the runtime
// cannot tell the static size the answer is yes, and the dyn_lds() that follows on that route returns the runtime's error.)
inline bool lds_fits(const void* kern, size_t bytes) { return static_lds(kern) + bytes <= LDS_MAX; }
// Before a launch of `kern` with `bytes` of dynamic LDS on the current device: 0, LDS_OVER, or the runtime's hipError_t.
// The attribute is raised once per (device, kernel) and again only when a later launch needs more; a launch that fits the
// default makes no runtime call after the kernel's first.
inline int dyn_lds(const void* kern, size_t bytes) {
  LdsState& s = lds_state();
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(s.mu);
  size_t st = 0;
  if (hipError_t e = s.static_of(kern, &st)) return (int)e;
  if (st + bytes > LDS_MAX) return LDS_OVER;
  if (st + bytes <= LDS_DEFAULT) return 0;
  size_t& have = s.configured[{dev, kern}];
  if (have < bytes) {
    if (hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) return (int)e;
    have = bytes;                                           // (only now: a failed call is tried again by the next launch)
  }
  return 0;
}

// ---- scratch: device memory a launcher keeps between calls, keyed by (site, current device, stream) and owned by the calling
// thread.  `site` is any id the caller gives its use (one per independent block).  A block only grows: hipFree, which
// synchronises the device, then hipMalloc -- the contents are scratch.  Streams come and go, so a (site, device) remembers
// SCRATCH_STREAMS of them and forgets the oldest, once the device is idle and nothing can still be using its block.
constexpr size_t SCRATCH_STREAMS = 8;
struct ScratchBlock { int site, dev; hipStream_t stream; void* p; size_t cap; };
inline hipError_t scratch(int site, hipStream_t stream, size_t bytes, void** out) {
  static thread_local std::vector<ScratchBlock> blocks;               // oldest first
  const int dev = current_device();
  ScratchBlock* b = nullptr;
  size_t same = 0, oldest = 0;
  for (size_t i = 0; i < blocks.size(); ++i) {
    if (blocks[i].site != site || blocks[i].dev != dev) continue;
    if (!same++) oldest = i;
    if (blocks[i].stream == stream) b = &blocks[i];
  }
  if (!b) {
    if (same >= SCRATCH_STREAMS) {
      if (hipError_t e = hipDeviceSynchronize()) return e;
      (void)hipFree(blocks[oldest].p);
      blocks.erase(blocks.begin() + oldest);
    }
    blocks.push_back({site, dev, stream, nullptr, 0});
    b = &blocks.back();
  }
  if (b->cap < bytes) {
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr; b->cap = 0;
    if (hipError_t e = hipMalloc(&b->p, bytes)) return e;
    b->cap = bytes;
  }
  *out = b->p;
  return hipSuccess;
}

}  // namespace mjx
