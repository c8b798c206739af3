// launch_state_san.cpp -- mjrl_amd/csrc/launch_state.h (dynamic-LDS limits, CU counts, scratch blocks) against a FAKE HIP runtime
// with two devices, built as plain C++ under -fsanitize=address,undefined or -fsanitize=thread and driven from four threads at
// once.  The box the GPU suite runs on has one GPU, so this is where the two-device behaviour is exercised.  The fake defines the
// handful of hip* functions the header calls (no HIP library is linked): a thread-local current device, the dynamic-LDS
// attribute per (device, kernel), a settable static-LDS size per kernel, a malloc-backed allocator that remembers the device of
// each block, per-thread call counters and injectable failures.  tests/test_host_sanitizers.py builds and runs both variants.
#include "../../mjrl_amd/csrc/launch_state.h"

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>

namespace fake {
std::mutex mu;
thread_local int device = 0;
std::map<std::pair<int, const void*>, int> attr;            // what hipFuncSetAttribute left on (device, kernel)
std::map<const void*, size_t> static_lds;
std::map<const void*, int> fail_set, fail_get;              // the next n calls for this kernel fail
std::map<void*, std::pair<int, size_t>> blocks;             // live block -> (device it was made on, bytes)
std::atomic<int> cu_queries{0};
thread_local int n_set = 0, n_get = 0, n_malloc = 0, n_free = 0, n_sync = 0;
thread_local void* last_freed = nullptr;                    // (by this thread: an address may be live again at once, in another thread)
int attr_of(int dev, const void* k) { std::lock_guard<std::mutex> lk(mu); auto it = attr.find({dev, k}); return it == attr.end() ? 0 : it->second; }
int owner(void* p) { std::lock_guard<std::mutex> lk(mu); auto it = blocks.find(p); return it == blocks.end() ? -1 : it->second.first; }
size_t size_of(void* p) { std::lock_guard<std::mutex> lk(mu); auto it = blocks.find(p); return it == blocks.end() ? 0 : it->second.second; }
}  // namespace fake

extern "C" {
hipError_t hipGetDevice(int* dev) { *dev = fake::device; return hipSuccess; }
hipError_t hipSetDevice(int dev) { fake::device = dev; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { ++fake::n_sync; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int dev) {
  if (a != hipDeviceAttributeMultiprocessorCount) return hipErrorInvalidValue;
  ++fake::cu_queries;
  *v = dev == 0 ? 256 : 128;
  return hipSuccess;
}
hipError_t hipFuncGetAttributes(hipFuncAttributes* fa, const void* k) {
  std::lock_guard<std::mutex> lk(fake::mu);
  ++fake::n_get;
  if (fake::fail_get[k] > 0) { --fake::fail_get[k]; return hipErrorInvalidDeviceFunction; }
  memset(fa, 0, sizeof *fa);
  fa->sharedSizeBytes = fake::static_lds[k];
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* k, hipFuncAttribute a, int value) {
  std::lock_guard<std::mutex> lk(fake::mu);
  ++fake::n_set;
  if (a != hipFuncAttributeMaxDynamicSharedMemorySize) return hipErrorInvalidValue;
  if (fake::fail_set[k] > 0) { --fake::fail_set[k]; return hipErrorInvalidValue; }
  fake::attr[{fake::device, k}] = value;
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) {
  *p = malloc(bytes ? bytes : 1);
  std::lock_guard<std::mutex> lk(fake::mu);
  ++fake::n_malloc;
  fake::blocks[*p] = {fake::device, bytes};
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  {
    std::lock_guard<std::mutex> lk(fake::mu);
    ++fake::n_free;
    fake::last_freed = p;
    if (!fake::blocks.erase(p)) { fprintf(stderr, "hipFree of a block that is not live\n"); abort(); }
  }
  free(p);
  return hipSuccess;
}
}  // extern "C"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "launch_state_san: %s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace {
using namespace mjx;
constexpr size_t KB = 1024;
char kernels[4][8];        // kernel stub addresses, a row per thread
char shared_kernel;        // ... and one that every thread configures

void* fetch(int site, int stream, size_t bytes) {           // a scratch block, written end to end (ASan sees a short or freed one)
  void* p = nullptr;
  CHECK(scratch(site, (hipStream_t)(uintptr_t)(0x1000 + 16 * stream), bytes, &p) == hipSuccess && p != nullptr);
  CHECK(fake::owner(p) == fake::device && fake::size_of(p) >= bytes);
  memset(p, 0x5a, bytes);
  return p;
}

void scenario(int t, int round) {
  const void* k0 = &kernels[t][0]; const void* k1 = &kernels[t][1]; const void* k2 = &kernels[t][2];
  const void* k3 = &kernels[t][3]; const void* k4 = &kernels[t][4];
  const bool first = round == 0;
  // 1. configured on device 0, then AGAIN, with its own size, on device 1.  (A `static thread_local bool configured` beside the
  //    launch -- what mjx_bl_gram and mjx_mlp_fit_adam had -- fails the attr_of(1, k0) check: its flag is per thread, device 1 is
  //    never configured.)
  hipSetDevice(0);
  fake::n_set = fake::n_get = 0;
  CHECK(dyn_lds(k0, 100 * KB) == 0);
  hipSetDevice(1);
  CHECK(dyn_lds(k0, 120 * KB) == 0);
  if (first) CHECK(fake::attr_of(0, k0) == (int)(100 * KB));
  CHECK(fake::attr_of(1, k0) == (int)(120 * KB));
  if (first) CHECK(fake::n_set == 2 && fake::n_get == 1);              // the static size is looked up once per kernel, not per device
  // 2. more bytes raise the attribute; equal or fewer make no runtime call
  hipSetDevice(0);
  CHECK(dyn_lds(k0, 130 * KB) == 0 && fake::attr_of(0, k0) == (int)(130 * KB));
  fake::n_set = fake::n_get = 0;
  CHECK(dyn_lds(k0, 130 * KB) == 0 && dyn_lds(k0, 90 * KB) == 0 && dyn_lds(k0, 1 * KB) == 0);
  CHECK(fake::n_set == 0 && fake::n_get == 0 && fake::attr_of(0, k0) == (int)(130 * KB));
  CHECK(fake::attr_of(1, k0) == (int)(120 * KB));
  // 3. static + dynamic: exactly the limit passes (128 B static, the k_dyn_fit case), one byte more is refused without an
  //    attribute call; what fits the default needs no attribute at all; the predicate touches nothing
  if (first) { std::lock_guard<std::mutex> lk(fake::mu); fake::static_lds[k1] = 128; fake::static_lds[k2] = 128; }
  fake::n_set = 0;
  CHECK(lds_fits(k1, LDS_MAX - 128) && !lds_fits(k1, LDS_MAX - 127) && static_lds(k1) == 128);
  CHECK(dyn_lds(k2, LDS_MAX - 127) == LDS_OVER && dyn_lds(k2, LDS_DEFAULT - 128) == 0);
  CHECK(fake::n_set == 0 && fake::attr_of(0, k2) == 0);
  CHECK(dyn_lds(k1, LDS_MAX - 128) == 0 && fake::attr_of(0, k1) == (int)(LDS_MAX - 128));
  CHECK(dyn_lds(k1, LDS_MAX - 127) == LDS_OVER && fake::attr_of(0, k1) == (int)(LDS_MAX - 128));
  // 4. a runtime error comes back and is not remembered as "configured" (nor a failed static-size query as "known")
  if (first) {
    { std::lock_guard<std::mutex> lk(fake::mu); fake::fail_set[k3] = 1; fake::fail_get[k4] = 1; }
    fake::n_set = fake::n_get = 0;
    CHECK(dyn_lds(k3, 100 * KB) == (int)hipErrorInvalidValue && fake::attr_of(0, k3) == 0);
    CHECK(dyn_lds(k3, 100 * KB) == 0 && fake::attr_of(0, k3) == (int)(100 * KB) && fake::n_set == 2);
    CHECK(dyn_lds(k4, 100 * KB) == (int)hipErrorInvalidDeviceFunction && fake::n_set == 2);
    CHECK(dyn_lds(k4, 100 * KB) == 0 && fake::n_set == 3 && fake::n_get == 3);
  }
  // ... and a kernel all threads ask for, with different sizes, ends at the largest on both devices
  for (int dev = 0; dev < 2; ++dev) { hipSetDevice(dev); CHECK(dyn_lds(&shared_kernel, (100 + t) * KB) == 0); }
  // CU counts: per device, one query each for the whole process
  hipSetDevice(0); CHECK(cu_count() == 256);
  hipSetDevice(1); CHECK(cu_count() == 128);
  // 5. scratch: on the current device, a block per stream, the same block back for the same (site, device, stream), grown on
  //    demand; the ninth stream of a (site, device) evicts the oldest after a device synchronise
  const int site = 10 * round, other = 10 * round + 1;       // (blocks stay with their thread: fresh sites per round)
  hipSetDevice(1);
  fake::n_malloc = fake::n_free = fake::n_sync = 0;
  void* a = fetch(site, 0, 1000);
  void* b = fetch(site, 1, 1000);
  CHECK(a != b && fake::owner(a) == 1 && fake::n_malloc == 2);
  CHECK(fetch(site, 0, 1000) == a && fetch(site, 0, 10) == a && fetch(site, 1, 1000) == b && fake::n_malloc == 2 && fake::n_free == 0);
  void* a2 = fetch(site, 0, 5000);                           // grows: the old block is freed first
  CHECK(fake::n_malloc == 3 && fake::n_free == 1 && fake::size_of(a2) >= 5000 && fetch(site, 1, 10) == b);
  hipSetDevice(0);
  void* a0 = fetch(site, 0, 1000);                           // the same site and stream on another device: its own block, made there
  CHECK(fake::owner(a0) == 0 && fake::owner(a2) == 1 && a0 != a2);
  void* o = fetch(other, 0, 64);                             // another site shares nothing
  CHECK(o != a0);
  hipSetDevice(1);
  for (int s = 2; s < 8; ++s) fetch(site, s, 100);
  CHECK(fake::n_sync == 0 && fetch(site, 0, 5000) == a2);
  const int frees = fake::n_free;
  fetch(site, 8, 100);                                       // the ninth stream
  CHECK(fake::n_sync == 1 && fake::n_free == frees + 1 && fake::last_freed == a2);        // stream 0's block was the oldest
  CHECK(fetch(site, 1, 10) == b);                            // the others are still there
  const int mallocs = fake::n_malloc;
  fetch(site, 0, 100);                                       // stream 0 comes back: a new block, and stream 1's is now the oldest
  CHECK(fake::n_malloc == mallocs + 1 && fake::n_sync == 2 && fake::last_freed == b);
  hipSetDevice(0);
  CHECK(fetch(site, 0, 1000) == a0 && fetch(other, 0, 64) == o);       // device 0's blocks were not part of that
}
}  // namespace

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 3;
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t) th.emplace_back([t, rounds] { for (int r = 0; r < rounds; ++r) scenario(t, r); });
  for (auto& x : th) x.join();
  CHECK(fake::attr_of(0, &shared_kernel) == (int)(103 * KB) && fake::attr_of(1, &shared_kernel) == (int)(103 * KB));
  CHECK(fake::cu_queries.load() == 2);
  printf("launch_state_san ok\n");
  return 0;
}
