// model_host.cpp -- the plain-C++ top of mjrl_amd/csrc/model_host.h against a table written out by hand, as an ordinary program: no
// HIP header, no GPU.  model_routes orders the MFMA routes of the four learned-model entries that have a wide one (2: the wide
// LDS-tile kernel, 1: the register-chained instance; 0, the generic tail, is what remains) and names what a call without rows
// reports.  tests/test_model_host_cpu.py builds and runs it, once more under -fsanitize=address,undefined.
#include "../../mjrl_amd/csrc/model_host.h"

#include <cstdio>

using namespace mjx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d  ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
  // every combination of (asked_wide, mfma_on, wide_on, wide_fits, chained_fits) -> the routes tried, in order, and the empty call's answer
  struct { int asked, mfma, wide_on, wide_fits, chained_fits, n, first, second, empty; } rows[] = {
      // the narrow entry: route 1 where the MFMA switch is on and the chained shape fits, whatever the wide side says
      {0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 1, 0, 0, 0, 0}, {0, 0, 0, 1, 0, 0, 0, 0, 0}, {0, 0, 0, 1, 1, 0, 0, 0, 0},
      {0, 0, 1, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 1, 0, 0, 0, 0}, {0, 0, 1, 1, 0, 0, 0, 0, 0}, {0, 0, 1, 1, 1, 0, 0, 0, 0},
      {0, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 0, 0, 1, 1, 1, 0, 1}, {0, 1, 0, 1, 0, 0, 0, 0, 0}, {0, 1, 0, 1, 1, 1, 1, 0, 1},
      {0, 1, 1, 0, 0, 0, 0, 0, 0}, {0, 1, 1, 0, 1, 1, 1, 0, 1}, {0, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 1, 1, 1, 1, 1, 0, 1},
      // the wide entry with the MFMA switch off: no MFMA route at all
      {1, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 1, 0, 0, 0, 0}, {1, 0, 0, 1, 0, 0, 0, 0, 0}, {1, 0, 0, 1, 1, 0, 0, 0, 0},
      {1, 0, 1, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 0, 1, 0, 0, 0, 0}, {1, 0, 1, 1, 0, 0, 0, 0, 0}, {1, 0, 1, 1, 1, 0, 0, 0, 0},
      // ... with the wide switch off: the narrow entry's routes
      {1, 1, 0, 0, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 1, 1, 1, 0, 1}, {1, 1, 0, 1, 0, 0, 0, 0, 0}, {1, 1, 0, 1, 1, 1, 1, 0, 1},
      // ... with both on: route 2 first where the wide shape fits, route 1 behind it where the chained shape fits too
      {1, 1, 1, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 0, 1, 1, 1, 0, 1}, {1, 1, 1, 1, 0, 1, 2, 0, 2}, {1, 1, 1, 1, 1, 2, 2, 1, 2}};
  CHECK(sizeof rows / sizeof rows[0] == 32, "32 rows");
  unsigned seen = 0;
  for (const auto& t : rows) {
    seen |= 1u << (t.asked << 4 | t.mfma << 3 | t.wide_on << 2 | t.wide_fits << 1 | t.chained_fits);
    const ModelRoutes r = model_routes(t.asked, t.mfma, t.wide_on, t.wide_fits, t.chained_fits);
    CHECK(r.n == t.n && r.route[0] == t.first && r.route[1] == t.second && r.empty() == t.empty,
          "model_routes(%d, %d, %d, %d, %d): %d routes [%d, %d], empty %d; want %d [%d, %d], %d", t.asked, t.mfma, t.wide_on, t.wide_fits,
          t.chained_fits, r.n, r.route[0], r.route[1], r.empty(), t.n, t.first, t.second, t.empty);
  }
  CHECK(seen == 0xFFFFFFFFu, "every combination once (mask %08x)", seen);
  CHECK(ModelRoutes().n == 0 && ModelRoutes().empty() == 0, "no routes: the generic tail");

  if (failures) { printf("model_host: %d failures\n", failures); return 1; }
  printf("model_host ok\n");
  return 0;
}
