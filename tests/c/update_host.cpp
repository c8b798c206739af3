// update_host.cpp -- the plain-C++ rules of the update path's host side against tables written out by hand, as an ordinary program:
// no HIP header, no GPU.  mjrl_amd/csrc/peer_layout.h: the peer exchange's buffer layout, the producer's and the consumer's view of
// one exchange (as offsets from fake base addresses that are never dereferenced) and the exchange counter; mjrl_amd/csrc/update_host.h:
// cg_route, peer_folds and ProfPick.  tests/test_update_host_cpu.py builds and runs it, tests/test_host_sanitizers.py once more
// under -fsanitize=address,undefined.
#include "../../mjrl_amd/csrc/update_host.h"

#include <cstdio>
#include <initializer_list>

using namespace mjx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d  ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static char* const BASE[3] = {(char*)0x10000000, (char*)0x20000000, (char*)0x30000000};   // three ranks' buffers, far apart
static long off(const void* p, const char* base) { return (long)((const char*)p - base); }

int main() {
  // ---- layout: a slot holds d floats rounded up to 16 bytes (scal_off) + 4 doubles, at least 64 doubles, in whole 256-byte lines
  struct { long d, scal_off, slot; } rows[] = {
      {1, 16, 512}, {3, 16, 512}, {4, 16, 512}, {5, 32, 512}, {124, 496, 768}, {8192, 32768, 33024}, {8193, 32784, 33024}, {166690, 666768, 666880}};
  for (const auto& r : rows)
    for (int w : {2, 3, 16}) {
      const PeerLayout L{r.d, w};
      const long slot = (long)L.slot_bytes(), total = (long)L.total_bytes();
      CHECK((long)L.scal_off() == r.scal_off && slot == r.slot, "d %ld: scal_off %zu slot %ld, want %ld / %ld", r.d, L.scal_off(), slot, r.scal_off, r.slot);
      CHECK(slot % 256 == 0 && slot >= 512 && r.d * 4 <= (long)L.scal_off() && (long)L.scal_off() + 32 <= slot, "d %ld: the vector and its 4 doubles fit the slot", r.d);
      CHECK(total == (2L * w + 1) * slot + 256, "d %ld world %d: %ld bytes in all", r.d, w, total);
      for (int par = 0; par < 2; ++par)
        for (int q = 0; q < w; ++q) CHECK((long)L.slot_off(par, q) == (long)(par * w + q) * slot, "d %ld world %d: slot (%d, %d)", r.d, w, par, q);
      CHECK((long)L.flags_off() == 2L * w * slot, "d %ld world %d: the flag block follows the last slot", r.d, w);
      CHECK((long)L.zeros_off() == (long)L.flags_off() + 256 && (long)L.zeros_off() + slot == total, "d %ld world %d: the slot of zeros ends the allocation", r.d, w);
    }
  // the flag block's 64 words: arrival flags 0..15 (one per source rank), then the two named words, apart from the flags and each other
  CHECK(PEER_MAX_WORLD == 16 && PeerLayout::FLAG_BLOCK == 256 && PeerLayout::TIMEOUTS == 32 && PeerLayout::FAULT_FLAG == 40, "flag words");
  CHECK(PeerLayout::TIMEOUTS >= PEER_MAX_WORLD && PeerLayout::FAULT_FLAG >= PEER_MAX_WORLD && PeerLayout::TIMEOUTS != PeerLayout::FAULT_FLAG &&
        4 * (PeerLayout::TIMEOUTS + 1) <= (int)PeerLayout::FLAG_BLOCK && 4 * (PeerLayout::FAULT_FLAG + 1) <= (int)PeerLayout::FLAG_BLOCK, "flag words do not overlap");

  // ---- views at d = 124 (768-byte slots): world 2 has its flag block at 3072, world 3 at 4608
  unsigned ticket_word = 0;
  for (int w : {2, 3}) {
    const PeerLayout L{124, w};
    const long S = 768, FL = 2L * w * S;
    for (int rank = 0; rank < w; ++rank)
      for (int par = 0; par < 2; ++par) {
        const unsigned seq = 40u + (unsigned)par;
        for (int fault = 0; fault <= 2; ++fault) {
          const PeerPush pp = peer_push_view(L, BASE, rank, par, seq, false, fault, &ticket_word);
          CHECK(pp.world == w && pp.rank == rank && pp.seq == seq && pp.ticket == &ticket_word, "push header (world %d rank %d)", w, rank);
          for (int q = 0; q < w; ++q) {
            const bool peer = q != rank;
            const long dst = (par * w + (peer && fault == 1 ? (rank + 1) % w : rank)) * S;          // fault 1: the next rank's slot, at the peers only
            CHECK(off(pp.dst[q], BASE[q]) == dst, "world %d rank %d par %d fault %d: dst[%d] at %ld, want %ld", w, rank, par, fault, q, off(pp.dst[q], BASE[q]), dst);
            if (peer && fault == 2) CHECK(off(pp.flag[q], BASE[rank]) == FL + 160, "fault 2: the flag for rank %d goes to word 40 of the own block", q);
            else CHECK(off(pp.flag[q], BASE[q]) == FL + 4 * rank, "world %d rank %d: flag[%d] at %ld, want word %d of rank %d's block", w, rank, q, off(pp.flag[q], BASE[q]), rank, q);
          }
          for (int q = w; q < 16; ++q) CHECK(pp.dst[q] == nullptr && pp.flag[q] == nullptr, "push entries beyond the world stay null");
        }
        // loop-back: every buffer is the own one; the flag raised for "peer" q is the one this rank polls for q
        char* const own[3] = {BASE[rank], BASE[rank], BASE[rank]};
        const PeerPush lb = peer_push_view(L, own, rank, par, seq, true, 0, &ticket_word);
        for (int q = 0; q < w; ++q)
          CHECK(off(lb.dst[q], BASE[rank]) == (par * w + rank) * S && off(lb.flag[q], BASE[rank]) == FL + 4 * q, "loop-back world %d rank %d par %d: entry %d", w, rank, par, q);

        const PeerSlots ps = peer_slots_view(L, BASE[rank], rank, par, seq, 12345ull);
        CHECK(ps.world == w && ps.rank == rank && ps.seq == seq && ps.ticks == 12345ull, "slots header (world %d rank %d)", w, rank);
        for (int r = 0; r < 16; ++r)
          CHECK(off(ps.slot[r], BASE[rank]) == (r < w ? (par * w + r) * S : FL + 256), "world %d rank %d par %d: slot[%d] at %ld", w, rank, par, r, off(ps.slot[r], BASE[rank]));
        CHECK(off(ps.flags, BASE[rank]) == FL && off(ps.timeouts, BASE[rank]) == FL + 128, "world %d rank %d: flags / time-out word", w, rank);
      }
  }
  {   // the same, some entries as plain numbers: world 3, rank 1, odd exchange
    const PeerLayout L{124, 3};
    const PeerPush pp = peer_push_view(L, BASE, 1, 1, 7u, false, 0, nullptr);
    CHECK(off(pp.dst[0], BASE[0]) == 3072 && off(pp.dst[2], BASE[2]) == 3072 && off(pp.flag[0], BASE[0]) == 4612 && off(pp.flag[1], BASE[1]) == 4612, "world 3 rank 1: producer");
    const PeerPush f1 = peer_push_view(L, BASE, 1, 1, 7u, false, 1, nullptr), f2 = peer_push_view(L, BASE, 1, 1, 7u, false, 2, nullptr);
    CHECK(off(f1.dst[0], BASE[0]) == 3840 && off(f1.dst[1], BASE[1]) == 3072 && off(f1.flag[0], BASE[0]) == 4612, "world 3 rank 1: fault 1");
    CHECK(off(f2.dst[0], BASE[0]) == 3072 && off(f2.flag[0], BASE[1]) == 4768 && off(f2.flag[1], BASE[1]) == 4612, "world 3 rank 1: fault 2");
    const PeerSlots ps = peer_slots_view(L, BASE[1], 1, 1, 7u, 1ull);
    CHECK(off(ps.slot[0], BASE[1]) == 2304 && off(ps.slot[2], BASE[1]) == 3840 && off(ps.slot[3], BASE[1]) == 4864 && off(ps.slot[15], BASE[1]) == 4864 &&
          off(ps.timeouts, BASE[1]) == 4736 && (long)L.total_bytes() == 4864 + 768, "world 3 rank 1: consumer");
  }

  // ---- exchange numbers: pre-incremented, parity = lowest bit, 32-bit wrap
  {
    uint32_t seq = 0;
    const unsigned want[][2] = {{1, 1}, {2, 0}, {3, 1}, {4, 0}};
    for (const auto& w : want) { const PeerRoundNo n = peer_next_round(&seq); CHECK(n.seq == w[0] && n.par == (int)w[1] && seq == w[0], "round %u", w[0]); }
    seq = 0xFFFFFFFEu;
    const unsigned wrap[][2] = {{0xFFFFFFFFu, 1}, {0, 0}, {1, 1}};
    for (const auto& w : wrap) { const PeerRoundNo n = peer_next_round(&seq); CHECK(n.seq == w[0] && n.par == (int)w[1] && seq == w[0], "round %u (wrap)", w[0]); }
  }

  // ---- routes around the register-resident limit
  struct { long d; CgRoute multi, single; bool folds; } routes[] = {
      {8188, CG_REG, CG_REG, true}, {8190, CG_REG, CG_REG, false}, {8192, CG_REG, CG_REG, true}, {8193, CG_MULTI, CG_LOOP, false}, {8196, CG_MULTI, CG_LOOP, false}};
  CHECK(CG_REG_MAX == 8192, "CG_REG_MAX");
  for (const auto& r : routes) {
    CHECK(cg_route(r.d, true) == r.multi && cg_route(r.d, false) == r.single, "cg_route(%ld): %d / %d", r.d, (int)cg_route(r.d, true), (int)cg_route(r.d, false));
    CHECK(peer_folds(TP_PEER, true, r.d) == r.folds, "peer_folds(peer, fused, %ld)", r.d);
    CHECK(!peer_folds(TP_PEER, false, r.d) && !peer_folds(TP_NONE, true, r.d) && !peer_folds(TP_RCCL, true, r.d) && !peer_folds(TP_HOOK, true, r.d), "peer_folds(%ld): fused path and peer exchange only", r.d);
  }

  // ---- profiling brackets: two solves of 10 iterations, as tests/test_gpu_operators.py runs them
  for (int k : {1, 7, 11}) {
    ProfPick p;
    CHECK(p.pick(ProfPick::PRODUCT, false) == -1 && p.seen == 0, "off until enabled");
    p.enable(k);
    int n = 0;
    for (int i = 0; i < 20; ++i) {
      CHECK(p.pick(ProfPick::ITERATION, i % 10 == 9) == -1, "enable(%d): no iteration brackets", k);
      const int pair = p.pick(ProfPick::PRODUCT, false);
      CHECK(pair == (i % k == 0 ? n : -1), "enable(%d): product %d -> pair %d", k, i, pair);
      if (pair >= 0) { p.close(); ++n; }
    }
    CHECK(n == (20 + k - 1) / k && p.used == (size_t)n && p.seen == 20, "enable(%d): %d pairs over 20 products", k, n);
    p.enable(-k);
    CHECK(p.used == 0 && p.seen == 0 && p.iter, "enable(%d) starts over", -k);
    n = 0;
    for (int i = 0, eligible = 0; i < 20; ++i) {
      const bool last = i % 10 == 9;
      const int pair = p.pick(ProfPick::ITERATION, last);
      CHECK(p.pick(ProfPick::PRODUCT, false) == -1, "enable(%d): no product brackets", -k);
      CHECK(pair == (!last && eligible % k == 0 ? n : -1), "enable(%d): iteration %d -> pair %d", -k, i, pair);
      if (!last) ++eligible;                                   // a solve's last iteration is neither bracketed nor counted
      if (pair >= 0) { p.close(); ++n; }
    }
    CHECK(n == (18 + k - 1) / k && p.used == (size_t)n && p.seen == 18, "enable(%d): %d pairs over 18 iterations", -k, n);
    p.enable(0);
    CHECK(!p.on && p.used == (size_t)n && p.pick(ProfPick::ITERATION, false) == -1 && p.pick(ProfPick::PRODUCT, false) == -1, "enable(0): off, the record stays");
  }
  {
    ProfPick p;
    p.enable(1);
    for (int i = 0; i < 2048; ++i) { const int pair = p.pick(ProfPick::PRODUCT, false); CHECK(pair == i, "pair %d of 2048", i); p.close(); }
    CHECK(ProfPick::PAIRS == 2048 && p.pick(ProfPick::PRODUCT, false) == -1 && p.used == 2048 && p.seen == 2049, "the pool ends at pair 2048");
    p.enable(7);
    CHECK(p.used == 0 && p.seen == 0 && p.stride == 7 && p.pick(ProfPick::PRODUCT, false) == 0, "enable resets an exhausted pool");
  }

  if (failures) { printf("update_host: %d failures\n", failures); return 1; }
  printf("update_host ok\n");
  return 0;
}
