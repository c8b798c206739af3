// peer_layout.h -- the peer exchange's buffer (mjx_peer_*) as one definition: where the slots, the flag block and the slot of zeros
// lie, what a producer and a consumer kernel are handed for one exchange, and how exchanges are numbered.  Arithmetic on sizes and
// base pointers only: no kernel, no HIP call, nothing is dereferenced -- plain C++ (tests/c/update_host.cpp checks it against a table
// without a GPU).  vecops.h includes this header for the structs its kernels take by value.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mjx {

// Peer exchange (mjx_peer_*).  Every rank owns one uncached buffer [2 parities][world slots] + one arrival flag PER SOURCE RANK;
// the peers' buffers are mapped through hipIpcOpenMemHandle.  An all-reduce = every rank WRITES its vector into slot `rank` of
// every buffer (posted stores over xGMI), then stores the exchange number into ITS flag in every peer's buffer; the consumer
// kernel waits (bounded) on the flags of its OWN buffer -- local memory, one polling thread per source rank -- and sums its local
// slots in rank order: the same bits on every rank, no host in the loop.  A flag is written by exactly one rank over the same
// path as that rank's data stores, after they were acknowledged: no ordering between DIFFERENT peers' traffic is relied upon
// (an aggregate counter would need it for world > 2).
constexpr int PEER_MAX_WORLD = 16;
struct PeerSlots {                     // consumer: the local slots of this exchange (entries >= world point at a slot of zeros)
  const void* slot[16]; const unsigned* flags; unsigned* timeouts; unsigned long long ticks; unsigned seq; int world, rank;
};
// producer: slot `rank` in every buffer + the flag each peer polls for this rank; world == 0: off
struct PeerPush { void* dst[16]; unsigned* flag[16]; unsigned* ticket; unsigned seq; int world, rank; };

// what follows the LAST vector update of a solve, folded into its kernel (r06: k_cg_finish + k_apply_npg_step were two dependent
// ~4.7 us launches of a 3.8 ms -- or, on an eighth of the batch, 0.8 ms -- update): mode 1: x_out = x, bdotx = b.x (k_cg_finish);
// mode 2: ... and theta_out = theta + sqrt(|step_size / (b.x + 1e-20)|) x with the log_std clamp, the step length to alpha_out
// (k_apply_npg_step); mode 3: the same with the caller's constant step length.  Same arithmetic, same order, same bits.
struct CgFin {
  int mode = 0;
  const float* b = nullptr; float* x_out = nullptr; double* bdotx = nullptr;
  const float* theta = nullptr; float* theta_out = nullptr; double* alpha_out = nullptr;
  double step_size = 0.0; float const_alpha = 0.f, min_log_std = 0.f; int oS = 0;
};

// One rank's buffer for vectors of d floats among `world` ranks, in bytes from its base:
//   [parity 0: world slots][parity 1: world slots] | flag block (256 B) | one slot of zeros
// A slot holds a d-float vector and, at scal_off, the 4 doubles that may travel with it (K1's sums beside the gradient); at least
// 64 doubles, a multiple of 256 bytes.  The flag block is 64 words: [0..15] one arrival flag per SOURCE rank (32-bit exchange
// numbers), [TIMEOUTS] timed-out waits of this rank's consumers (mjx_peer_status), [FAULT_FLAG] where fault mode 2 sends the flags
// it withholds; the rest is unused.
struct PeerLayout {
  int64_t d; int world;
  static constexpr int TIMEOUTS = 32, FAULT_FLAG = 40;
  static constexpr size_t FLAG_BLOCK = 256;
  size_t scal_off() const { return ((size_t)d * sizeof(float) + 15) & ~(size_t)15; }
  size_t slot_bytes() const {
    size_t s = scal_off() + 4 * sizeof(double);
    if (s < 64 * sizeof(double)) s = 64 * sizeof(double);
    return (s + 255) & ~(size_t)255;
  }
  size_t slot_off(int par, int r) const { return (size_t)(par * world + r) * slot_bytes(); }   // the vector rank r contributed, parity par
  size_t flags_off() const { return (size_t)2 * world * slot_bytes(); }
  size_t zeros_off() const { return flags_off() + FLAG_BLOCK; }
  size_t total_bytes() const { return zeros_off() + slot_bytes(); }

  char* slot(char* base, int par, int r) const { return base + slot_off(par, r); }
  unsigned* flags(char* base) const { return (unsigned*)(base + flags_off()); }
};

// The producer's view of exchange `seq` for `rank`: map[q] = rank q's buffer as this rank sees it.  It writes slot `rank` of every
// buffer and raises the flag rank q polls for it; in the loop-back rehearsal (every map[q] is the own buffer) that is the flag
// this rank polls for "peer" q.  fault (MJX_PEER_FAULT, tests/test_gpu_multirank.py): what a mis-mapped buffer (1: the vectors land
// in the next rank's slot at the peers) or a lost flag store (2: the flags go to an unused word of the OWN flag block) would look
// like to the known-answer sum the host runs before it trusts a transport (engine._transport_self_test).
inline PeerPush peer_push_view(const PeerLayout& L, char* const* map, int rank, int par, uint32_t seq, bool loopback, int fault, unsigned* ticket) {
  PeerPush pp{};
  pp.world = L.world; pp.rank = rank; pp.seq = seq; pp.ticket = ticket;
  for (int q = 0; q < L.world; ++q) {
    pp.dst[q] = L.slot(map[q], par, rank);
    pp.flag[q] = loopback ? L.flags(map[rank]) + q : L.flags(map[q]) + rank;
    if (q != rank && fault == 1) pp.dst[q] = L.slot(map[q], par, (rank + 1) % L.world);
    if (q != rank && fault == 2) pp.flag[q] = L.flags(map[rank]) + PeerLayout::FAULT_FLAG;
  }
  return pp;
}
// The consumer's view of exchange `seq`: the slots of its own buffer in rank order (the surplus entries: the slot of zeros) and
// the flags the peers raise to `seq` once their vectors have landed; a wait gives up after `ticks` (100 MHz) and counts itself.
inline PeerSlots peer_slots_view(const PeerLayout& L, char* own, int rank, int par, uint32_t seq, unsigned long long ticks) {
  PeerSlots ps{};
  ps.world = L.world; ps.rank = rank; ps.seq = seq; ps.ticks = ticks;
  for (int r = 0; r < PEER_MAX_WORLD; ++r) ps.slot[r] = r < L.world ? L.slot(own, par, r) : own + L.zeros_off();
  ps.flags = L.flags(own);
  ps.timeouts = L.flags(own) + PeerLayout::TIMEOUTS;
  return ps;
}

// The next exchange after `*seq`: numbers are 32 bits, compared as a signed difference by the kernels, and may wrap; consecutive
// exchanges alternate between the two slot sets, so a rank one exchange ahead never overwrites what a slower one still reads.
struct PeerRoundNo { uint32_t seq; int par; };
inline PeerRoundNo peer_next_round(uint32_t* seq) { const uint32_t s = ++*seq; return PeerRoundNo{s, (int)(s & 1u)}; }

}  // namespace mjx
