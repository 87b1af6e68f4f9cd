// chunk_peers.h — the chunk peers (chunk_peers.hip): for a batch's chunks, per
// file, the bytes it shares with EVERY file that holds any of them in a holders
// index (chunk_holders.h), and the top k of those files. include/sdcas.h has the
// public definition; this is the workspace and the one device call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "chunk_holders.h"

namespace sdcas {

constexpr uint32_t kPeersCounts = 7;             // sdcas_peers_counts' words
constexpr uint32_t kPeersMaxK = 64;              // SDCAS_PEERS_MAX_K
constexpr uint32_t kPeersMaxHolders = 1u << 20;  // SDCAS_PEERS_MAX_HOLDERS
constexpr uint64_t kPeersMaxPairs = 1ull << 30;  // place numbers are 32-bit
constexpr uint32_t kPeersEarlier = 0, kPeersAll = 1;  // SDCAS_PEERS_*

// the bound on the (chunk, holder) pairs that can never overflow
inline uint64_t peers_pair_bound(uint64_t m, uint64_t max_holders) {
  const uint64_t p = m * max_holders;  // m <= 2^30, max_holders <= 2^20
  return p < kPeersMaxPairs ? p : kPeersMaxPairs;
}

// The workspace for a batch of m chunks and q = max_pairs pair places, in bytes
// from its start (every part 16-byte aligned):
//   first, cnt, off, self  u32[m]  the run's first entry, the counted holders (0: none, common or
//                                  no part), their exclusive scan, self's place in the run (ALL mode)
//   cscan                          holders_scan_layout(m): the scan's upper levels
//   p_file   u32[q]  p_holder u64[q]  p_len u64[q]   the expansion, by place
//   ord_a/b  u32[q]                the places, then the edges, in order: the merge sorts' ping and pong
//   run      u64[q]                the lengths in place order, then their exclusive scan per tile of 256
//   s1 s2 s3 stot   u64            that scan's upper levels (2^22, 2^14, 2^6 sums for 2^30 places) and total
//   head     u8[q]                 the place is the first of its (file, holder)
//   hscan                          holders_scan_layout(q): the heads counted; tot[0] is the number of edges
//   e_file   u32[q]  e_holder u64[q]  e_beg u64[q]   the edges, by rank among the heads; e_beg turns into
//                                  the edge's bytes. The scan at a run's end goes to e_end = p_len, whose
//                                  lengths the scan has taken over by then
//   sc       u64[4]                pairs (P), chunks, common chunks, files with a peer
//   np       u32[4]                [0] the places expanded (0 on overflow), [1] overflow
//   counts   u64[7]
// 16 bytes per chunk, 57 per pair place and the scans' 1/64 and 1/32 word.
struct PeersLayout {
  uint64_t first, cnt, off, self, p_file, p_holder, p_len, ord_a, ord_b, run, s1, s2, s3, stot, head, e_file, e_holder,
      e_beg, sc, np, counts, bytes;
  uint32_t n1, n2, n3;  // the u64 scan's counts per level
  HoldersScanLayout cscan, hscan;
};
inline PeersLayout peers_layout(uint64_t m, uint64_t q) {
  PeersLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.first = take(4 * m), l.cnt = take(4 * m), l.off = take(4 * m), l.self = take(4 * m);
  l.cscan = holders_scan_layout(m, o);
  o = l.cscan.bytes;
  l.p_file = take(4 * q), l.p_holder = take(8 * q), l.p_len = take(8 * q);
  l.ord_a = take(4 * q), l.ord_b = take(4 * q), l.run = take(8 * q);
  l.n1 = holders_tiles(q), l.n2 = holders_tiles(l.n1), l.n3 = holders_tiles(l.n2);
  l.s1 = take(8ull * l.n1), l.s2 = take(8ull * l.n2), l.s3 = take(8ull * l.n3), l.stot = take(16);
  l.head = take(q);
  l.hscan = holders_scan_layout(q, o);
  o = l.hscan.bytes;
  l.e_file = take(4 * q), l.e_holder = take(8 * q), l.e_beg = take(8 * q);
  l.sc = take(8 * 4), l.np = take(4 * 4), l.counts = take(8 * kPeersCounts);
  l.bytes = o;
  return l;
}

// the batch and the request
struct PeersIn {
  const uint64_t* keys;
  const uint8_t* digests;
  const uint8_t* valid;  // null: all valid
  const uint32_t* chunk_file;
  const uint64_t* chunk_len;
  const uint64_t* file_ids;
  uint32_t m, n_files, k, max_holders, mode;
};
// every one may be null
struct PeersOut {
  uint32_t* peer_count;  // [n_files]
  uint64_t* peers;       // [n_files * k]
  uint64_t* peer_bytes;  // [n_files * k]
  uint64_t* shared;      // [n_files]
  uint64_t* unique;      // [n_files]
  uint64_t* common;      // [n_files]
};

// ws: peers_layout(in.m, max_pairs).bytes, 16-byte aligned. m <= 2^30, n_files
// < 2^32 - 1, 1 <= k <= 64, max_pairs <= 2^30. counts (u64[kPeersCounts],
// overwritten) may be null. Enqueues on st and never waits: every grid is sized
// from m, n_files and max_pairs, the pairs and the edges stay on the device.
hipError_t chunk_peers(uint8_t* ws, const IndexView& idx, const PeersIn& in, uint32_t max_pairs, const PeersOut& out,
                       unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
