// families.h — the file families (families.hip): the connected components of
// the graph whose edges are the peer rows (chunk_peers.h) that pass a
// shared-bytes threshold. include/sdcas.h has the public definition; this is
// the workspace and the one device call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "chunk_peers.h"

namespace sdcas {

constexpr uint32_t kFamiliesCounts = 10;             // sdcas_families_counts' words
constexpr uint64_t kFamiliesMaxFiles = 1ull << 30;   // labels are 32-bit row indices
constexpr uint32_t kFamiliesTB = 256;                // every kernel: one row per thread
constexpr uint32_t kFamiliesMaxPasses = 30;          // ceil_log2(2^30)

// ceil_log2(n) for n >= 1: the jump passes that flatten a forest of n rows
inline uint32_t families_passes(uint64_t n) {
  uint32_t lg = 0;
  while ((1ull << lg) < n) ++lg;
  return lg;
}

// The workspace for n rows, in bytes from its start (every part 16-byte aligned):
//   parent  u32[n]   the forest: parent[x] <= x, a root points at itself
//   size    u32[n]   per root: the rows of its component
//   flags   u32[32]  [0] unsorted; [1 + p] pass p of the jumps moved something
//   sc      u64[8]   slots, missing, self, weak, links, families, members, largest
// 8 bytes per row and 192 bytes.
struct FamiliesLayout {
  uint64_t parent, size, flags, sc, bytes;
};
inline FamiliesLayout families_layout(uint64_t n) {
  FamiliesLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.parent = take(4 * n), l.size = take(4 * n);
  l.flags = take(4 * 32), l.sc = take(8 * 8);
  l.bytes = o;
  return l;
}

// the rows and the request
struct FamiliesIn {
  const uint64_t* ids;         // [n] strictly ascending (checked on the device)
  const uint64_t* sizes;       // [n]
  const uint32_t* peer_count;  // [n]
  const uint64_t* peers;       // [n * k]
  const uint64_t* peer_bytes;  // [n * k]
  uint32_t n, k, num, den;
};

// ws: families_layout(in.n).bytes, 16-byte aligned. n <= 2^30, 1 <= k <= 64,
// den >= 1, num <= den. family (i64[n]), family_size (u32[n]) and counts
// (u64[kFamiliesCounts], overwritten) may each be null. Enqueues on st and
// never waits: every grid is sized from n, the number of jump passes is
// ceil_log2(n).
hipError_t file_families(uint8_t* ws, const FamiliesIn& in, int64_t* family, uint32_t* family_size,
                         unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
