// chunk_index.h — the persistent, sorted chunk index (chunk_index.hip): the
// "existing" side of the chunk group-by. An index is four caller-owned arrays
// (include/sdcas.h has the public definition): keys, 32-byte digests and
// values, strictly ascending in (key, digest as 32 bytes in memcmp order), and
// a directory over the keys' top bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "confirm.h"
#include "dupsets.h"

namespace sdcas {

constexpr uint64_t kIndexMaxEntries = 1ull << 30;  // entry numbers are 32-bit, bit 31 is a flag
constexpr uint32_t kIndexMaxBits = 28;
constexpr uint32_t kIndexMatchCounts = 4;  // sdcas_index_match_counts' words
constexpr uint32_t kIndexAddCounts = 6;    // sdcas_index_add_counts' words

// an index on the device (n == 0: no array is read)
struct IndexView {
  const uint64_t* keys;
  const uint8_t* digests;
  const uint64_t* values;
  const uint32_t* dir;
  uint32_t n;
  uint32_t bits;
};
// the arrays of the index an add writes
struct IndexOut {
  uint64_t* keys;
  uint8_t* digests;
  uint64_t* values;
  uint32_t* dir;
  uint32_t bits;
};

inline uint32_t index_dir_bits(uint64_t n) {
  if (n < 8) return 0;
  uint32_t lg = 0;  // ceil_log2(n)
  while ((1ull << lg) < n) ++lg;
  return lg - 2 < kIndexMaxBits ? lg - 2 : kIndexMaxBits;
}
inline uint64_t index_dir_slots(uint32_t bits) { return (1ull << bits) + 1; }

// every kernel of the two indexes: workgroups of 256, one item per thread
constexpr uint32_t kIndexTB = 256;
inline uint32_t index_blocks(uint64_t items) { return (uint32_t)((items + kIndexTB - 1) / kIndexTB); }
// the part of a workspace that starts `off` bytes in
template <typename T>
inline T* index_at(uint8_t* ws, uint64_t off) {
  return reinterpret_cast<T*>(ws + off);
}

// 0: an index; 1: entry *bad does not order after the one before; 2: directory
// slot *bad does not hold its count. Host arrays.
int index_check(const uint64_t* keys, const uint8_t* digests, const uint32_t* dir, uint64_t n, uint32_t bits,
                uint64_t* bad);
// the directory half of a check: 0, or 2 with the first slot that is wrong in *bad
int index_dir_check(const uint64_t* keys, const uint32_t* dir, uint64_t n, uint32_t bits, uint64_t* bad);

// The three steps both indexes' adds (and the holders' remove) end with, each
// one kernel enqueued on st; the caller reads hipGetLastError.
// An old entry goes to its index plus the number of lbs[0 .. min(*na_p, m))
// (the added entries' lower bounds, ascending) that are <= it.
void index_place_old(const IndexView& old, const uint32_t* lbs, const uint32_t* na_p, uint32_t m, const IndexOut& out,
                     uint32_t cap, hipStream_t st);
// dir[j] <- the number of the n = base + min(*extra_p, extra_max) entries of
// nkeys whose key's top `bits` bits are below j
void index_build_dir(const uint64_t* nkeys, uint32_t base, const uint32_t* extra_p, uint32_t extra_max, uint32_t bits,
                     uint32_t* dir, hipStream_t st);
// cts[4], cts[5] <- entries_old, entries_new
void index_add_totals(const uint32_t* na_p, uint32_t m, uint32_t n_old, unsigned long long* cts, hipStream_t st);

// The add's workspace for a batch of m, in bytes from its start (every part
// 16-byte aligned):
//   rep        i64[m]      confirm's rep over the batch: the lowest position with the pair
//   mlb        u32[m]      the pair's lower bound in the old index, bit 31: it is there
//   npos       u32[m]      an added pair's entry in the new index, by batch position
//   key_a/b    u64[m + 1]  the sort's keys, ping and pong
//   val_a/b    u32[m]      the sort's values: batch positions
//   ord        u32[m]      the added pairs' batch positions in index order
//   lbs        u32[m]      their lower bounds in the old index (ascending)
//   hist, bsum             the radix sort's (dupsets.h)
//   tot        u32[4]      [0] added, [1] a long run met, [2] the long path's count, [3] a scan's unused total
//   counts     u64[6]
// 52 bytes per batch entry (and 1/16 word of histogram); confirm's tables
// (confirm.h) are the context's own.
struct IndexAddLayout {
  uint64_t rep, mlb, npos, key_a, key_b, val_a, val_b, ord, lbs, hist, bsum, tot, counts, bytes;
};
inline IndexAddLayout index_add_layout(uint64_t m) {
  IndexAddLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  const uint64_t tiles = dupsets_tiles(m);
  l.rep = take(8 * m), l.mlb = take(4 * m), l.npos = take(4 * m);
  l.key_a = take(8 * (m + 1)), l.key_b = take(8 * (m + 1));
  l.val_a = take(4 * m), l.val_b = take(4 * m), l.ord = take(4 * m), l.lbs = take(4 * m);
  l.hist = take(4 * 256 * tiles);
  l.bsum = take(4 * ((uint64_t)dupsets_tiles(256 * tiles) + 2));
  l.tot = take(16);
  l.counts = take(8 * kIndexAddCounts);
  l.bytes = o;
  return l;
}

// m queries against the index: pos (i64[m]), value (u64[m]) and counts
// (u64[kIndexMatchCounts], overwritten) may each be null. m in [1, 2^30].
// Enqueues on st, uses no workspace.
hipError_t index_match(const IndexView& idx, const uint64_t* keys, const uint8_t* digests, const uint8_t* valid,
                       uint32_t m, int64_t* pos, uint64_t* value, unsigned long long* counts, hipStream_t st);

// The merge of the batch into a new index. ws: index_add_layout(m).bytes,
// 16-byte aligned; cf_ws: confirm_ws_words(m) words. values may be null (0).
// pos (i64[m]), flags (u8[m]) and counts (u64[kIndexAddCounts], overwritten)
// may each be null. old.n + m <= 2^30; m == 0 copies the old entries and builds
// the directory at out.bits. Enqueues on st and never waits.
hipError_t index_add(uint8_t* ws, uint32_t* cf_ws, const IndexView& old, const uint64_t* keys, const uint8_t* digests,
                     const uint64_t* values, const uint8_t* valid, uint32_t m, const IndexOut& out, int64_t* pos,
                     uint8_t* flags, unsigned long long* counts, hipStream_t st);
}  // namespace sdcas
