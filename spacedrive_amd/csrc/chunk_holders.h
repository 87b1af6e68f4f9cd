// chunk_holders.h — the holders index (chunk_holders.hip): the chunk index's
// sibling that keeps EVERY holder of a pair, so that a file's entries can be
// taken out again. The same four caller-owned arrays as the chunk index
// (chunk_index.h, include/sdcas.h), but strictly ascending in the TRIPLE (key,
// digest as 32 bytes in memcmp order, value as u64): a pair repeats once per
// distinct value, lowest value first. Every chunk index is a holders index.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "chunk_index.h"

namespace sdcas {

constexpr uint32_t kHoldersRemoveCounts = 4;  // sdcas_holders_remove_counts' words
constexpr uint32_t kHoldersTB = 256;          // entries per workgroup, and counts per scan tile

// 0: a holders index; 1: entry *bad does not order after the one before (by
// the triple); 2: directory slot *bad does not hold its count. Host arrays;
// values may be null (all 0).
int holders_check(const uint64_t* keys, const uint8_t* digests, const uint64_t* values, const uint32_t* dir, uint64_t n,
                  uint32_t bits, uint64_t* bad);

// The ordered compactions' counts for `items` flags, one u32 per 256 of them,
// scanned in three levels of 256 (2^30 items: 2^22, 2^14, 2^6 counts) with the
// total behind them:
//   l1  u32[ceil(items / 256)]   per workgroup, then their exclusive scan within each tile of 256
//   l2  u32[ceil(l1 / 256)]      per l1 tile, likewise
//   l3  u32[ceil(l2 / 256)]      per l2 tile (at most 64: one workgroup scans them all)
//   tot u32[4]                   [0] the sum of all
// A flag's place is l1[b] + l2[b >> 8] + l3[b >> 16] plus its rank in its
// workgroup b.
struct HoldersScanLayout {
  uint64_t l1, l2, l3, tot, bytes;
  uint32_t n1, n2, n3;
};
inline uint32_t holders_tiles(uint64_t items) { return items ? (uint32_t)((items + kHoldersTB - 1) / kHoldersTB) : 1u; }
inline HoldersScanLayout holders_scan_layout(uint64_t items, uint64_t from) {
  HoldersScanLayout l{};
  uint64_t o = from;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.n1 = holders_tiles(items), l.n2 = holders_tiles(l.n1), l.n3 = holders_tiles(l.n2);
  l.l1 = take(4ull * l.n1), l.l2 = take(4ull * l.n2), l.l3 = take(4ull * l.n3), l.tot = take(16);
  l.bytes = o;
  return l;
}

// The add's workspace for a batch of m, in bytes from its start (every part
// 16-byte aligned):
//   ord_a/b    u32[m]   the batch positions in triple order: the merge sort's ping and pong
//   lbf        u32[m]   by place in that order: the triple's lower bound in the old index,
//                       bit 31: the triple is there, bit 30: the place is a new triple's first
//   lbs        u32[m]   the new triples' lower bounds, compacted (ascending)
//   scan                holders_scan_layout(m): 4 bytes per 256 places and less above
//   counts     u64[6]
// 16 bytes per batch entry and 1/64 word of counts; nothing grows with n_old.
struct HoldersAddLayout {
  uint64_t ord_a, ord_b, lbf, lbs, counts, bytes;
  HoldersScanLayout scan;
};
inline HoldersAddLayout holders_add_layout(uint64_t m) {
  HoldersAddLayout l{};
  const uint64_t w = (4 * m + 15) & ~15ull;
  l.ord_a = 0, l.ord_b = w, l.lbf = 2 * w, l.lbs = 3 * w;
  l.scan = holders_scan_layout(m, 4 * w);
  l.counts = l.scan.bytes;
  l.bytes = l.counts + 8 * kIndexAddCounts;
  return l;
}

// The remove's workspace for n_old entries: per workgroup of 256 entries the
// four waves' keep masks (u64[4], so that `removed` is searched once per
// entry) and the counts above; 36 bytes and a little per 256 entries.
struct HoldersRemoveLayout {
  uint64_t masks, counts, bytes;
  HoldersScanLayout scan;
};
inline HoldersRemoveLayout holders_remove_layout(uint64_t n_old) {
  HoldersRemoveLayout l{};
  l.masks = 0;
  l.scan = holders_scan_layout(n_old, 32ull * holders_tiles(n_old));
  l.counts = l.scan.bytes;
  l.bytes = l.counts + 8 * kHoldersRemoveCounts;
  return l;
}

// m queries against the holders index: pos (i64[m]: the FIRST entry with the
// pair), value (u64[m]: its value, the lowest holder), holders (u32[m]: the
// entries with the pair) and counts (u64[kIndexMatchCounts], overwritten) may
// each be null. m in [1, 2^30]. Enqueues on st, uses no workspace.
hipError_t holders_match(const IndexView& idx, const uint64_t* keys, const uint8_t* digests, const uint8_t* valid,
                         uint32_t m, int64_t* pos, uint64_t* value, uint32_t* holders, unsigned long long* counts,
                         hipStream_t st);

// The merge of the batch's valid triples into a new index. ws:
// holders_add_layout(m).bytes, 16-byte aligned. values may be null (0). pos
// (i64[m]), flags (u8[m]) and counts (u64[kIndexAddCounts], overwritten) may
// each be null. old.n + m <= 2^30; m == 0 copies the old entries and builds the
// directory at out.bits. Enqueues on st and never waits.
hipError_t holders_add(uint8_t* ws, const IndexView& old, const uint64_t* keys, const uint8_t* digests,
                       const uint64_t* values, const uint8_t* valid, uint32_t m, const IndexOut& out, int64_t* pos,
                       uint8_t* flags, unsigned long long* counts, hipStream_t st);

// The old entries whose value is not in removed[r] (ascending), in their old
// order, into `out` (arrays of old.n entries) with the directory at out.bits.
// ws: holders_remove_layout(old.n).bytes, 16-byte aligned. counts
// (u64[kHoldersRemoveCounts], overwritten) may be null. Enqueues on st and
// never waits.
hipError_t holders_remove(uint8_t* ws, const IndexView& old, const uint64_t* removed, uint32_t r, const IndexOut& out,
                          unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
