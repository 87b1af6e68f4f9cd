// dupsets.h — duplicate sets from a per-file label (dupsets.hip): the grouped,
// ordered form of sdcas_confirm_duplicates' rep, with the bytes of one copy
// and what deleting the extra copies gives back.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

constexpr uint64_t kDupsetsMaxFiles = 1ull << 30;  // file indices and set ranks are 32-bit
constexpr uint32_t kDupsetsCounts = 6;             // sdcas_sets_counts' words
constexpr uint32_t kDupsetsTile = 4096;            // files (sets, histogram words) per workgroup
constexpr uint32_t kDupsetsBySetRep = 0, kDupsetsByReclaimable = 1;  // SDCAS_SETS_BY_*

// The workspace for n files, in u32 words from its start (every offset even,
// so the u64 parts are 8-byte aligned when the workspace is):
//   cnt, low, rank      n each      per label: files, lowest file, final set rank
//   hd_file/cnt/label   h each      per set in rep order (h = n / 2 + 1)
//   fcnt                h           per set in final order: files, then their offsets
//   key_a, key_b        n + 2 each  the sorts' keys, ping and pong (u64 per set or u32 per member)
//   val_a, val_b        n each      the sorts' values
//   hist                256 per tile of n
//   bsum, tcnt          per-tile sums of the scans and of the compactions
//   tot                 4           sets, members in sets, a scan's unused total
//   counts              6 u64
// 9 words = 36 bytes per file, plus 1/16 word per file of histogram.
struct DupsetsLayout {
  uint64_t cnt, low, rank, hd_file, hd_cnt, hd_label, fcnt, key_a, key_b, val_a, val_b, hist, bsum, tcnt, tot, counts,
      words;
  uint32_t h, tiles;
};
inline uint32_t dupsets_tiles(uint64_t m) { return m ? (uint32_t)((m + kDupsetsTile - 1) / kDupsetsTile) : 1u; }
inline DupsetsLayout dupsets_layout(uint64_t n) {
  DupsetsLayout l{};
  const uint64_t ne = (n + 1) & ~1ull;
  l.h = (uint32_t)(n / 2 + 1);
  const uint64_t he = ((uint64_t)l.h + 1) & ~1ull;
  l.tiles = dupsets_tiles(n);
  uint64_t o = 0;
  auto take = [&o](uint64_t words) {
    const uint64_t at = o;
    o += (words + 1) & ~1ull;
    return at;
  };
  l.cnt = take(ne), l.low = take(ne), l.rank = take(ne);
  l.hd_file = take(he), l.hd_cnt = take(he), l.hd_label = take(he), l.fcnt = take(he);
  l.key_a = take(ne + 2), l.key_b = take(ne + 2), l.val_a = take(ne), l.val_b = take(ne);
  l.hist = take(256ull * l.tiles);
  l.bsum = take((uint64_t)dupsets_tiles(256ull * l.tiles) + dupsets_tiles(l.h) + 2);
  l.tcnt = take((uint64_t)l.tiles + 2);
  l.tot = take(4);
  l.counts = take(2 * kDupsetsCounts);
  l.words = o;
  return l;
}
inline uint64_t dupsets_ws_words(uint64_t n) { return dupsets_layout(n).words; }

// rep[n] (i64) and sizes[n] (u64, may be null): device inputs. set_rep /
// set_bytes (n / 2 entries), set_offsets (n / 2 + 1), members (n) and counts
// (u64[kDupsetsCounts], overwritten) may each be null; entries past the number
// of sets / members are not written. ws: dupsets_ws_words(n) words, 8-byte
// aligned. Enqueues on st and never waits for it; n in [1, kDupsetsMaxFiles],
// order a kDupsetsBy* with sizes non-null for kDupsetsByReclaimable.
hipError_t duplicate_sets(uint32_t* ws, const int64_t* rep, const uint64_t* sizes, uint32_t n, uint32_t order,
                          int64_t* set_rep, uint64_t* set_offsets, uint64_t* set_bytes, int64_t* members,
                          unsigned long long* counts, hipStream_t st);

// ---- the passes dirtree.hip shares -----------------------------------------------
// The stable LSD radix sort (k_ds_hist / k_ds_scatter and the scan between
// them): the first *m_p of at most `bound` (key, value) pairs by the keys' low
// 8 * passes bits; the result is in (ka, va) after an even number of passes,
// else in (kb, vb). hist: 256 words per tile of `bound`; bsum:
// dupsets_tiles(256 * dupsets_tiles(bound)) + 2 words; scan_total: one word.
hipError_t dupsets_sort_u64(uint64_t* ka, uint64_t* kb, uint32_t* va, uint32_t* vb, uint32_t bound,
                            const uint32_t* m_p, uint32_t passes, uint32_t* hist, uint32_t* bsum,
                            uint32_t* scan_total, hipStream_t st);
hipError_t dupsets_sort_u32(uint32_t* ka, uint32_t* kb, uint32_t* va, uint32_t* vb, uint32_t bound,
                            const uint32_t* m_p, uint32_t passes, uint32_t* hist, uint32_t* bsum,
                            uint32_t* scan_total, hipStream_t st);
// k_ds_count: cnt[label] += the entries that carry it, low[label] = the lowest
// of them (cnt zeroed and low filled with 0xFF by the caller), counts[0] += the
// entries whose label lies in [0, n)
hipError_t dupsets_label_counts(const int64_t* rep, uint32_t n, uint32_t* cnt, uint32_t* low,
                                unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
