// family_bytes.h — the family bytes (family_bytes.hip): what the rows of one
// label store and give back, a group-by over (label of the chunk's row, chunk
// class). include/sdcas.h has the public definition; this is the workspace and
// the one device call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

constexpr uint32_t kFamilyBytesCounts = 9;              // sdcas_family_bytes_counts' words
constexpr uint64_t kFamilyBytesMaxChunks = 1ull << 30;  // chunk positions are 32-bit, the table has 2 m slots
constexpr uint64_t kFamilyBytesMaxFiles = 1ull << 30;   // labels are 32-bit row indices
constexpr uint32_t kFamilyBytesTB = 256;                // every kernel: one item per thread

// the class table's slots for m chunks: a power of two, at least 2 m (never more than half full)
inline uint64_t family_bytes_slots(uint64_t m) {
  uint64_t cap = 16;
  while (cap < 2 * m) cap <<= 1;
  return cap;
}

// ceil_log2(n) for n >= 1: the merge passes that order n rows
inline uint32_t family_bytes_passes(uint64_t n) {
  uint32_t lg = 0;
  while ((1ull << lg) < n) ++lg;
  return lg;
}

// The workspace for m chunks of n rows, in bytes from its start (every part
// 16-byte aligned). Filled with 0xFF before a call:
//   table      u32[slots]  per slot: its class's lowest participating chunk
//   lab_low    u32[n]      per label: its lowest participating row
// filled with 0 before a call:
//   row_sum    u64[3 n]    per row: delta, self, inherited
//   lab_total  u64[n]      per label: the bytes of its rows
//   lab_stored u64[n]      per label: the delta bytes of its rows
//   lab_rows   u32[n]      per label: its participating rows
//   sc         u64[16]     the nine counts as they add up
// written before they are read:
//   slot       u32[m]      per chunk: its class's slot, or none
//   rec        u64[n]      per row: the reclaimable bytes of the set it heads
//   head       u8[n]       per row: it is the lowest row of a set
//   ord        u32[2][n]   the rows as the merge passes order them
struct FamilyBytesLayout {
  uint64_t table, lab_low, row_sum, lab_total, lab_stored, lab_rows, sc, slot, rec, head, ord0, ord1, bytes;
  uint64_t slots;
};
inline FamilyBytesLayout family_bytes_layout(uint64_t m, uint64_t n) {
  FamilyBytesLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.slots = family_bytes_slots(m);
  l.table = take(4 * l.slots), l.lab_low = take(4 * n);
  l.row_sum = take(8 * 3 * n), l.lab_total = take(8 * n), l.lab_stored = take(8 * n), l.lab_rows = take(4 * n);
  l.sc = take(8 * 16);
  l.slot = take(4 * m), l.rec = take(8 * n), l.head = take(n);
  l.ord0 = take(4 * n), l.ord1 = take(4 * n);
  l.bytes = o;
  return l;
}

struct FamilyBytesIn {
  const uint32_t* chunk_file;  // [m]
  const uint64_t* chunk_len;   // [m]
  const int64_t* rep;          // [m]
  const int64_t* family;       // [n]
  uint32_t m, n;
};

// each may be null; the set arrays hold n / 2 entries, of which the first `sets` are written
struct FamilyBytesOut {
  uint64_t *file_bytes, *delta_bytes, *self_bytes, *inherited_bytes;  // [n]
  int64_t* set_rep;
  uint32_t* set_files;
  uint64_t *set_total, *set_stored;
};

// ws: family_bytes_layout(in.m, in.n).bytes, 16-byte aligned. m, n <= 2^30.
// counts (u64[kFamilyBytesCounts], overwritten) may be null. Enqueues on st and
// never waits: every grid is sized from m or n, the number of merge passes is
// ceil_log2(n).
hipError_t family_bytes(uint8_t* ws, const FamilyBytesIn& in, const FamilyBytesOut& out, unsigned long long* counts,
                        hipStream_t st);

}  // namespace sdcas
