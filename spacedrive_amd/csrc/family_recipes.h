// family_recipes.h — the family recipes (family_recipes.hip): the byte ranges
// that rebuild every row from what its family stores, over family_bytes.hip's
// classes. include/sdcas.h has the public definition; this is the workspace
// and the one device call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "family_bytes.h"

namespace sdcas {

constexpr uint32_t kFamilyRecipesCounts = 8;  // sdcas_family_recipes_counts' words
// The counters are kept in this many copies of 16 words, one 128-byte line each; a workgroup adds to the copy of
// its number. With one copy, the five adds of each of m / 256 workgroups to one line were the call's largest
// part: 102 of 266 us at m = 2^20, whatever the data.
constexpr uint32_t kFamilyRecipesScCopies = 64;

// the workgroups of kFamilyBytesTB chunks, each with a count of op heads
inline uint64_t family_recipes_groups(uint64_t m) { return (m + kFamilyBytesTB - 1) / kFamilyBytesTB; }

// The workspace for m chunks of n rows, in bytes from its start (every part
// 16-byte aligned). Filled with 0xFF before a call:
//   table      u32[slots]  per slot: its class's lowest participating chunk
//   row_first  u32[n]      per row: its lowest op
// filled with 0 before a call:
//   row_ops    u32[n]      per row: its ops
//   sc         u64[64][16] the counts as they add up, in kFamilyRecipesScCopies copies
//   tot        u32[4]      the ops
// written before they are read:
//   slot       u32[m]      per chunk: its class's slot, or none; from k_fr_emit on: its op, or none
//   first      u32[m]      per chunk: f(c), or none
//   head       u8[m]       per chunk: it starts an op
//   gcnt       u32[groups] per workgroup: its heads, then the heads before it
//   op_start   u64[m]      per op: its head's chunk_off
struct FamilyRecipesLayout {
  uint64_t table, row_first, row_ops, sc, tot, slot, first, head, gcnt, op_start, bytes;
  uint64_t slots;
};
inline FamilyRecipesLayout family_recipes_layout(uint64_t m, uint64_t n) {
  FamilyRecipesLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.slots = family_bytes_slots(m);
  l.table = take(4 * l.slots), l.row_first = take(4 * n);
  l.row_ops = take(4 * n), l.sc = take(8 * 16 * kFamilyRecipesScCopies), l.tot = take(4 * 4);
  l.slot = take(4 * m), l.first = take(4 * m), l.head = take(m);
  l.gcnt = take(4 * family_recipes_groups(m)), l.op_start = take(8 * m);
  l.bytes = o;
  return l;
}

struct FamilyRecipesIn {
  FamilyBytesIn fb;           // chunk_file, chunk_len, rep [m]; family [n]; m, n
  const uint64_t* chunk_off;  // [m]
};

// each may be null; the op arrays hold m entries, of which the first `ops` are written
struct FamilyRecipesOut {
  uint32_t *op_chunk, *op_src_chunk, *op_row, *op_src_row;
  uint64_t *op_dst_off, *op_src_off, *op_len;
  uint32_t* chunk_op;                 // [m]
  uint32_t *row_ops, *row_first_op;   // [n]
};

// ws: family_recipes_layout(m, n).bytes, 16-byte aligned. m, n <= 2^30. counts
// (u64[kFamilyRecipesCounts], overwritten) may be null. Enqueues on st and never
// waits: every grid is sized from m or n, the number of ops stays on the device.
hipError_t family_recipes(uint8_t* ws, const FamilyRecipesIn& in, const FamilyRecipesOut& out,
                          unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
