// family_store.h — the family store (family_store.hip): where every op of the
// family recipes finds its bytes in one dense store of the literal ranges, and
// the byte mover that packs the store from file windows and restores windows
// from it. include/sdcas.h has the public definition; this is the workspace
// and the device calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

constexpr uint64_t kFamilyStoreMaxOps = 1ull << 30;
constexpr uint64_t kFamilyStoreMaxFiles = 1ull << 30;
constexpr uint32_t kFamilyStoreLayoutCounts = 6;  // sdcas_family_store_counts' words
constexpr uint32_t kFamilyStoreMoveCounts = 4;    // sdcas_family_move_counts' words
constexpr uint64_t kFamilyStoreNone = ~0ull;

// The mover's tile: this many destination bytes, cut at 16-byte aligned
// destination addresses, one workgroup of kFamilyStoreTB threads at a time and
// kFamilyStorePer 16-byte units per thread.
constexpr uint32_t kFamilyStoreTB = 256;
constexpr uint32_t kFamilyStorePer = 2;
constexpr uint32_t kFamilyStoreTile = kFamilyStoreTB * kFamilyStorePer * 16;
// the mover's grid: a constant number of workgroups, each with a contiguous share of the tiles
constexpr uint32_t kFamilyStoreGrid = 256 * 8;
// the counters as they add up: copies of a 128-byte line, as family_recipes.h keeps them
constexpr uint32_t kFamilyStoreScCopies = 64;

// the workgroups of kFamilyStoreTB ops, each with a sum that the scan turns into an offset
inline uint64_t family_store_groups(uint64_t max_ops) { return (max_ops + kFamilyStoreTB - 1) / kFamilyStoreTB; }

// The workspace for max_ops ops, in bytes from its start (every part 16-byte
// aligned), shared by the layout and the mover. Filled with 0 before a call:
//   sc      u64[64][16]   the counts as they add up
// written before they are read:
//   tot     u64[2]        the scan's total: the store's bytes (layout), the tiles (mover)
//   gsum    u64[groups]   per workgroup of ops: its sum, then the sum before it
//   start   u64[max_ops]  mover: per op its tiles, then the tiles before it
//   dst     u64[max_ops]  mover: per op with a tile, where its clipped bytes go in the destination buffer
//   src     u64[max_ops]  mover: where they come from in the source buffer
//   len     u64[max_ops]  mover: how many they are
struct FamilyStoreLayout {
  uint64_t sc, tot, gsum, start, dst, src, len, bytes;
};
inline FamilyStoreLayout family_store_layout(uint64_t max_ops) {
  FamilyStoreLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.sc = take(8 * 16 * kFamilyStoreScCopies), l.tot = take(8 * 2);
  l.gsum = take(8 * family_store_groups(max_ops));
  l.start = take(8 * max_ops), l.dst = take(8 * max_ops), l.src = take(8 * max_ops), l.len = take(8 * max_ops);
  l.bytes = o;
  return l;
}

// sdcas_dev_family_recipes' op arrays; op_chunk and op_src_chunk say which op is a literal
struct FamilyStoreOps {
  const uint32_t *op_chunk, *op_src_chunk, *op_row, *op_src_row;
  const uint64_t *op_dst_off, *op_src_off, *op_len;
  const uint64_t* d_ops;  // device: the number of ops; the calls use min(*d_ops, max_ops)
  uint32_t max_ops;
};

// ws: family_store_layout(max_ops).bytes, 16-byte aligned. chunk_op[m]. counts
// (u64[kFamilyStoreLayoutCounts], overwritten) and store_off may be null.
// Enqueues on st and never waits.
hipError_t family_store_offsets(uint8_t* ws, const FamilyStoreOps& ops, const uint32_t* chunk_op, uint32_t m,
                                uint64_t* store_off, unsigned long long* counts, hipStream_t st);

struct FamilyStoreRows {
  const uint64_t *row_at, *row_base, *row_len;  // row_base may be null: zeros
  uint32_t n;
};

// The mover. restore == false: blob -> store, literal ops only (op_src_row,
// op_src_off unused); true: store -> blob, every op with a store offset.
// counts (u64[kFamilyStoreMoveCounts], overwritten) may be null. Enqueues on st
// and never waits; the grid of the copy is kFamilyStoreGrid workgroups whatever
// the data.
hipError_t family_store_move(uint8_t* ws, const FamilyStoreOps& ops, const uint64_t* store_off,
                             const FamilyStoreRows& rows, uint8_t* blob, uint64_t blob_bytes, uint8_t* store,
                             uint64_t store_bytes, bool restore, unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
