// family_forget.h — a family store that forgets rows (family_forget.hip): the
// chunk arrays of the rows that stay, renumbered, with their classes and labels
// elected again, and the byte ranges that carry the old store's bytes into the
// new one. include/sdcas.h has the public definition; this is the workspace and
// the two device calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

constexpr uint64_t kFamilyForgetMax = 1ull << 30;  // chunks, rows, ops
constexpr uint32_t kFamilyKeepCounts = 6;          // sdcas_family_keep_counts' words
constexpr uint32_t kFamilyMovesCounts = 6;         // sdcas_family_moves_counts' words
constexpr uint32_t kFamilyForgetTB = 256;
// the counters as they add up: copies of a 128-byte line, as family_recipes.h keeps them
constexpr uint32_t kFamilyForgetScCopies = 64;

// the workgroups of kFamilyForgetTB rows or chunks, each with a count that the scan turns into an offset
inline uint64_t family_forget_groups(uint64_t k) { return (k + kFamilyForgetTB - 1) / kFamilyForgetTB; }

// keep's workspace for m chunks of n rows, in bytes from its start (every part
// 16-byte aligned). Filled with 0xFF before a call:
//   rtab       u32[m]        per class number r: its lowest surviving chunk
//   ltab       u32[n]        per label: its lowest kept row that takes part
// filled with 0 before a call:
//   sc         u64[64][16]   the counts as they add up
//   tot        u32[4]        the scans' totals: the rows kept, the chunks kept
// written before they are read:
//   row_new    u32[n]        per row: its new number, or none
//   chunk_new  u32[m]        per chunk: its new position, or none
//   rcnt       u32[groups(n)]  per workgroup of rows: the kept, then the kept before it
//   ccnt       u32[groups(m)]  the same for the chunks
struct FamilyKeepLayout {
  uint64_t rtab, ltab, sc, tot, row_new, chunk_new, rcnt, ccnt, bytes;
};
// moves' workspace for max_chunks new chunks. Filled with 0 before a call:
//   sc, tot    as above; tot[0] the moves
// written before they are read:
//   at         u64[max_chunks]  per new chunk: old_at, or none (also for a chunk that is no literal)
//   start      u64[max_chunks]  per move: its head's old_at
//   flag       u8[max_chunks]   per new chunk: 0 no part of a move, 1 a head, 2 continues the chunk below
//   gcnt       u32[groups]      per workgroup of chunks: its heads, then the heads before it
struct FamilyMovesLayout {
  uint64_t sc, tot, at, start, flag, gcnt, bytes;
};
inline FamilyKeepLayout family_keep_layout(uint64_t m, uint64_t n) {
  FamilyKeepLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.rtab = take(4 * m), l.ltab = take(4 * n);
  l.sc = take(8 * 16 * kFamilyForgetScCopies), l.tot = take(4 * 4);
  l.row_new = take(4 * n), l.chunk_new = take(4 * m);
  l.rcnt = take(4 * family_forget_groups(n)), l.ccnt = take(4 * family_forget_groups(m));
  l.bytes = o;
  return l;
}
inline FamilyMovesLayout family_moves_layout(uint64_t max_chunks) {
  FamilyMovesLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.sc = take(8 * 16 * kFamilyForgetScCopies), l.tot = take(4 * 4);
  l.at = take(8 * max_chunks), l.start = take(8 * max_chunks), l.flag = take(max_chunks);
  l.gcnt = take(4 * family_forget_groups(max_chunks));
  l.bytes = o;
  return l;
}
// one buffer serves both calls
inline uint64_t family_forget_bytes(uint64_t m, uint64_t n) {
  const uint64_t a = family_keep_layout(m, n).bytes, b = family_moves_layout(m).bytes;
  return a > b ? a : b;
}

struct FamilyKeepIn {
  const uint32_t* chunk_file;  // [m]
  const uint64_t *chunk_off, *chunk_len;
  const int64_t* rep;
  const int64_t* family;  // [n]
  const uint8_t* keep;    // [n]
  uint32_t m, n;
};
// each may be null; the row arrays hold n entries and the chunk arrays m, of which the first n' and m' are written
struct FamilyKeepOut {
  uint32_t *row_new, *row_from;
  int64_t* family;
  uint32_t *chunk_from, *chunk_file;
  uint64_t *chunk_off, *chunk_len;
  int64_t* rep;
};

// ws: family_keep_layout(m, n).bytes, 16-byte aligned. counts
// (u64[kFamilyKeepCounts], overwritten) may be null. Enqueues on st and never
// waits: every grid is sized from m or n.
hipError_t family_chunks_keep(uint8_t* ws, const FamilyKeepIn& in, const FamilyKeepOut& out,
                              unsigned long long* counts, hipStream_t st);

struct FamilyMovesIn {
  // the old store's side: chunk arrays [m], op arrays [max_ops], the ops on the device
  const uint64_t* chunk_off;
  const uint32_t* chunk_op;
  uint32_t m;
  const uint64_t *op_dst_off, *op_store_off, *d_ops;
  uint32_t max_ops;
  // the new store's side: chunk arrays [max_chunks], op arrays [max_nops], both numbers on the device
  const uint32_t* nchunk_from;
  const uint64_t *nchunk_off, *nchunk_len;
  const uint32_t* nchunk_op;
  const uint64_t* d_chunks;
  uint32_t max_chunks;
  const uint32_t *nop_chunk, *nop_src_chunk;
  const uint64_t *nop_dst_off, *nop_store_off, *d_nops;
  uint32_t max_nops;
};

// ws: family_moves_layout(max_chunks).bytes, 16-byte aligned. The move arrays
// hold max_chunks entries each and may be null, as may counts
// (u64[kFamilyMovesCounts], overwritten). Enqueues on st and never waits.
hipError_t family_store_moves(uint8_t* ws, const FamilyMovesIn& in, uint64_t* move_dst, uint64_t* move_src,
                              uint64_t* move_len, unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
