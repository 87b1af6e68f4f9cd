// dirtree.h — directory digests (a Merkle tree over the entries of a scan) and
// the top-most duplicate rule (dirtree.hip; definitions in include/sdcas.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace sdcas {

constexpr uint64_t kTreeMaxEntries = 1ull << 30;  // entry indices are 32-bit
constexpr uint32_t kTreeMaxDepth = 4096;          // SDCAS_TREE_MAX_DEPTH
constexpr uint32_t kTreeCounts = 6;               // sdcas_tree_counts' / sdcas_top_counts' words
constexpr uint32_t kTreeDir = 1, kTreeIncomplete = 2, kTreeEmpty = 4;  // SDCAS_TREE_*
constexpr uint32_t kTopDup = 1, kTopNested = 2;                        // SDCAS_TOP_*
constexpr uint64_t kTreeHead = 16, kTreeRecord = 72;                   // M(d) = 16 + 72 k bytes

// ---- the shape, from the host arrays (GPU-free) --------------------------------
//
// Directories are ranked by (depth, entry index); everything the device needs
// to know about the shape is indexed by that rank, and prank[i] (1 + the rank
// of entry i's parent, 0 for a root) is both the second sort key and the way
// from a child to its directory's numbers. Sorted by (prank, name32) the
// children of directory rank r stand at [dir_cstart[r], dir_cstart[r] + dir_k[r]),
// and the children of one level's directories are one range of positions.
struct TreeShape {
  uint32_t n = 0, dirs = 0, roots = 0;
  uint32_t levels = 0;      // 1 + the largest depth of any entry (0: no entry)
  uint32_t dir_levels = 0;  // 1 + the largest depth of a directory (0: none)
  uint64_t largest_dir = 0;
  std::vector<uint32_t> depth;     // per entry
  std::vector<uint64_t> children;  // per entry: direct children
  std::vector<uint32_t> prank;     // per entry
  std::vector<uint32_t> dir_entry, dir_k, dir_cstart;  // per rank
  std::vector<uint32_t> dir_moff;     // per rank: M(d)'s offset in its level's blob, in 16-byte units
  std::vector<uint32_t> level_first;  // [dir_levels + 1]: the first rank of each depth
  std::vector<uint64_t> level_bytes;  // per depth: the blob's bytes
  std::vector<uint64_t> level_chunks; // per depth: BLAKE3 chunks of its messages
  uint32_t max_level_dirs = 0;
  uint64_t max_level_bytes = 0, max_level_chunks = 0;
};
enum TreeShapeError { kTreeOk = 0, kTreeInvalid = 1, kTreeCapacity = 2 };
// with_layout false: depth, children, levels and the checks only (sdcas_tree_plan)
TreeShapeError tree_shape(const int64_t* parent, const uint8_t* is_dir, size_t n, bool with_layout, TreeShape& out,
                          const char** why);

// ---- the device workspace of one tree_digests call ----------------------------
// byte offsets from its start, each 16-byte aligned
struct TreeLayout {
  uint64_t prank, dir_entry, dir_k, dir_cstart, dir_moff, is_dir, counts, nword;  // the uploaded part, contiguous
  uint64_t meta_bytes;
  uint64_t key_a, key_b, val_a, val_b, ord, hist, bsum, tot;
  uint64_t acc_bytes, acc_files, acc_flags;
  uint64_t offs, lens, tdig, blob;
  uint64_t bytes;
};
TreeLayout tree_layout(uint64_t n, uint64_t dirs, uint64_t max_level_dirs, uint64_t max_level_bytes);
// the uploaded part, written into host memory of l.meta_bytes bytes
void tree_meta_fill(const TreeShape& s, const uint8_t* is_dir, const TreeLayout& l, uint8_t* host);

// The passes around the per-level batch hash (which the caller enqueues between
// tree_level_gather and tree_level_finish: messages at ws + l.blob with the
// offsets / lengths at ws + l.offs / l.lens, digests to ws + l.tdig).
struct TreeArgs {
  uint8_t* ws;
  const uint8_t* name32;
  const uint64_t* sizes;
  uint64_t* keys;
  uint8_t* digests32;
  uint8_t* valid;
  uint64_t* tree_bytes;
  uint64_t* tree_files;
  uint8_t* flags;
};
// clears the accumulators, sorts the entries by (parent, name32) and writes the
// file entries' rollups and flags
hipError_t tree_begin(const TreeShape& s, const TreeLayout& l, const TreeArgs& a, hipStream_t st);
hipError_t tree_level_gather(const TreeShape& s, const TreeLayout& l, const TreeArgs& a, uint32_t depth,
                             hipStream_t st);
hipError_t tree_level_finish(const TreeShape& s, const TreeLayout& l, const TreeArgs& a, uint32_t depth,
                             hipStream_t st);

// ---- top-most duplicates -------------------------------------------------------
// ws: tree_top_ws_words(n) u32 words, 8-byte aligned; parent / rep device
// arrays; top_rep, flags and counts (u64[kTreeCounts], overwritten) may be null
inline uint64_t tree_top_ws_words(uint64_t n) { return 3 * ((n + 1) & ~1ull) + 2 * kTreeCounts; }
hipError_t tree_top(uint32_t* ws, const int64_t* parent, const int64_t* rep, uint32_t n, int64_t* top_rep,
                    uint8_t* flags, unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
