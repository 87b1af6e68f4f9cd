// dirtree.hip — a digest per directory (a Merkle tree over the entries of a
// scan, one level at a time from the deepest up) and the rule that keeps only
// the top-most duplicates. Definitions: include/sdcas.h, DESIGN.md §3.4.
//
// The shape (parent, is_dir) is host data: tree_shape ranks the directories by
// (depth, index) and works out, per rank, where the directory's children stand
// once the entries are sorted by (parent rank, name32), and where its message
// M(d) lies in its level's blob. No grid is sized from a device value.
//   k_dt_keys      the sort keys: name32's first 8 bytes, big-endian
//   (dupsets.hip)  the stable radix sort on those 64 bits, k_dt_pkeys, then the
//                  stable sort on the parent rank
//   k_dt_fix       runs of equal (parent, 8-byte prefix) ordered by all 32
//                  bytes, then by index: each entry of a run of up to 64
//                  counts the entries of the run below it (runs of more than
//                  one entry do not occur in real trees)
//   k_dt_gate,     a longer run (forged names) is not ordered by k_dt_fix:
//   k_dt_wkeys,    the order is then made again by the same stable sort on all
//   k_dt_select    four 8-byte words of the names and the parent rank. These
//                  launches are always enqueued and do nothing otherwise
//   k_dt_files     the file entries' rollups and flags
// per level, deepest first:
//   k_dt_gather    one thread per child in child order: its 72-byte record
//                  into M(d), and its bytes / files / completeness added to
//                  its directory's accumulators (a wave whose children share
//                  one directory adds once)
//   k_dt_head      per directory: "SDTREE01" || le64(k), the message's offset
//                  and its length (0 for an incomplete directory: no byte of
//                  it is read or hashed)
//   (b3_batch.hip) the batch hash over the level's messages
//   k_dt_finish    per directory: T(d), the tree key, valid, the flags, the
//                  rollups and the counts
// Workgroups hand data to each other only across launches; within a launch the
// only shared words are integer atomics whose result does not depend on order.
#include <hip/hip_runtime.h>

#include <cstring>

#include "dirtree.h"
#include "dupsets.h"

namespace sdcas {

// ---- the shape (host) -------------------------------------------------------------

TreeShapeError tree_shape(const int64_t* parent, const uint8_t* is_dir, size_t n, bool with_layout, TreeShape& s,
                          const char** why) {
  static const char* none = "";
  if (!why) why = &none;
  s = TreeShape{};
  if (n > kTreeMaxEntries) return *why = "more than 2^30 entries", kTreeCapacity;
  s.n = (uint32_t)n;
  if (n == 0) return kTreeOk;
  if (!parent || !is_dir) return *why = "null parent or is_dir", kTreeInvalid;
  s.children.assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    const int64_t p = parent[i];
    if (p < -1 || p >= (int64_t)n) return *why = "a parent outside [-1, n)", kTreeInvalid;
    if (p < 0) {
      ++s.roots;
      continue;
    }
    if (!is_dir[p]) return *why = "a parent that is not a directory", kTreeInvalid;
    ++s.children[p];
  }
  // depths: walk up to the first entry whose depth is known, then back down
  constexpr uint32_t kUnset = 0xFFFFFFFFu, kOnPath = 0xFFFFFFFEu;
  s.depth.assign(n, kUnset);
  std::vector<uint32_t> path;
  uint64_t deepest = 0;
  for (size_t i = 0; i < n; ++i) {
    if (s.depth[i] != kUnset) continue;
    path.clear();
    int64_t at = (int64_t)i;
    while (at >= 0 && s.depth[at] == kUnset) {
      s.depth[at] = kOnPath;
      path.push_back((uint32_t)at);
      at = parent[at];
    }
    if (at >= 0 && s.depth[at] == kOnPath) return *why = "an entry that is its own ancestor", kTreeInvalid;
    uint64_t d = at < 0 ? 0 : (uint64_t)s.depth[at] + 1;
    for (size_t k = path.size(); k-- > 0; ++d) {
      // (the depth is stored clamped; `deepest` keeps the true one for the check below)
      s.depth[path[k]] = (uint32_t)(d < kOnPath ? d : kOnPath - 1);
      if (d > deepest) deepest = d;
    }
  }
  if (deepest + 1 > kTreeMaxDepth) return *why = "more than SDCAS_TREE_MAX_DEPTH levels", kTreeCapacity;
  s.levels = (uint32_t)deepest + 1;
  for (size_t i = 0; i < n; ++i) {
    if (!is_dir[i]) continue;
    ++s.dirs;
    if (s.children[i] > s.largest_dir) s.largest_dir = s.children[i];
    if (s.depth[i] + 1 > s.dir_levels) s.dir_levels = s.depth[i] + 1;
  }
  if (!with_layout) return kTreeOk;

  // ranks by (depth, index): a counting sort on the depth
  s.level_first.assign(s.dir_levels + 1, 0);
  for (size_t i = 0; i < n; ++i)
    if (is_dir[i]) ++s.level_first[s.depth[i] + 1];
  for (uint32_t d = 0; d < s.dir_levels; ++d) s.level_first[d + 1] += s.level_first[d];
  std::vector<uint32_t> next(s.level_first.begin(), s.level_first.end());
  std::vector<uint32_t> rank(n, 0);
  s.dir_entry.assign(s.dirs, 0);
  for (size_t i = 0; i < n; ++i) {
    if (!is_dir[i]) continue;
    const uint32_t r = next[s.depth[i]]++;
    rank[i] = r;
    s.dir_entry[r] = (uint32_t)i;
  }
  s.prank.assign(n, 0);
  for (size_t i = 0; i < n; ++i) s.prank[i] = parent[i] < 0 ? 0u : rank[parent[i]] + 1;
  s.dir_k.assign(s.dirs, 0);
  s.dir_cstart.assign(s.dirs, 0);
  s.dir_moff.assign(s.dirs, 0);
  s.level_bytes.assign(s.dir_levels, 0);
  s.level_chunks.assign(s.dir_levels, 0);
  uint64_t at = s.roots;
  for (uint32_t d = 0; d < s.dir_levels; ++d) {
    uint64_t units = 0, chunks = 0;
    for (uint32_t r = s.level_first[d]; r < s.level_first[d + 1]; ++r) {
      const uint64_t k = s.children[s.dir_entry[r]];
      const uint64_t len = kTreeHead + kTreeRecord * k;
      s.dir_k[r] = (uint32_t)k;
      s.dir_cstart[r] = (uint32_t)at;
      s.dir_moff[r] = (uint32_t)units;
      at += k;
      units += (len + 15) / 16;
      chunks += (len + 1023) / 1024;
    }
    s.level_bytes[d] = 16 * units;
    s.level_chunks[d] = chunks;
    const uint32_t nd = s.level_first[d + 1] - s.level_first[d];
    if (nd > s.max_level_dirs) s.max_level_dirs = nd;
    if (16 * units > s.max_level_bytes) s.max_level_bytes = 16 * units;
    if (chunks > s.max_level_chunks) s.max_level_chunks = chunks;
  }
  return kTreeOk;
}

TreeLayout tree_layout(uint64_t n, uint64_t dirs, uint64_t max_level_dirs, uint64_t max_level_bytes) {
  TreeLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  const uint64_t nt = dupsets_tiles(n);
  l.prank = take(4 * n), l.dir_entry = take(4 * dirs), l.dir_k = take(4 * dirs), l.dir_cstart = take(4 * dirs);
  l.dir_moff = take(4 * dirs), l.is_dir = take(n), l.counts = take(8 * kTreeCounts), l.nword = take(16);
  l.meta_bytes = o;
  l.key_a = take(8 * n), l.key_b = take(8 * n), l.val_a = take(4 * n), l.val_b = take(4 * n), l.ord = take(4 * n);
  l.hist = take(4 * 256 * nt), l.bsum = take(4 * ((uint64_t)dupsets_tiles(256 * nt) + 2)), l.tot = take(16);
  l.acc_bytes = take(8 * n), l.acc_files = take(4 * n), l.acc_flags = take(4 * n);
  l.offs = take(8 * max_level_dirs), l.lens = take(8 * max_level_dirs), l.tdig = take(32 * max_level_dirs);
  l.blob = take(max_level_bytes + 64);  // readable 64 B past every message's end
  l.bytes = o;
  return l;
}

void tree_meta_fill(const TreeShape& s, const uint8_t* is_dir, const TreeLayout& l, uint8_t* h) {
  memset(h, 0, l.meta_bytes);
  memcpy(h + l.prank, s.prank.data(), 4ull * s.n);
  memcpy(h + l.dir_entry, s.dir_entry.data(), 4ull * s.dirs);
  memcpy(h + l.dir_k, s.dir_k.data(), 4ull * s.dirs);
  memcpy(h + l.dir_cstart, s.dir_cstart.data(), 4ull * s.dirs);
  memcpy(h + l.dir_moff, s.dir_moff.data(), 4ull * s.dirs);
  memcpy(h + l.is_dir, is_dir, s.n);
  // sdcas_tree_counts: entries, dirs, complete_dirs, empty_dirs (both counted by k_dt_finish), levels, largest_dir
  const uint64_t counts[kTreeCounts] = {s.n, s.dirs, 0, 0, s.levels, s.largest_dir};
  memcpy(h + l.counts, counts, sizeof counts);
  memcpy(h + l.nword, &s.n, 4);
}

namespace {

constexpr uint32_t kDtTB = 256;
constexpr uint32_t kAccIncomplete = 1, kAccHasFile = 2;  // the accumulators' flag word

inline uint32_t dt_blocks(uint64_t m) { return m ? (uint32_t)((m + kDtTB - 1) / kDtTB) : 1u; }

template <typename T>
__device__ __forceinline__ T dt_wave_sum(T v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ uint32_t dt_wave_or(uint32_t v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v |= __shfl_xor(v, d);
  return v;
}

// the first 8 bytes of entry c's name digest as the u64 whose order is memcmp's
__device__ __forceinline__ uint64_t dt_prefix(const uint8_t* __restrict__ name32, uint32_t c) {
  return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(name32 + 32ull * c));
}

__global__ void __launch_bounds__(kDtTB) k_dt_keys(const uint8_t* __restrict__ name32, uint32_t n,
                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * kDtTB + threadIdx.x;
  if (i >= n) return;
  keys[i] = dt_prefix(name32, i);
  vals[i] = i;
}

// the second sort's keys: the parent rank of the entry at each position
// (gate non-null: only when *gate != 0)
__global__ void __launch_bounds__(kDtTB) k_dt_pkeys(const uint32_t* __restrict__ vals,
                                                    const uint32_t* __restrict__ prank, uint32_t n,
                                                    const uint32_t* __restrict__ gate, uint32_t* __restrict__ pk) {
  const uint32_t p = blockIdx.x * kDtTB + threadIdx.x;
  if (p >= n || (gate && *gate == 0)) return;
  const uint32_t c = vals[p];
  pk[p] = c < n ? prank[c] : 0u;  // c < n always: vals is a permutation of [0, n)
}

// The long-run path's keys, only when *gate != 0: 8-byte word w of the name
// digest of the entry at each position (vals null: position i holds entry i,
// and vals_out is set to that).
__global__ void __launch_bounds__(kDtTB) k_dt_wkeys(const uint32_t* __restrict__ vals,
                                                    const uint8_t* __restrict__ name32, uint32_t w, uint32_t n,
                                                    const uint32_t* __restrict__ gate, uint64_t* __restrict__ keys,
                                                    uint32_t* __restrict__ vals_out) {
  const uint32_t i = blockIdx.x * kDtTB + threadIdx.x;
  if (i >= n || *gate == 0) return;
  const uint32_t c = vals ? vals[i] : i;
  if (c >= n) return;  // never
  keys[i] = __builtin_bswap64(reinterpret_cast<const uint64_t*>(name32 + 32ull * c)[w]);
  if (!vals) vals_out[i] = i;
}

// *count <- n when k_dt_fix met a run it did not order, else 0: the number of
// items the long-run path's sorts work on
__global__ void k_dt_gate(const uint32_t* __restrict__ long_run, uint32_t n, uint32_t* __restrict__ count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *count = *long_run ? n : 0u;
}

// the long-run path's order replaces k_dt_fix's, only when *gate != 0
__global__ void __launch_bounds__(kDtTB) k_dt_select(const uint32_t* __restrict__ gate,
                                                     const uint32_t* __restrict__ sorted, uint32_t n,
                                                     uint32_t* __restrict__ ord) {
  const uint32_t p = blockIdx.x * kDtTB + threadIdx.x;
  if (p < n && *gate != 0) ord[p] = sorted[p];
}

// entry a's name digest orders before entry b's (all 32 bytes, then the index)
__device__ __forceinline__ bool dt_name_less(const uint8_t* __restrict__ name32, uint32_t a, uint32_t b) {
  const uint64_t* x = reinterpret_cast<const uint64_t*>(name32 + 32ull * a);
  const uint64_t* y = reinterpret_cast<const uint64_t*>(name32 + 32ull * b);
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const uint64_t u = __builtin_bswap64(x[w]), v = __builtin_bswap64(y[w]);
    if (u != v) return u < v;
  }
  return a < b;
}

// ord_in: the entries sorted by (parent rank, 8-byte prefix), pk: the sorted
// parent ranks. An entry alone with its (rank, prefix) keeps its position; an
// entry of a run of at most kDtRunCap goes to the run's start plus the number
// of the run's entries that order before it. A longer run (forged names: real
// name digests do not share 8 bytes) is not ordered here: its entries set
// *long_run, and the whole order is then made again by sorting on all 32 bytes
// (tree_begin). Every thread's work is bounded by 2 * kDtRunCap comparisons.
constexpr uint32_t kDtRunCap = 64;

__global__ void __launch_bounds__(kDtTB) k_dt_fix(const uint32_t* __restrict__ ord_in,
                                                  const uint32_t* __restrict__ pk,
                                                  const uint8_t* __restrict__ name32, uint32_t n,
                                                  uint32_t* __restrict__ ord_out, uint32_t* __restrict__ long_run) {
  const uint32_t p = blockIdx.x * kDtTB + threadIdx.x;
  if (p >= n) return;
  const uint32_t c = ord_in[p];
  if (c >= n) return;  // never: ord_in is a permutation of [0, n)
  const uint32_t r = pk[p];
  const uint64_t pre = dt_prefix(name32, c);
  auto same = [&](uint32_t q) {
    const uint32_t e = ord_in[q];
    return pk[q] == r && e < n && dt_prefix(name32, e) == pre;
  };
  uint32_t lo = p, hi = p;
  bool too_long = false;
  while (lo > 0 && same(lo - 1)) {
    --lo;
    if (p - lo >= kDtRunCap) {
      too_long = true;
      break;
    }
  }
  while (!too_long && hi + 1 < n && same(hi + 1)) {
    ++hi;
    too_long = hi - lo + 1 > kDtRunCap;
  }
  if (too_long) {  // every entry of such a run comes here
    if (__hip_atomic_load(long_run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(long_run, 1u);
    return;
  }
  uint32_t below = p - lo;
  if (hi != lo) {
    below = 0;
    for (uint32_t q = lo; q <= hi; ++q)
      if (q != p) below += dt_name_less(name32, ord_in[q], c);
  }
  ord_out[lo + below] = c;  // lo + below <= hi < n
}

__global__ void __launch_bounds__(kDtTB) k_dt_files(const uint8_t* __restrict__ is_dir,
                                                    const uint64_t* __restrict__ sizes, uint32_t n,
                                                    uint64_t* __restrict__ tree_bytes,
                                                    uint64_t* __restrict__ tree_files, uint8_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * kDtTB + threadIdx.x;
  if (i >= n || is_dir[i]) return;
  if (tree_bytes) tree_bytes[i] = sizes ? sizes[i] : 0ull;
  if (tree_files) tree_files[i] = 1;
  if (flags) flags[i] = 0;
}

// Positions [pos_lo, pos_hi) of the sorted order: the children of one level's
// directories, directory by directory, in child order.
__global__ void __launch_bounds__(kDtTB) k_dt_gather(
    const uint32_t* __restrict__ ord, uint32_t pos_lo, uint32_t pos_hi, uint32_t n, uint32_t dirs,
    const uint32_t* __restrict__ prank, const uint32_t* __restrict__ dir_entry, const uint32_t* __restrict__ dir_k,
    const uint32_t* __restrict__ dir_cstart, const uint32_t* __restrict__ dir_moff,
    const uint8_t* __restrict__ is_dir, const uint8_t* __restrict__ name32, const uint8_t* __restrict__ digests32,
    const uint8_t* __restrict__ valid, const uint64_t* __restrict__ sizes, uint64_t blob_bytes,
    uint8_t* __restrict__ blob, unsigned long long* __restrict__ acc_bytes, uint32_t* __restrict__ acc_files,
    uint32_t* __restrict__ acc_flags) {
  const uint32_t p = pos_lo + blockIdx.x * kDtTB + threadIdx.x;
  bool act = p < pos_hi;
  uint32_t c = 0, r = 0xFFFFFFFFu, d = 0;
  unsigned long long bytes = 0;
  uint32_t files = 0, fl = 0;
  if (act) {
    c = ord[p];
    act = c < n;  // always
  }
  if (act) {
    r = prank[c] - 1;  // prank >= 1: a root is no child
    act = r < dirs;    // always, with a shape made for these arrays
  }
  if (act) {
    d = dir_entry[r];
    const uint32_t j = p - dir_cstart[r];
    const uint64_t at = 16ull * dir_moff[r] + kTreeHead + kTreeRecord * j;
    act = d < n && j < dir_k[r] && at + kTreeRecord <= blob_bytes;  // always
    if (act) {
      const bool dir = is_dir[c] != 0;
      if (dir) {
        fl = acc_flags[c], bytes = acc_bytes[c], files = acc_files[c];  // final: c's level ran before
      } else {
        const bool ok = valid ? valid[c] != 0 : true;
        fl = kAccHasFile | (ok ? 0u : kAccIncomplete);
        bytes = sizes ? sizes[c] : 0ull;
        files = 1;
      }
      const uint4* nm = reinterpret_cast<const uint4*>(name32 + 32ull * c);
      const uint4* ct = reinterpret_cast<const uint4*>(digests32 + 32ull * c);
      const uint4 n0 = nm[0], n1 = nm[1], c0 = ct[0], c1 = ct[1];
      uint64_t* rec = reinterpret_cast<uint64_t*>(blob + at);  // 8-byte aligned
      rec[0] = (uint64_t)n0.x | (uint64_t)n0.y << 32, rec[1] = (uint64_t)n0.z | (uint64_t)n0.w << 32;
      rec[2] = (uint64_t)n1.x | (uint64_t)n1.y << 32, rec[3] = (uint64_t)n1.z | (uint64_t)n1.w << 32;
      rec[4] = (uint64_t)c0.x | (uint64_t)c0.y << 32, rec[5] = (uint64_t)c0.z | (uint64_t)c0.w << 32;
      rec[6] = (uint64_t)c1.x | (uint64_t)c1.y << 32, rec[7] = (uint64_t)c1.z | (uint64_t)c1.w << 32;
      rec[8] = dir ? 1ull : 0ull;
    }
  }
  // One directory over the whole wave (any directory of 64 children or more):
  // one add per word instead of 64 on the same word. Every lane takes part in
  // the votes and shuffles, active or not.
  const uint32_t r0 = __builtin_amdgcn_readfirstlane(r);
  if (__all(r == r0)) {
    bytes = dt_wave_sum(bytes);
    files = dt_wave_sum(files);
    fl = dt_wave_or(fl);
    if ((threadIdx.x & 63) != 0) act = false;
  }
  if (!act) return;
  atomicAdd(&acc_bytes[d], bytes);
  atomicAdd(&acc_files[d], files);
  if (fl) atomicOr(&acc_flags[d], fl);
}

// Ranks [r_lo, r_hi): one level's directories. After k_dt_gather, so that the
// accumulators are final.
__global__ void __launch_bounds__(kDtTB) k_dt_head(uint32_t r_lo, uint32_t r_hi, uint32_t n,
                                                   const uint32_t* __restrict__ dir_entry,
                                                   const uint32_t* __restrict__ dir_k,
                                                   const uint32_t* __restrict__ dir_moff,
                                                   const uint32_t* __restrict__ acc_flags, uint64_t blob_bytes,
                                                   uint8_t* __restrict__ blob, uint64_t* __restrict__ offs,
                                                   uint64_t* __restrict__ lens) {
  const uint32_t r = r_lo + blockIdx.x * kDtTB + threadIdx.x;
  if (r >= r_hi) return;
  const uint32_t d = dir_entry[r];
  const uint64_t at = 16ull * dir_moff[r], k = dir_k[r];
  const bool ok = d < n && at + kTreeHead + kTreeRecord * k <= blob_bytes;  // always
  const bool incomplete = !ok || (acc_flags[d] & kAccIncomplete);
  if (ok) {
    uint64_t* head = reinterpret_cast<uint64_t*>(blob + at);
    head[0] = 0x3130454552544453ull;  // "SDTREE01"
    head[1] = k;
  }
  offs[r - r_lo] = ok ? at : 0ull;
  lens[r - r_lo] = incomplete ? 0ull : kTreeHead + kTreeRecord * k;
}

__global__ void __launch_bounds__(kDtTB) k_dt_finish(
    uint32_t r_lo, uint32_t r_hi, uint32_t n, const uint32_t* __restrict__ dir_entry,
    const uint32_t* __restrict__ acc_flags, const unsigned long long* __restrict__ acc_bytes,
    const uint32_t* __restrict__ acc_files, const uint8_t* __restrict__ tdig, uint64_t* __restrict__ keys,
    uint8_t* __restrict__ digests32, uint8_t* __restrict__ valid, uint64_t* __restrict__ tree_bytes,
    uint64_t* __restrict__ tree_files, uint8_t* __restrict__ flags, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_sum[2];
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t r = r_lo + blockIdx.x * kDtTB + threadIdx.x;
  uint32_t complete = 0, empty = 0;
  if (r < r_hi) {
    const uint32_t d = dir_entry[r];
    if (d < n) {  // always
      const uint32_t fl = acc_flags[d];
      const bool inc = fl & kAccIncomplete;
      empty = !(fl & kAccHasFile);
      complete = !inc;
      uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0;
      if (!inc) {
        const uint4* t = reinterpret_cast<const uint4*>(tdig + 32ull * (r - r_lo));
        t0 = t[0], t1 = t[1];
      }
      uint4* out = reinterpret_cast<uint4*>(digests32 + 32ull * d);
      out[0] = t0, out[1] = t1;
      if (keys) keys[d] = __builtin_bswap64((uint64_t)t0.x | (uint64_t)t0.y << 32);
      if (valid) valid[d] = !inc && !empty;
      if (flags) flags[d] = (uint8_t)(kTreeDir | (inc ? kTreeIncomplete : 0u) | (empty ? kTreeEmpty : 0u));
      if (tree_bytes) tree_bytes[d] = acc_bytes[d];
      if (tree_files) tree_files[d] = acc_files[d];
    }
  }
  complete = dt_wave_sum(complete);
  empty = dt_wave_sum(empty);
  if ((threadIdx.x & 63) == 0) {
    if (complete) atomicAdd(&s_sum[0], complete);
    if (empty) atomicAdd(&s_sum[1], empty);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_sum[0]) atomicAdd(&counts[2], (unsigned long long)s_sum[0]);
    if (s_sum[1]) atomicAdd(&counts[3], (unsigned long long)s_sum[1]);
  }
}

// ---- top-most duplicates ---------------------------------------------------------

// the label of entry i when it takes part and at least two entries carry it
__device__ __forceinline__ bool tt_dup(const int64_t* __restrict__ rep, uint32_t n, uint32_t i,
                                       const uint32_t* __restrict__ cnt, uint32_t& label) {
  const int64_t v = rep[i];
  if (v < 0 || (uint64_t)v >= (uint64_t)n) return false;
  label = (uint32_t)v;
  return cnt[label] >= 2;
}
// DUP and NESTED of entry i < n; a parent outside [0, n) is no parent
__device__ __forceinline__ uint32_t tt_flags(const int64_t* __restrict__ parent, const int64_t* __restrict__ rep,
                                             uint32_t n, uint32_t i, const uint32_t* __restrict__ cnt,
                                             uint32_t& label) {
  if (!tt_dup(rep, n, i, cnt, label)) return 0;
  const int64_t p = parent[i];
  uint32_t pl;
  if (p >= 0 && (uint64_t)p < (uint64_t)n && tt_dup(rep, n, (uint32_t)p, cnt, pl)) return kTopDup | kTopNested;
  return kTopDup;
}

// open[label] <- 1 when a carrier of the label is not nested (the word is
// read first: a label of 100 000 carriers sends a handful of atomics, not one each)
__global__ void __launch_bounds__(kDtTB) k_tt_mark(const int64_t* __restrict__ parent,
                                                   const int64_t* __restrict__ rep, uint32_t n,
                                                   const uint32_t* __restrict__ cnt, uint32_t* __restrict__ open) {
  const uint32_t i = blockIdx.x * kDtTB + threadIdx.x;
  if (i >= n) return;
  uint32_t label = 0;
  if (tt_flags(parent, rep, n, i, cnt, label) != kTopDup) return;
  if (__hip_atomic_load(&open[label], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(&open[label], 1u);
}

// counts [1..5]: dup_entries, nested_entries, top_entries, kept_classes, dropped_classes
__global__ void __launch_bounds__(kDtTB) k_tt_write(const int64_t* __restrict__ parent,
                                                    const int64_t* __restrict__ rep, uint32_t n,
                                                    const uint32_t* __restrict__ cnt,
                                                    const uint32_t* __restrict__ low,
                                                    const uint32_t* __restrict__ open, int64_t* __restrict__ top_rep,
                                                    uint8_t* __restrict__ flags,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_sum[5];
  if (threadIdx.x < 5) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kDtTB + threadIdx.x;
  uint32_t a[5] = {0, 0, 0, 0, 0};
  if (i < n) {
    uint32_t label = 0;
    const uint32_t f = tt_flags(parent, rep, n, i, cnt, label);
    const bool kept = f && open[label];
    if (flags) flags[i] = (uint8_t)f;
    if (top_rep) top_rep[i] = kept ? (int64_t)label : -1;
    a[0] = f != 0, a[1] = (f & kTopNested) != 0, a[2] = kept;
    if (f && low[label] == i) a[3] = kept, a[4] = !kept;
  }
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) {
    a[k] = dt_wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0 && a[k]) atomicAdd(&s_sum[k], a[k]);
  }
  __syncthreads();
  if (threadIdx.x < 5 && s_sum[threadIdx.x]) atomicAdd(&counts[1 + threadIdx.x], (unsigned long long)s_sum[threadIdx.x]);
}

template <typename T>
inline T* at(uint8_t* ws, uint64_t off) {
  return reinterpret_cast<T*>(ws + off);
}

}  // namespace

hipError_t tree_begin(const TreeShape& s, const TreeLayout& l, const TreeArgs& a, hipStream_t st) {
  const uint32_t n = s.n;
  hipError_t e;
  // acc_bytes | acc_files | acc_flags are adjacent
  if ((e = hipMemsetAsync(a.ws + l.acc_bytes, 0, l.offs - l.acc_bytes, st))) return e;
  const uint8_t* is_dir = a.ws + l.is_dir;
  if (a.tree_bytes || a.tree_files || a.flags)
    hipLaunchKernelGGL(k_dt_files, dim3(dt_blocks(n)), dim3(kDtTB), 0, st, is_dir, a.sizes, n, a.tree_bytes,
                       a.tree_files, a.flags);
  if (s.dirs == 0) return hipGetLastError();
  uint64_t* key_a = at<uint64_t>(a.ws, l.key_a);
  uint64_t* key_b = at<uint64_t>(a.ws, l.key_b);
  uint32_t* val_a = at<uint32_t>(a.ws, l.val_a);
  uint32_t* val_b = at<uint32_t>(a.ws, l.val_b);
  uint32_t* hist = at<uint32_t>(a.ws, l.hist);
  uint32_t* bsum = at<uint32_t>(a.ws, l.bsum);
  uint32_t* tot = at<uint32_t>(a.ws, l.tot);
  const uint32_t* nword = at<uint32_t>(a.ws, l.nword);
  if ((e = hipMemsetAsync(tot, 0, 16, st))) return e;  // [0] the scans' total, [1] long run met, [2] its sorts' count
  uint32_t* long_run = tot + 1;
  uint32_t* gate = tot + 2;
  uint32_t* ord = at<uint32_t>(a.ws, l.ord);
  const uint32_t* prank = at<const uint32_t>(a.ws, l.prank);
  const dim3 grid(dt_blocks(n)), block(kDtTB);
  hipLaunchKernelGGL(k_dt_keys, grid, block, 0, st, a.name32, n, key_a, val_a);
  if ((e = dupsets_sort_u64(key_a, key_b, val_a, val_b, n, nword, 8, hist, bsum, tot, st))) return e;
  // (8 passes: the result is in key_a / val_a; the key buffers now hold the parent ranks)
  uint32_t* pk_a = reinterpret_cast<uint32_t*>(key_a);
  uint32_t* pk_b = reinterpret_cast<uint32_t*>(key_b);
  hipLaunchKernelGGL(k_dt_pkeys, grid, block, 0, st, (const uint32_t*)val_a, prank, n, (const uint32_t*)nullptr, pk_a);
  uint32_t bits = 1;
  while (bits < 32 && (1ull << bits) <= (uint64_t)s.dirs) ++bits;  // ranks + 1 lie in [0, dirs]
  const uint32_t passes = (bits + 7) / 8;
  if ((e = dupsets_sort_u32(pk_a, pk_b, val_a, val_b, n, nword, passes, hist, bsum, tot, st))) return e;
  const bool odd = passes & 1;
  hipLaunchKernelGGL(k_dt_fix, grid, block, 0, st, (const uint32_t*)(odd ? val_b : val_a),
                     (const uint32_t*)(odd ? pk_b : pk_a), a.name32, n, ord, long_run);
  // The long-run path, enqueued always and working only when k_dt_fix met a
  // run above its cap (its sorts' item count is then n, else 0: their kernels
  // return at once): the same order from a stable sort on all 32 name bytes,
  // lowest word first, then on the parent rank.
  hipLaunchKernelGGL(k_dt_gate, dim3(1), dim3(64), 0, st, (const uint32_t*)long_run, n, gate);
  for (uint32_t w = 4; w-- > 0;) {
    hipLaunchKernelGGL(k_dt_wkeys, grid, block, 0, st, w == 3 ? (const uint32_t*)nullptr : (const uint32_t*)val_a,
                       a.name32, w, n, (const uint32_t*)gate, key_a, val_a);
    if ((e = dupsets_sort_u64(key_a, key_b, val_a, val_b, n, gate, 8, hist, bsum, tot, st))) return e;
  }
  hipLaunchKernelGGL(k_dt_pkeys, grid, block, 0, st, (const uint32_t*)val_a, prank, n, (const uint32_t*)gate, pk_a);
  if ((e = dupsets_sort_u32(pk_a, pk_b, val_a, val_b, n, gate, passes, hist, bsum, tot, st))) return e;
  hipLaunchKernelGGL(k_dt_select, grid, block, 0, st, (const uint32_t*)gate, (const uint32_t*)(odd ? val_b : val_a), n,
                     ord);
  return hipGetLastError();
}

hipError_t tree_level_gather(const TreeShape& s, const TreeLayout& l, const TreeArgs& a, uint32_t depth,
                             hipStream_t st) {
  const uint32_t r_lo = s.level_first[depth], r_hi = s.level_first[depth + 1];
  if (r_lo == r_hi) return hipSuccess;
  const uint32_t pos_lo = s.dir_cstart[r_lo], pos_hi = r_hi < s.dirs ? s.dir_cstart[r_hi] : s.n;
  const uint64_t blob_bytes = s.level_bytes[depth];
  uint8_t* blob = a.ws + l.blob;
  if (pos_hi > pos_lo)
    hipLaunchKernelGGL(k_dt_gather, dim3(dt_blocks(pos_hi - pos_lo)), dim3(kDtTB), 0, st,
                       at<const uint32_t>(a.ws, l.ord), pos_lo, pos_hi, s.n, s.dirs,
                       at<const uint32_t>(a.ws, l.prank), at<const uint32_t>(a.ws, l.dir_entry),
                       at<const uint32_t>(a.ws, l.dir_k), at<const uint32_t>(a.ws, l.dir_cstart),
                       at<const uint32_t>(a.ws, l.dir_moff), (const uint8_t*)(a.ws + l.is_dir), a.name32,
                       (const uint8_t*)a.digests32, (const uint8_t*)a.valid, a.sizes, blob_bytes, blob,
                       at<unsigned long long>(a.ws, l.acc_bytes), at<uint32_t>(a.ws, l.acc_files),
                       at<uint32_t>(a.ws, l.acc_flags));
  hipLaunchKernelGGL(k_dt_head, dim3(dt_blocks(r_hi - r_lo)), dim3(kDtTB), 0, st, r_lo, r_hi, s.n,
                     at<const uint32_t>(a.ws, l.dir_entry), at<const uint32_t>(a.ws, l.dir_k),
                     at<const uint32_t>(a.ws, l.dir_moff), at<const uint32_t>(a.ws, l.acc_flags), blob_bytes, blob,
                     at<uint64_t>(a.ws, l.offs), at<uint64_t>(a.ws, l.lens));
  return hipGetLastError();
}

hipError_t tree_level_finish(const TreeShape& s, const TreeLayout& l, const TreeArgs& a, uint32_t depth,
                             hipStream_t st) {
  const uint32_t r_lo = s.level_first[depth], r_hi = s.level_first[depth + 1];
  if (r_lo == r_hi) return hipSuccess;
  hipLaunchKernelGGL(k_dt_finish, dim3(dt_blocks(r_hi - r_lo)), dim3(kDtTB), 0, st, r_lo, r_hi, s.n,
                     at<const uint32_t>(a.ws, l.dir_entry), at<const uint32_t>(a.ws, l.acc_flags),
                     at<const unsigned long long>(a.ws, l.acc_bytes), at<const uint32_t>(a.ws, l.acc_files),
                     (const uint8_t*)(a.ws + l.tdig), a.keys, a.digests32, a.valid, a.tree_bytes, a.tree_files,
                     a.flags, at<unsigned long long>(a.ws, l.counts));
  return hipGetLastError();
}

hipError_t tree_top(uint32_t* ws, const int64_t* parent, const int64_t* rep, uint32_t n, int64_t* top_rep,
                    uint8_t* flags, unsigned long long* counts, hipStream_t st) {
  const uint64_t ne = ((uint64_t)n + 1) & ~1ull;
  uint32_t* cnt = ws;
  uint32_t* low = ws + ne;
  uint32_t* open = ws + 2 * ne;
  unsigned long long* cts = reinterpret_cast<unsigned long long*>(ws + 3 * ne);
  hipError_t e;
  if ((e = hipMemsetAsync(cnt, 0, ne * sizeof(uint32_t), st))) return e;
  if ((e = hipMemsetAsync(low, 0xFF, ne * sizeof(uint32_t), st))) return e;
  if ((e = hipMemsetAsync(open, 0, (ne + 2 * kTreeCounts) * sizeof(uint32_t), st))) return e;  // open and the counts
  if ((e = dupsets_label_counts(rep, n, cnt, low, cts, st))) return e;
  hipLaunchKernelGGL(k_tt_mark, dim3(dt_blocks(n)), dim3(kDtTB), 0, st, parent, rep, n, (const uint32_t*)cnt, open);
  hipLaunchKernelGGL(k_tt_write, dim3(dt_blocks(n)), dim3(kDtTB), 0, st, parent, rep, n, (const uint32_t*)cnt,
                     (const uint32_t*)low, (const uint32_t*)open, top_rep, flags, cts);
  if ((e = hipGetLastError())) return e;
  if (counts) return hipMemcpyAsync(counts, cts, kTreeCounts * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  return hipSuccess;
}

}  // namespace sdcas
