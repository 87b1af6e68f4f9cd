// chunk_index.hip — the persistent chunk index: a batch's (key, digest) pairs
// matched against, and merged into, the pairs stored by earlier batches.
//
// An index is sorted by (key, digest as 32 bytes in memcmp order) with a
// directory over the keys' top bits (chunk_index.h, include/sdcas.h). Nothing
// here hashes: a query reads one directory pair, then halves its bucket, one
// dependent read per step (the key; the 32 digest bytes as two 16-byte loads
// only where the key is equal). At the recommended width a bucket holds about 4
// entries, so a query costs about 4 dependent requests whatever n is; forged or
// skewed keys make long buckets, and those cost their logarithm.
//   k_ci_match     one query per thread: bucket, lower bound, compare. The add
//                  keeps the lower bound too (where a missing pair would go)
// The add, for a batch of m against n_old entries, every grid sized from m or
// n_old and the number of added pairs left on the device:
//   (confirm.hip)  rep[c]: the lowest batch position with c's pair
//   k_ci_match     against the old index
//   k_ci_select    the positions that are their pair's lowest and miss the old
//                  index, compacted (in any order: the pairs are distinct, so
//                  their sorted order is one)
//   (dupsets.hip)  the stable 8-bit LSD radix sort, by key
//   k_ci_fix       runs of one key ordered by the digest; a run above its cap
//                  (forged keys) raises a flag, and then k_ci_merge (a merge
//                  sort by all 40 bytes, one launch per doubling) and
//                  k_ci_take order everything again. That path is enqueued
//                  always and works on 0 items otherwise
//   k_ci_place_new an added pair goes to its rank plus its lower bound in the
//                  old index; the lower bounds, now ascending, are kept
//   k_ix_place_old an old entry goes to its index plus the number of kept
//                  lower bounds that are <= it: a search in a contiguous u32
//                  array, narrowed per workgroup to what its 256 entries span
//   k_ci_add_out   pos and flags per batch position, the counts
//   k_ix_dir       one lower bound in the new keys per directory slot
// Every directory value is clamped to n, every computed place is checked
// against the arrays' bound before a store.
// k_ix_place_old, k_ix_dir and k_ix_add_totals are the holders index's too
// (chunk_holders.hip): it reaches them through index_place_old,
// index_build_dir and index_add_totals, since a kernel cannot be launched
// from another file without relocatable device code. The digest, the searches
// and the bucket are index_device.h's.
#include <hip/hip_runtime.h>
#include <string.h>

#include "chunk_index.h"
#include "index_device.h"

namespace sdcas {

namespace {

constexpr uint32_t kCiTB = kIndexTB;
constexpr uint32_t kCiHitBit = 0x80000000u;
constexpr uint32_t kCiRunCap = 64;
constexpr uint8_t kCiHit = 1, kCiAdded = 2, kCiSkipped = 4;  // SDCAS_INDEX_*

// the first entry of [lo, hi) that is not below (key, dig); found: it is equal
__device__ __forceinline__ uint32_t ci_lower_bound(const uint64_t* __restrict__ keys,
                                                   const uint8_t* __restrict__ digests, uint32_t lo, uint32_t hi,
                                                   uint64_t key, const IxDigest& dig, bool& found) {
  found = false;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t k = keys[mid];
    bool below;
    if (k != key) {
      below = k < key;
    } else {
      const int c = ix_cmp(ix_digest(digests, mid), dig);
      if (c == 0) {
        found = true;
        return mid;
      }
      below = c < 0;
    }
    if (below) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// pos / value / counts: the match's outputs; mlb: the add's (the lower bound,
// with kCiHitBit when the pair is there; 0 for a skipped query)
__global__ void __launch_bounds__(kCiTB) k_ci_match(IndexView ix, const uint64_t* __restrict__ keys,
                                                    const uint8_t* __restrict__ digests,
                                                    const uint8_t* __restrict__ valid, uint32_t m,
                                                    int64_t* __restrict__ pos, uint64_t* __restrict__ value,
                                                    uint32_t* __restrict__ mlb,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_cnt[kIndexMatchCounts];
  if (threadIdx.x < kIndexMatchCounts) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * kCiTB + threadIdx.x;
  bool add[kIndexMatchCounts] = {false, false, false, false};  // queries, hits, misses, skipped
  if (c < m) {
    const bool take = !valid || valid[c];
    bool found = false;
    uint32_t at = 0;
    if (take && ix.n) {
      const uint64_t key = keys[c];
      const IxDigest dig = ix_digest(digests, c);
      uint32_t lo, hi;
      ix_bucket(ix, key, lo, hi);
      at = ci_lower_bound(ix.keys, ix.digests, lo, hi, key, dig, found);
    }
    if (pos) pos[c] = found ? (int64_t)at : -1;
    if (value) value[c] = found && ix.values ? ix.values[at] : 0ull;
    if (mlb) mlb[c] = at | (found ? kCiHitBit : 0u);
    add[0] = take, add[1] = found, add[2] = take && !found, add[3] = !take;
  }
  if (!counts) return;  // the same for every thread of the grid
#pragma unroll
  for (uint32_t w = 0; w < kIndexMatchCounts; ++w) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(add[w]));
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(&s_cnt[w], cnt);
  }
  __syncthreads();
  if (threadIdx.x < kIndexMatchCounts && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// (key, position) of every batch position that is the lowest with its pair and
// whose pair the old index lacks; *na <- how many. One atomic per wave.
__global__ void __launch_bounds__(kCiTB) k_ci_select(const int64_t* __restrict__ rep,
                                                     const uint32_t* __restrict__ mlb,
                                                     const uint64_t* __restrict__ keys, uint32_t m,
                                                     uint64_t* __restrict__ key_a, uint32_t* __restrict__ val_a,
                                                     uint32_t* __restrict__ na) {
  const uint32_t c = blockIdx.x * kCiTB + threadIdx.x;
  const bool f = c < m && rep[c] == (int64_t)c && !(mlb[c] & kCiHitBit);
  const uint64_t bal = __ballot(f);
  if (bal == 0) return;  // uniform over the wave
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t leader = (uint32_t)__builtin_ctzll(bal);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(na, (uint32_t)__popcll(bal));
  base = __shfl(base, leader);
  if (f) {
    const uint32_t at = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (at < m) {  // always: at most m positions are selected
      key_a[at] = keys[c];
      val_a[at] = c;
    }
  }
}

// vals: the added positions sorted by key, skeys: their keys. A position alone
// with its key keeps its place; one of a run of at most kCiRunCap goes to the
// run's start plus the number of the run's digests below its own (the pairs
// are distinct). A longer run is not ordered here: its positions raise
// *long_run. Every thread's work is bounded by 2 * kCiRunCap steps.
__global__ void __launch_bounds__(kCiTB) k_ci_fix(const uint32_t* __restrict__ vals,
                                                  const uint64_t* __restrict__ skeys,
                                                  const uint8_t* __restrict__ digests, uint32_t m,
                                                  const uint32_t* __restrict__ na_p, uint32_t* __restrict__ ord,
                                                  uint32_t* __restrict__ long_run) {
  const uint32_t na = ix_min(*na_p, m);
  const uint32_t p = blockIdx.x * kCiTB + threadIdx.x;
  if (p >= na) return;
  const uint32_t c = vals[p];
  if (c >= m) return;  // never: vals holds batch positions
  const uint64_t key = skeys[p];
  uint32_t lo = p, hi = p;
  bool too_long = false;
  while (lo > 0 && skeys[lo - 1] == key) {
    --lo;
    if (p - lo >= kCiRunCap) {
      too_long = true;
      break;
    }
  }
  while (!too_long && hi + 1 < na && skeys[hi + 1] == key) {
    ++hi;
    too_long = hi - lo + 1 > kCiRunCap;
  }
  if (too_long) {  // every position of such a run comes here
    if (__hip_atomic_load(long_run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(long_run, 1u);
    return;
  }
  uint32_t below = 0;
  if (hi != lo) {
    const IxDigest dig = ix_digest(digests, c);
    for (uint32_t q = lo; q <= hi; ++q) {
      const uint32_t e = vals[q];
      if (q != p && e < m) below += ix_cmp(ix_digest(digests, e), dig) < 0;
    }
  }
  ord[lo + below] = c;  // lo + below <= hi < na <= m
}

// *gate <- the number of added positions when k_ci_fix met a run it did not
// order, else 0: the number of items the long path's passes work on
__global__ void k_ci_gate(const uint32_t* __restrict__ long_run, const uint32_t* __restrict__ na_p, uint32_t m,
                          uint32_t* __restrict__ gate) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *gate = *long_run ? ix_min(*na_p, m) : 0u;
}

// The long path: one pass of a merge sort by (key, digest) over the first
// *gate places. `in` holds batch positions in runs of w places, each run in
// order; every pair of neighbouring runs is merged into `out`. A position goes
// to its rank in its own run plus the number of the sibling run's pairs below
// its own, found by halving (the pairs are distinct, so no two compare equal
// and the merge needs no tie rule). ceil_log2(m) passes from w = 1 order
// everything; each thread's work in a pass is bounded by 30 steps.
__global__ void __launch_bounds__(kCiTB) k_ci_merge(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                    const uint64_t* __restrict__ keys,
                                                    const uint8_t* __restrict__ digests, uint32_t w, uint32_t m,
                                                    const uint32_t* __restrict__ gate) {
  const uint32_t n = ix_min(*gate, m);
  const uint32_t p = blockIdx.x * kCiTB + threadIdx.x;
  if (p >= n) return;
  const uint32_t c = in[p];
  if (c >= m) return;  // never: `in` holds batch positions
  const uint32_t first = p / (2 * w) * (2 * w);  // w <= 2^29: 2 w fits
  const uint32_t mid = ix_min(first + w, n), end = ix_min(first + 2 * w, n);
  const bool left = p < mid;
  uint32_t lo = left ? mid : first, hi = left ? end : mid;
  const uint32_t sib = lo;
  const uint64_t key = keys[c];
  const IxDigest dig = ix_digest(digests, c);
  while (lo < hi) {  // the sibling run's pairs below (key, dig)
    const uint32_t q = lo + ((hi - lo) >> 1);
    const uint32_t e = in[q];
    bool below = false;
    if (e < m) {  // always
      const uint64_t k = keys[e];
      below = k != key ? k < key : ix_cmp(ix_digest(digests, e), dig) < 0;
    }
    if (below) lo = q + 1;
    else hi = q;
  }
  const uint32_t at = first + (p - (left ? first : mid)) + (lo - sib);
  if (at < n) out[at] = c;  // always: a rank among the pair's end - first places
}

// the long path's order replaces k_ci_fix's
__global__ void __launch_bounds__(kCiTB) k_ci_take(const uint32_t* __restrict__ gate,
                                                   const uint32_t* __restrict__ sorted, uint32_t m,
                                                   uint32_t* __restrict__ ord) {
  const uint32_t p = blockIdx.x * kCiTB + threadIdx.x;
  if (p < ix_min(*gate, m)) ord[p] = sorted[p];
}

__global__ void __launch_bounds__(kCiTB) k_ci_place_new(const uint32_t* __restrict__ ord,
                                                        const uint32_t* __restrict__ na_p,
                                                        const uint32_t* __restrict__ mlb,
                                                        const uint64_t* __restrict__ keys,
                                                        const uint8_t* __restrict__ digests,
                                                        const uint64_t* __restrict__ values, uint32_t m, IndexOut out,
                                                        uint32_t cap, uint32_t* __restrict__ npos,
                                                        uint32_t* __restrict__ lbs) {
  const uint32_t p = blockIdx.x * kCiTB + threadIdx.x;
  if (p >= ix_min(*na_p, m)) return;
  const uint32_t c = ord[p];
  if (c >= m) return;  // never
  const uint32_t lb = mlb[c] & ~kCiHitBit;
  const uint32_t at = p + lb;
  lbs[p] = lb;
  npos[c] = at;
  if (at >= cap) return;  // never with an index that is one: lb <= n_old, p < m
  out.keys[at] = keys[c];
  ix_store(out.digests, at, ix_digest(digests, c));
  out.values[at] = values ? values[c] : 0ull;
}

// Shared with the holders index (chunk_index.h: index_place_old)
__global__ void __launch_bounds__(kCiTB) k_ix_place_old(IndexView old, const uint32_t* __restrict__ lbs,
                                                        const uint32_t* __restrict__ na_p, uint32_t m, IndexOut out,
                                                        uint32_t cap) {
  __shared__ uint32_t s_span[2];
  const uint32_t na = ix_min(*na_p, m);
  const uint32_t first = blockIdx.x * kCiTB;
  if (threadIdx.x < 2) {
    const uint32_t v = threadIdx.x == 0 ? first : ix_min(first + kCiTB - 1, old.n - 1);
    s_span[threadIdx.x] = ix_upper(lbs, 0, na, v);
  }
  __syncthreads();
  const uint32_t i = first + threadIdx.x;
  if (i >= old.n) return;
  const uint32_t at = i + ix_upper(lbs, s_span[0], s_span[1], i);
  if (at >= cap) return;  // never: at most na <= m added entries stand before an old entry
  out.keys[at] = old.keys[i];
  ix_store(out.digests, at, ix_digest(old.digests, i));
  out.values[at] = old.values ? old.values[i] : 0ull;
}

__global__ void __launch_bounds__(kCiTB) k_ci_add_out(const int64_t* __restrict__ rep,
                                                      const uint32_t* __restrict__ mlb,
                                                      const uint32_t* __restrict__ npos,
                                                      const uint32_t* __restrict__ lbs,
                                                      const uint32_t* __restrict__ na_p, uint32_t m,
                                                      int64_t* __restrict__ pos, uint8_t* __restrict__ flags,
                                                      unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_cnt[4];
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t na = ix_min(*na_p, m);
  const uint32_t c = blockIdx.x * kCiTB + threadIdx.x;
  bool add[4] = {false, false, false, false};  // queries, hits, added, batch_duplicates
  if (c < m) {
    const int64_t r = rep[c];
    int64_t at = -1;
    uint8_t fl = kCiSkipped;
    if (r >= 0 && r <= (int64_t)c) {  // valid: confirm's rep is the lowest position with the pair
      const uint32_t w = mlb[c];
      add[0] = true;
      if (w & kCiHitBit) {
        const uint32_t i = w & ~kCiHitBit;
        at = (int64_t)i + ix_upper(lbs, 0, na, i);
        fl = kCiHit, add[1] = true;
      } else if (r == (int64_t)c) {
        at = npos[c];
        fl = kCiAdded, add[2] = true;
      } else {
        at = npos[(uint32_t)r];
        fl = 0, add[3] = true;
      }
    }
    if (pos) pos[c] = at;
    if (flags) flags[c] = fl;
  }
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(add[w]));
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(&s_cnt[w], cnt);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// entries_old, entries_new (index_add_totals)
__global__ void k_ix_add_totals(const uint32_t* __restrict__ na_p, uint32_t m, uint32_t n_old,
                                unsigned long long* __restrict__ counts) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    counts[4] = n_old;
    counts[5] = (unsigned long long)n_old + ix_min(*na_p, m);
  }
}

// dir[j] <- the number of the n = base + min(*extra_p, extra_max) entries
// whose key's top `bits` bits are below j (index_build_dir)
__global__ void __launch_bounds__(kCiTB) k_ix_dir(const uint64_t* __restrict__ nkeys, uint32_t base,
                                                  const uint32_t* __restrict__ extra_p, uint32_t extra_max,
                                                  uint32_t bits, uint32_t* __restrict__ dir) {
  const uint64_t j = (uint64_t)blockIdx.x * kCiTB + threadIdx.x;
  const uint64_t slots = 1ull << bits;
  if (j > slots) return;
  const uint32_t n = base + ix_min(*extra_p, extra_max);
  if (j == slots) {
    dir[j] = n;
    return;
  }
  if (j == 0) {
    dir[0] = 0;
    return;
  }
  const uint64_t thr = j << (64 - bits);  // bits >= 1 here: 0 < j < 2^bits
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (nkeys[mid] < thr) lo = mid + 1;
    else hi = mid;
  }
  dir[j] = lo;
}

// memcmp order of two host pairs
inline bool host_pair_less(uint64_t ka, const uint8_t* da, uint64_t kb, const uint8_t* db) {
  if (ka != kb) return ka < kb;
  return memcmp(da, db, 32) < 0;
}

}  // namespace

int index_check(const uint64_t* keys, const uint8_t* digests, const uint32_t* dir, uint64_t n, uint32_t bits,
                uint64_t* bad) {
  for (uint64_t i = 1; i < n; ++i) {
    if (!host_pair_less(keys[i - 1], digests + 32 * (i - 1), keys[i], digests + 32 * i)) {
      *bad = i;
      return 1;
    }
  }
  return index_dir_check(keys, dir, n, bits, bad);
}

int index_dir_check(const uint64_t* keys, const uint32_t* dir, uint64_t n, uint32_t bits, uint64_t* bad) {
  const uint64_t slots = 1ull << bits;
  uint64_t i = 0;  // the entries whose bucket is below j
  for (uint64_t j = 0; j <= slots; ++j) {
    if (j == slots) {
      i = n;
    } else if (bits) {
      while (i < n && (keys[i] >> (64 - bits)) < j) ++i;
    }
    if (dir[j] != i) {
      *bad = j;
      return 2;
    }
  }
  return 0;
}

void index_place_old(const IndexView& old, const uint32_t* lbs, const uint32_t* na_p, uint32_t m, const IndexOut& out,
                     uint32_t cap, hipStream_t st) {
  hipLaunchKernelGGL(k_ix_place_old, dim3(index_blocks(old.n)), dim3(kCiTB), 0, st, old, lbs, na_p, m, out, cap);
}

void index_build_dir(const uint64_t* nkeys, uint32_t base, const uint32_t* extra_p, uint32_t extra_max, uint32_t bits,
                     uint32_t* dir, hipStream_t st) {
  hipLaunchKernelGGL(k_ix_dir, dim3(index_blocks(index_dir_slots(bits))), dim3(kCiTB), 0, st, nkeys, base, extra_p,
                     extra_max, bits, dir);
}

void index_add_totals(const uint32_t* na_p, uint32_t m, uint32_t n_old, unsigned long long* cts, hipStream_t st) {
  hipLaunchKernelGGL(k_ix_add_totals, dim3(1), dim3(64), 0, st, na_p, m, n_old, cts);
}

hipError_t index_match(const IndexView& idx, const uint64_t* keys, const uint8_t* digests, const uint8_t* valid,
                       uint32_t m, int64_t* pos, uint64_t* value, unsigned long long* counts, hipStream_t st) {
  hipError_t e;
  if (counts && (e = hipMemsetAsync(counts, 0, kIndexMatchCounts * sizeof(unsigned long long), st))) return e;
  if (!pos && !value && !counts) return hipSuccess;
  hipLaunchKernelGGL(k_ci_match, dim3(index_blocks(m)), dim3(kCiTB), 0, st, idx, keys, digests, valid, m, pos, value,
                     (uint32_t*)nullptr, counts);
  return hipGetLastError();
}

hipError_t index_add(uint8_t* ws, uint32_t* cf_ws, const IndexView& old, const uint64_t* keys, const uint8_t* digests,
                     const uint64_t* values, const uint8_t* valid, uint32_t m, const IndexOut& out, int64_t* pos,
                     uint8_t* flags, unsigned long long* counts, hipStream_t st) {
  const IndexAddLayout l = index_add_layout(m);
  int64_t* rep = index_at<int64_t>(ws, l.rep);
  uint32_t* mlb = index_at<uint32_t>(ws, l.mlb);
  uint32_t* npos = index_at<uint32_t>(ws, l.npos);
  uint64_t* key_a = index_at<uint64_t>(ws, l.key_a);
  uint64_t* key_b = index_at<uint64_t>(ws, l.key_b);
  uint32_t* val_a = index_at<uint32_t>(ws, l.val_a);
  uint32_t* val_b = index_at<uint32_t>(ws, l.val_b);
  uint32_t* ord = index_at<uint32_t>(ws, l.ord);
  uint32_t* lbs = index_at<uint32_t>(ws, l.lbs);
  uint32_t* hist = index_at<uint32_t>(ws, l.hist);
  uint32_t* bsum = index_at<uint32_t>(ws, l.bsum);
  uint32_t* tot = index_at<uint32_t>(ws, l.tot);
  unsigned long long* cts = index_at<unsigned long long>(ws, l.counts);
  uint32_t* na = tot + 0;
  uint32_t* long_run = tot + 1;
  uint32_t* gate = tot + 2;
  const uint32_t cap = old.n + m;
  const dim3 block(kCiTB), grid(index_blocks(m));
  hipError_t e;
  if ((e = hipMemsetAsync(tot, 0, l.bytes - l.tot, st))) return e;  // tot and counts
  if (m) {
    if ((e = confirm_duplicates(cf_ws, keys, digests, valid, m, rep, nullptr, nullptr, nullptr, st))) return e;
    hipLaunchKernelGGL(k_ci_match, grid, block, 0, st, old, keys, digests, valid, m, (int64_t*)nullptr,
                       (uint64_t*)nullptr, mlb, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_ci_select, grid, block, 0, st, (const int64_t*)rep, (const uint32_t*)mlb, keys, m, key_a,
                       val_a, na);
    if ((e = hipGetLastError())) return e;
    // 8 passes: the result is back in key_a / val_a
    if ((e = dupsets_sort_u64(key_a, key_b, val_a, val_b, m, na, 8, hist, bsum, tot + 3, st))) return e;
    hipLaunchKernelGGL(k_ci_fix, grid, block, 0, st, (const uint32_t*)val_a, (const uint64_t*)key_a, digests, m,
                       (const uint32_t*)na, ord, long_run);
    // The long path, enqueued always and working only when k_ci_fix met a run
    // above its cap (else on 0 places: its kernels return at once): a merge
    // sort of the positions by (key, digest), ceil_log2(m) passes of one
    // launch each, from val_a to val_b and back.
    hipLaunchKernelGGL(k_ci_gate, dim3(1), dim3(64), 0, st, (const uint32_t*)long_run, (const uint32_t*)na, m, gate);
    uint32_t* src = val_a;
    uint32_t* dst = val_b;
    for (uint64_t w = 1; w < m; w <<= 1) {
      hipLaunchKernelGGL(k_ci_merge, grid, block, 0, st, (const uint32_t*)src, dst, keys, digests, (uint32_t)w, m,
                         (const uint32_t*)gate);
      uint32_t* t = src;
      src = dst, dst = t;
    }
    hipLaunchKernelGGL(k_ci_take, grid, block, 0, st, (const uint32_t*)gate, (const uint32_t*)src, m, ord);
    hipLaunchKernelGGL(k_ci_place_new, grid, block, 0, st, (const uint32_t*)ord, (const uint32_t*)na,
                       (const uint32_t*)mlb, keys, digests, values, m, out, cap, npos, lbs);
    if ((e = hipGetLastError())) return e;
  }
  if (old.n) index_place_old(old, lbs, na, m, out, cap, st);
  if (m && (pos || flags || counts))
    hipLaunchKernelGGL(k_ci_add_out, grid, block, 0, st, (const int64_t*)rep, (const uint32_t*)mlb,
                       (const uint32_t*)npos, (const uint32_t*)lbs, (const uint32_t*)na, m, pos, flags, cts);
  index_build_dir(out.keys, old.n, na, m, out.bits, out.dir, st);
  if ((e = hipGetLastError())) return e;
  if (counts) {
    index_add_totals(na, m, old.n, cts, st);
    if ((e = hipGetLastError())) return e;
    return hipMemcpyAsync(counts, cts, kIndexAddCounts * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  }
  return hipSuccess;
}

}  // namespace sdcas
