// chunk_holders.hip — the holders index: the chunk index (chunk_index.hip) with
// every holder of a pair kept, so that a file's entries can be removed again.
//
// The entries are sorted by the triple (key, digest as 32 bytes in memcmp
// order, value), with the chunk index's directory over the keys' top bits. A
// pair's entries are a run, lowest value first; a run is not bounded by
// anything (every sparse file holds the all-zero chunk), so no thread here
// ever walks one: run ends are found by halving, orders by merging.
//   k_ch_match     one query per thread: its bucket, the lower bound of the
//                  pair, then the upper bound from there to the bucket's end
// The add, for a batch of m against n_old entries, every grid sized from m or
// n_old and the number of added triples left on the device:
//   k_ch_iota, k_ch_merge  the batch positions ordered by (valid first, triple,
//                  position): a merge sort by halving, one launch per doubling,
//                  so that equal triples are neighbours with the lowest
//                  position first
//   k_ch_head      per place in that order: the triple's lower bound in the
//                  old index, whether it is there, and whether the place is
//                  the first of a triple that is not; the new firsts counted
//                  per workgroup
//   k_ch_scan      the counts scanned, three levels of 256 (chunk_holders.h)
//   k_ch_place     a new first goes to its rank among the new firsts plus its
//                  lower bound; that rank also places every later copy and
//                  every hit, so pos and flags are written here, and the
//                  counts
//   index_place_old  an old entry goes to its index plus the number of new
//                  lower bounds that are <= it: the chunk index's kernel
//                  (chunk_index.hip: k_ix_place_old)
//   index_build_dir  one lower bound in the new keys per directory slot
//                  (k_ix_dir)
// The remove, one thread per old entry:
//   k_ch_rm_mark   membership of the entry's value in `removed` by halving;
//                  the waves' keep masks and the kept per workgroup
//   k_ch_scan      as above
//   k_ch_rm_scatter a kept entry goes to the kept before its workgroup plus
//                  its rank in it: the order is preserved
//   index_build_dir  the directory of what is left
// Every directory value is clamped to n, every computed place is checked
// against the arrays' bound before a store. The digest, the searches and the
// bucket are index_device.h's; the triple's order, the run searches, ch_rank,
// ch_base and the scan are holders_device.h's, shared with chunk_peers.hip.
#include <hip/hip_runtime.h>
#include <string.h>

#include "chunk_holders.h"
#include "holders_device.h"
#include "index_device.h"

namespace sdcas {

namespace {

constexpr uint32_t kChHitBit = 0x80000000u, kChNewBit = 0x40000000u, kChLbMask = 0x3FFFFFFFu;
constexpr uint8_t kChHit = 1, kChAdded = 2, kChSkipped = 4;  // SDCAS_INDEX_*

__global__ void __launch_bounds__(kChTB) k_ch_match(IndexView ix, const uint64_t* __restrict__ keys,
                                                    const uint8_t* __restrict__ digests,
                                                    const uint8_t* __restrict__ valid, uint32_t m,
                                                    int64_t* __restrict__ pos, uint64_t* __restrict__ value,
                                                    uint32_t* __restrict__ holders,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_cnt[kIndexMatchCounts];
  if (threadIdx.x < kIndexMatchCounts) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * kChTB + threadIdx.x;
  bool add[kIndexMatchCounts] = {false, false, false, false};  // queries, hits, misses, skipped
  if (c < m) {
    const bool take = !valid || valid[c];
    uint32_t first = 0, end = 0;
    if (take && ix.n) {
      const uint64_t key = keys[c];
      const IxDigest dig = ix_digest(digests, c);
      uint32_t lo, hi;
      ix_bucket(ix, key, lo, hi);
      first = ch_pair_bound(ix, lo, hi, key, dig, false);
      // the run's end lies in the same bucket: its entries share the key
      end = ch_pair_bound(ix, first, hi, key, dig, true);
    }
    const bool found = end > first;
    if (pos) pos[c] = found ? (int64_t)first : -1;
    if (value) value[c] = found && ix.values ? ix.values[first] : 0ull;
    if (holders) holders[c] = end - first;
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

__global__ void __launch_bounds__(kChTB) k_ch_iota(uint32_t* __restrict__ ord, uint32_t m) {
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  if (p < m) ord[p] = p;
}

// One pass of the merge sort over all m batch positions by (valid first,
// triple, position): a total order, so no two compare equal. `in` holds the
// positions in runs of w places, each run in order; every pair of neighbouring
// runs is merged into `out`. A position goes to its rank in its own run plus
// the number of the sibling run's positions before it, found by halving: at
// most 30 steps per thread and pass, whatever the data.
__global__ void __launch_bounds__(kChTB) k_ch_merge(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                    const uint64_t* __restrict__ keys,
                                                    const uint8_t* __restrict__ digests,
                                                    const uint64_t* __restrict__ values,
                                                    const uint8_t* __restrict__ valid, uint32_t w, uint32_t m) {
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  if (p >= m) return;
  const uint32_t c = in[p];
  if (c >= m) return;  // never: `in` holds batch positions
  const uint32_t first = p / (2 * w) * (2 * w);  // w <= 2^29: 2 w fits
  const uint32_t mid = ix_min(first + w, m), end = ix_min(first + 2 * w, m);
  const bool left = p < mid;
  uint32_t lo = left ? mid : first, hi = left ? end : mid;
  const uint32_t sib = lo;
  const bool vc = !valid || valid[c];
  const ChTriple t = ch_triple(keys, digests, values, c);
  while (lo < hi) {  // the sibling run's positions before c
    const uint32_t q = lo + ((hi - lo) >> 1);
    const uint32_t e = in[q];
    bool before = false;
    if (e < m) {  // always
      const bool ve = !valid || valid[e];
      if (ve != vc) {
        before = ve;
      } else if (!ve) {
        before = e < c;
      } else {
        const int r = ch_cmp3(keys, digests, values, e, t);
        before = r ? r < 0 : e < c;
      }
    }
    if (before) lo = q + 1;
    else hi = q;
  }
  const uint32_t at = first + (p - (left ? first : mid)) + (lo - sib);
  if (at < m) out[at] = c;  // always: a rank among the pair's end - first places
}

// lbf[p] for every place p of the order, the new firsts per workgroup into l1
__global__ void __launch_bounds__(kChTB) k_ch_head(IndexView old, const uint32_t* __restrict__ ord,
                                                   const uint64_t* __restrict__ keys,
                                                   const uint8_t* __restrict__ digests,
                                                   const uint64_t* __restrict__ values,
                                                   const uint8_t* __restrict__ valid, uint32_t m,
                                                   uint32_t* __restrict__ lbf, uint32_t* __restrict__ l1) {
  __shared__ uint32_t s_w[kChTB / 64];
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  bool fresh = false;
  if (p < m) {
    const uint32_t c = ord[p];
    uint32_t w = 0;
    if (c < m && (!valid || valid[c])) {
      const ChTriple t = ch_triple(keys, digests, values, c);
      bool found;
      const uint32_t lb = ch_lower_bound3(old, t, found);
      bool head = p == 0;
      if (!head) {  // the place before holds a valid position: those come first
        const uint32_t e = ord[p - 1];
        head = e >= m || ch_cmp3(keys, digests, values, e, t) != 0;
      }
      fresh = head && !found;
      w = (lb & kChLbMask) | (found ? kChHitBit : 0u) | (fresh ? kChNewBit : 0u);
    }
    lbf[p] = w;
  }
  uint32_t total;
  (void)ch_rank(fresh, s_w, &total);
  if (threadIdx.x == 0) l1[blockIdx.x] = total;
}

// The new firsts into the new index, their lower bounds compacted into lbs,
// pos and flags of every batch position, the four batch counts.
__global__ void __launch_bounds__(kChTB) k_ch_place(const uint32_t* __restrict__ ord, const uint32_t* __restrict__ lbf,
                                                    const uint32_t* __restrict__ l1, const uint32_t* __restrict__ l2,
                                                    const uint32_t* __restrict__ l3,
                                                    const uint64_t* __restrict__ keys,
                                                    const uint8_t* __restrict__ digests,
                                                    const uint64_t* __restrict__ values,
                                                    const uint8_t* __restrict__ valid, uint32_t m, IndexOut out,
                                                    uint32_t cap, uint32_t* __restrict__ lbs,
                                                    int64_t* __restrict__ pos, uint8_t* __restrict__ flags,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_w[kChTB / 64];
  __shared__ uint32_t s_cnt[4];
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  const uint32_t w = p < m ? lbf[p] : 0u;
  const bool fresh = (w & kChNewBit) != 0;
  uint32_t total;
  // the new firsts at places <= p
  const uint32_t upto = ch_base(l1, l2, l3, blockIdx.x) + ch_rank(fresh, s_w, &total) + (fresh ? 1u : 0u);
  bool add[4] = {false, false, false, false};  // queries, hits, added, batch_duplicates
  if (p < m) {
    const uint32_t c = ord[p];
    if (c < m) {  // always
      int64_t at = -1;
      uint8_t fl = kChSkipped;
      if (!valid || valid[c]) {
        const uint32_t lb = w & kChLbMask;
        add[0] = true;
        if (w & kChHitBit) {  // the new firsts before p stand before the old entry, no other does
          at = (int64_t)lb + upto;
          fl = kChHit, add[1] = true;
        } else if (upto) {  // always: the triple's first is a new first at or before p
          const uint32_t rank = upto - 1;
          at = (int64_t)lb + rank;
          fl = fresh ? kChAdded : 0, add[fresh ? 2 : 3] = true;
          if (fresh) {
            if (rank < m) lbs[rank] = lb;
            if (at < (int64_t)cap) {  // always with an index that is one: lb <= n_old, rank < m
              out.keys[at] = keys[c];
              ix_store(out.digests, (uint32_t)at, ix_digest(digests, c));
              out.values[at] = values ? values[c] : 0ull;
            }
          }
        }
      }
      if (pos) pos[c] = at;
      if (flags) flags[c] = fl;
    }
  }
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(add[q]));
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(&s_cnt[q], cnt);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// masks[4 b + wave]: the lanes whose entry stays; l1[b]: how many of workgroup b's do
__global__ void __launch_bounds__(kChTB) k_ch_rm_mark(const uint64_t* __restrict__ values, uint32_t n,
                                                      const uint64_t* __restrict__ removed, uint32_t r,
                                                      unsigned long long* __restrict__ masks,
                                                      uint32_t* __restrict__ l1) {
  __shared__ uint32_t s_w[kChTB / 64];
  const uint32_t i = blockIdx.x * kChTB + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const uint64_t v = values ? values[i] : 0ull;
    uint32_t lo = 0, hi = r;
    while (lo < hi) {  // the first of removed that is not below v
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (removed[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    keep = !(lo < r && removed[lo] == v);
  }
  const uint64_t bal = __ballot(keep);
  if ((threadIdx.x & 63) == 0) masks[(size_t)blockIdx.x * (kChTB / 64) + (threadIdx.x >> 6)] = bal;
  uint32_t total;
  (void)ch_rank(keep, s_w, &total);
  if (threadIdx.x == 0) l1[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kChTB) k_ch_rm_scatter(IndexView old, const unsigned long long* __restrict__ masks,
                                                         const uint32_t* __restrict__ l1,
                                                         const uint32_t* __restrict__ l2,
                                                         const uint32_t* __restrict__ l3, IndexOut out, uint32_t cap) {
  const uint32_t i = blockIdx.x * kChTB + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long* mk = masks + (size_t)blockIdx.x * (kChTB / 64);
  uint32_t before = 0;
#pragma unroll
  for (uint32_t w = 0; w < kChTB / 64; ++w) before += w < wave ? (uint32_t)__popcll(mk[w]) : 0u;
  const uint64_t bal = mk[wave];
  if (i >= old.n || !((bal >> lane) & 1ull)) return;
  const uint32_t at = ch_base(l1, l2, l3, blockIdx.x) + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
  if (at >= cap) return;  // never: a rank among at most n_old kept entries
  out.keys[at] = old.keys[i];
  ix_store(out.digests, at, ix_digest(old.digests, i));
  out.values[at] = old.values ? old.values[i] : 0ull;
}

// entries_old, removed, entries_new, values
__global__ void k_ch_rm_totals(const uint32_t* __restrict__ kept_p, uint32_t n_old, uint32_t r,
                               unsigned long long* __restrict__ counts) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const uint32_t kept = ix_min(*kept_p, n_old);
    counts[0] = n_old;
    counts[1] = n_old - kept;
    counts[2] = kept;
    counts[3] = r;
  }
}

}  // namespace

int holders_check(const uint64_t* keys, const uint8_t* digests, const uint64_t* values, const uint32_t* dir, uint64_t n,
                  uint32_t bits, uint64_t* bad) {
  for (uint64_t i = 1; i < n; ++i) {
    bool less = keys[i - 1] < keys[i];
    if (keys[i - 1] == keys[i]) {
      const int c = memcmp(digests + 32 * (i - 1), digests + 32 * i, 32);
      less = c < 0 || (c == 0 && values && values[i - 1] < values[i]);
    }
    if (!less) {
      *bad = i;
      return 1;
    }
  }
  return index_dir_check(keys, dir, n, bits, bad);
}

hipError_t holders_match(const IndexView& idx, const uint64_t* keys, const uint8_t* digests, const uint8_t* valid,
                         uint32_t m, int64_t* pos, uint64_t* value, uint32_t* holders, unsigned long long* counts,
                         hipStream_t st) {
  hipError_t e;
  if (counts && (e = hipMemsetAsync(counts, 0, kIndexMatchCounts * sizeof(unsigned long long), st))) return e;
  if (!pos && !value && !holders && !counts) return hipSuccess;
  hipLaunchKernelGGL(k_ch_match, dim3(index_blocks(m)), dim3(kChTB), 0, st, idx, keys, digests, valid, m, pos, value,
                     holders, counts);
  return hipGetLastError();
}

hipError_t holders_add(uint8_t* ws, const IndexView& old, const uint64_t* keys, const uint8_t* digests,
                       const uint64_t* values, const uint8_t* valid, uint32_t m, const IndexOut& out, int64_t* pos,
                       uint8_t* flags, unsigned long long* counts, hipStream_t st) {
  const HoldersAddLayout l = holders_add_layout(m);
  uint32_t* src = index_at<uint32_t>(ws, l.ord_a);
  uint32_t* dst = index_at<uint32_t>(ws, l.ord_b);
  uint32_t* lbf = index_at<uint32_t>(ws, l.lbf);
  uint32_t* lbs = index_at<uint32_t>(ws, l.lbs);
  uint32_t* l1 = index_at<uint32_t>(ws, l.scan.l1);
  uint32_t* l2 = index_at<uint32_t>(ws, l.scan.l2);
  uint32_t* l3 = index_at<uint32_t>(ws, l.scan.l3);
  uint32_t* na = index_at<uint32_t>(ws, l.scan.tot);
  unsigned long long* cts = index_at<unsigned long long>(ws, l.counts);
  const uint32_t cap = old.n + m;
  const dim3 block(kChTB), grid(index_blocks(m));
  hipError_t e;
  if ((e = hipMemsetAsync(na, 0, l.bytes - l.scan.tot, st))) return e;  // tot and counts
  if (m) {
    hipLaunchKernelGGL(k_ch_iota, grid, block, 0, st, src, m);
    for (uint64_t w = 1; w < m; w <<= 1) {
      hipLaunchKernelGGL(k_ch_merge, grid, block, 0, st, (const uint32_t*)src, dst, keys, digests, values, valid,
                         (uint32_t)w, m);
      uint32_t* t = src;
      src = dst, dst = t;
    }
    if ((e = hipGetLastError())) return e;
    hipLaunchKernelGGL(k_ch_head, grid, block, 0, st, old, (const uint32_t*)src, keys, digests, values, valid, m, lbf,
                       l1);
    ch_scan(ws, l.scan, st);
    hipLaunchKernelGGL(k_ch_place, grid, block, 0, st, (const uint32_t*)src, (const uint32_t*)lbf,
                       (const uint32_t*)l1, (const uint32_t*)l2, (const uint32_t*)l3, keys, digests, values, valid, m,
                       out, cap, lbs, pos, flags, cts);
    if ((e = hipGetLastError())) return e;
  }
  if (old.n) index_place_old(old, lbs, na, m, out, cap, st);
  index_build_dir(out.keys, old.n, na, m, out.bits, out.dir, st);
  if ((e = hipGetLastError())) return e;
  if (counts) {
    index_add_totals(na, m, old.n, cts, st);
    if ((e = hipGetLastError())) return e;
    return hipMemcpyAsync(counts, cts, kIndexAddCounts * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  }
  return hipSuccess;
}

hipError_t holders_remove(uint8_t* ws, const IndexView& old, const uint64_t* removed, uint32_t r, const IndexOut& out,
                          unsigned long long* counts, hipStream_t st) {
  const HoldersRemoveLayout l = holders_remove_layout(old.n);
  unsigned long long* masks = index_at<unsigned long long>(ws, l.masks);
  uint32_t* l1 = index_at<uint32_t>(ws, l.scan.l1);
  uint32_t* l2 = index_at<uint32_t>(ws, l.scan.l2);
  uint32_t* l3 = index_at<uint32_t>(ws, l.scan.l3);
  uint32_t* kept = index_at<uint32_t>(ws, l.scan.tot);
  unsigned long long* cts = index_at<unsigned long long>(ws, l.counts);
  const dim3 block(kChTB), grid(index_blocks(old.n));
  hipError_t e;
  if ((e = hipMemsetAsync(kept, 0, l.bytes - l.scan.tot, st))) return e;  // tot and counts
  if (old.n) {
    hipLaunchKernelGGL(k_ch_rm_mark, grid, block, 0, st, old.values, old.n, removed, r, masks, l1);
    ch_scan(ws, l.scan, st);
    hipLaunchKernelGGL(k_ch_rm_scatter, grid, block, 0, st, old, (const unsigned long long*)masks,
                       (const uint32_t*)l1, (const uint32_t*)l2, (const uint32_t*)l3, out, old.n);
    if ((e = hipGetLastError())) return e;
  }
  index_build_dir(out.keys, 0u, kept, old.n, out.bits, out.dir, st);
  if ((e = hipGetLastError())) return e;
  if (counts) {
    hipLaunchKernelGGL(k_ch_rm_totals, dim3(1), dim3(64), 0, st, (const uint32_t*)kept, old.n, r, cts);
    if ((e = hipGetLastError())) return e;
    return hipMemcpyAsync(counts, cts, kHoldersRemoveCounts * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  }
  return hipSuccess;
}

}  // namespace sdcas
