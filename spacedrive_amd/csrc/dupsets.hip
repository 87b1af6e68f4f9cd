// dupsets.hip — duplicate sets: the files that carry one label (rep[i], what
// sdcas_confirm_duplicates writes per file) grouped into sets of two or more,
// the sets ordered, their members listed ascending in compressed-row layout,
// with the bytes of one copy and the bytes the extra copies hold.
//
// Workgroups hand data to each other only across launches (count, then scan,
// then write); within a launch the only shared words are integer atomics whose
// result does not depend on their order. Every pass below is one tile of 4096
// items per workgroup of 256 (16 rounds of one item per thread, in index
// order, which is what keeps compactions and sorts stable).
//   k_ds_count        per label: how many files carry it, and the lowest one
//                     (combined per 1024 files in LDS before the global atomics)
//   k_ds_head_count,  ordered compaction of the files that are the lowest of a
//   k_ds_head_write   label with >= 2 files: the sets in set_rep order, their
//                     sort keys, and the counts (one atomic per counter per
//                     workgroup)
//   k_ds_hist,        one 8-bit digit of a stable LSD radix sort: per-tile
//   k_ds_scatter      digit histogram (digit-major), its scan, the scatter.
//                     u64 keys for the sets (the complement of the reclaimable
//                     bytes), u32 keys for the members (the final set rank)
//   k_ds_scan_reduce, exclusive scan of a long array: per-tile sums, the
//   k_ds_scan,        one-workgroup scan of those (wg_scan.h, shared with
//   k_ds_scan_apply   dist_dedup.hip), the tiles' own scans
//   k_ds_final        per set in final order: set_rep, set_bytes, its count,
//                     and its rank stored under its label
//   k_ds_offsets      the scanned counts as set_offsets
//   k_ds_mem_count,   ordered compaction of the files whose label is a set:
//   k_ds_mem_write    (final rank, file) pairs in file order, sorted by rank
//   k_ds_members_out  the sorted files as members
// Every value read from rep[] is checked against [0, n) before it indexes
// anything; the number of sets and of members stays on the device (grids are
// sized from their bounds n / 2 and n).
#include <hip/hip_runtime.h>

#include "dupsets.h"
#include "wg_scan.h"

namespace sdcas {

namespace {

constexpr uint32_t kDsTB = 256;
constexpr uint32_t kDsR = kDupsetsTile / kDsTB;
constexpr uint32_t kDsWaves = kDsTB / 64;

template <typename T>
__device__ __forceinline__ T ds_wave_sum(T v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the label of file i when it takes part (in [0, n)), else false
__device__ __forceinline__ bool ds_label(const int64_t* __restrict__ rep, uint32_t n, uint32_t i, uint32_t& label) {
  if (i >= n) return false;
  const int64_t v = rep[i];
  if (v < 0 || (uint64_t)v >= (uint64_t)n) return false;
  label = (uint32_t)v;
  return true;
}
// file i is the lowest file of a label that at least two files carry
__device__ __forceinline__ bool ds_is_head(const int64_t* __restrict__ rep, uint32_t n, uint32_t i,
                                           const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ low,
                                           uint32_t& label) {
  return ds_label(rep, n, i, label) && low[label] == i && cnt[label] >= 2;
}
// file i carries a label that at least two files carry
__device__ __forceinline__ bool ds_is_member(const int64_t* __restrict__ rep, uint32_t n, uint32_t i,
                                             const uint32_t* __restrict__ cnt, uint32_t& label) {
  return ds_label(rep, n, i, label) && cnt[label] >= 2;
}

// One round of an ordered compaction, called by the whole workgroup: the
// number of flagged threads below this one; `all` <- the workgroup's total.
__device__ __forceinline__ uint32_t ds_round_rank(bool f, uint32_t* ws, uint32_t& all) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t bal = __ballot(f);
  const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
  if (lane == 0) ws[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0;
  all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kDsWaves; ++w) {
    if (w < wave) before += ws[w];
    all += ws[w];
  }
  __syncthreads();
  return before + below;
}

// the workgroup's number of flagged items -> tcnt[blockIdx.x]
__device__ __forceinline__ void ds_tile_total(uint32_t c, uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t ws[kDsWaves];
  c = ds_wave_sum(c);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDsWaves; ++w) t += ws[w];
    tcnt[blockIdx.x] = t;
  }
}

// Per label: files and lowest file. A label that many files carry (the head of
// a Zipf corpus: 170 504 of 6.25 M files) would take one global atomic per file
// on ONE word, and those serialise (2.4 ms of that call's 2.9); so each
// workgroup first combines 1024 files at a time in an LDS table of 2048 slots
// (label, files, lowest file; open addressing, never more than half full).
// The lowest of those files with a label then sends the label's global add and
// min: the files that are alone with their own index as label (most of
// confirm's output) send theirs lane by lane to consecutive words, the shape
// global atomics are fast in (sent in slot order: 716 us against 396 us for
// 6.25 M files).
constexpr uint32_t kDsSub = 1024, kDsSlots = 2048, kDsNone = 0xFFFFFFFFu;

__global__ void __launch_bounds__(kDsTB) k_ds_count(const int64_t* __restrict__ rep, uint32_t n,
                                                    uint32_t* __restrict__ cnt, uint32_t* __restrict__ low,
                                                    unsigned long long* __restrict__ counts) {
  constexpr uint32_t kPer = kDsSub / kDsTB;
  __shared__ uint32_t t_lab[kDsSlots], t_cnt[kDsSlots], t_low[kDsSlots];
  __shared__ uint32_t s_files;
  if (threadIdx.x == 0) s_files = 0;
  const uint32_t lo = blockIdx.x * kDupsetsTile;
  uint32_t c = 0;
#pragma unroll 1
  for (uint32_t sub = 0; sub < kDupsetsTile; sub += kDsSub) {
    if (lo + sub >= n) break;  // uniform
    for (uint32_t k = threadIdx.x; k < kDsSlots; k += kDsTB) t_lab[k] = kDsNone, t_cnt[k] = 0, t_low[k] = kDsNone;
    __syncthreads();
    uint32_t slot[kPer];
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
      const uint32_t i = lo + sub + r * kDsTB + threadIdx.x;
      uint32_t label;
      slot[r] = kDsNone;
      if (!ds_label(rep, n, i, label)) continue;
      ++c;
      uint32_t h = (label * 0x9E3779B1u) >> 21;  // 11 bits
      for (;;) {
        uint32_t cur = __hip_atomic_load(&t_lab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == kDsNone) {
          cur = atomicCAS(&t_lab[h], kDsNone, label);
          if (cur == kDsNone) break;
        }
        if (cur == label) break;
        h = (h + 1) & (kDsSlots - 1);
      }
      atomicAdd(&t_cnt[h], 1u);
      atomicMin(&t_low[h], i);
      slot[r] = h;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
      const uint32_t i = lo + sub + r * kDsTB + threadIdx.x;
      const uint32_t h = slot[r];
      if (h == kDsNone || t_low[h] != i) continue;  // not the lowest of these files with its label
      const uint32_t label = t_lab[h];
      if (label >= n) continue;  // never: only checked labels enter the table
      atomicAdd(&cnt[label], t_cnt[h]);
      if (__hip_atomic_load(&low[label], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&low[label], i);
    }
    __syncthreads();
  }
  c = ds_wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_files, c);
  __syncthreads();
  if (threadIdx.x == 0 && s_files) atomicAdd(&counts[0], (unsigned long long)s_files);
}

__global__ void __launch_bounds__(kDsTB) k_ds_head_count(const int64_t* __restrict__ rep, uint32_t n,
                                                         const uint32_t* __restrict__ cnt,
                                                         const uint32_t* __restrict__ low,
                                                         uint32_t* __restrict__ tcnt) {
  const uint32_t lo = blockIdx.x * kDupsetsTile;
  uint32_t c = 0;
#pragma unroll 4
  for (uint32_t r = 0; r < kDsR; ++r) {
    uint32_t label;
    c += ds_is_head(rep, n, lo + r * kDsTB + threadIdx.x, cnt, low, label);
  }
  ds_tile_total(c, tcnt);
}

// one workgroup: tcnt[b] <- its exclusive prefix; *total <- the sum
__global__ void __launch_bounds__(1024) k_ds_scan(uint32_t* __restrict__ tcnt, uint32_t nb,
                                                  uint32_t* __restrict__ total) {
  wg_scan_exclusive_1024(tcnt, nb, total);
}

// The sets in set_rep order: set s's lowest file, files and label; for the
// order by reclaimable bytes its sort key and value (keys non-null); the
// counts [1..5]: sets, members, duplicate_files, reclaimable_bytes, largest_set.
__global__ void __launch_bounds__(kDsTB) k_ds_head_write(
    const int64_t* __restrict__ rep, const uint64_t* __restrict__ sizes, uint32_t n, const uint32_t* __restrict__ cnt,
    const uint32_t* __restrict__ low, const uint32_t* __restrict__ toff, const uint32_t* __restrict__ total,
    uint32_t* __restrict__ hd_file, uint32_t* __restrict__ hd_cnt, uint32_t* __restrict__ hd_label,
    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t ws[kDsWaves];
  __shared__ unsigned long long s_sum[3];  // sets, members, reclaimable
  __shared__ uint32_t s_max;
  const uint32_t b = blockIdx.x;
  const uint32_t mine = (b + 1 < gridDim.x ? toff[b + 1] : *total) - toff[b];
  if (mine == 0) return;  // uniform over the workgroup
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  if (threadIdx.x == 3) s_max = 0;
  const uint32_t lo = b * kDupsetsTile;
  uint32_t run = toff[b];
  uint32_t a_sets = 0, a_max = 0;
  unsigned long long a_members = 0, a_recl = 0;
#pragma unroll 1
  for (uint32_t r = 0; r < kDsR; ++r) {
    const uint32_t i = lo + r * kDsTB + threadIdx.x;
    uint32_t label = 0, all;
    const bool f = ds_is_head(rep, n, i, cnt, low, label);
    const uint32_t s = run + ds_round_rank(f, ws, all);
    if (f) {
      const uint32_t c = cnt[label];
      const uint64_t recl = (uint64_t)(c - 1) * (sizes ? sizes[i] : 0ull);
      hd_file[s] = i;
      hd_cnt[s] = c;
      hd_label[s] = label;
      if (keys) {
        keys[s] = ~recl;
        vals[s] = s;
      }
      ++a_sets;
      a_members += c;
      a_recl += recl;
      a_max = a_max > c ? a_max : c;
    }
    run += all;
  }
  a_sets = ds_wave_sum(a_sets);
  a_members = ds_wave_sum(a_members);
  a_recl = ds_wave_sum(a_recl);
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    const uint32_t o = __shfl_xor(a_max, d);
    a_max = a_max > o ? a_max : o;
  }
  if ((threadIdx.x & 63) == 0 && a_sets) {
    atomicAdd(&s_sum[0], (unsigned long long)a_sets);
    atomicAdd(&s_sum[1], a_members);
    atomicAdd(&s_sum[2], a_recl);
    atomicMax(&s_max, a_max);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&counts[1], s_sum[0]);
    atomicAdd(&counts[2], s_sum[1]);
    atomicAdd(&counts[3], s_sum[1] - s_sum[0]);
    atomicAdd(&counts[4], s_sum[2]);
    atomicMax(&counts[5], (unsigned long long)s_max);
  }
}

// ---- the stable radix sort, one 8-bit digit per pass -------------------------

// hist[d * gridDim.x + tile] <- the tile's items (of the first *m_p) with digit d
template <typename K>
__global__ void __launch_bounds__(kDsTB) k_ds_hist(const K* __restrict__ keys, const uint32_t* __restrict__ m_p,
                                                   uint32_t shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[257];  // [256]: the items past the end
  h[threadIdx.x] = 0;
  if (threadIdx.x == 0) h[256] = 0;
  __syncthreads();
  const uint32_t m = *m_p;
  const uint32_t lo = blockIdx.x * kDupsetsTile;
#pragma unroll 1
  for (uint32_t r = 0; r < kDsR; ++r) {
    if (lo + r * kDsTB >= m) break;  // uniform
    const uint32_t i = lo + r * kDsTB + threadIdx.x;
    const uint32_t d = i < m ? (uint32_t)(keys[i] >> shift) & 255u : 256u;
    // one digit over the whole wave (the high digits of small keys): one add
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    if (__all(d == d0)) {
      if ((threadIdx.x & 63) == 0) atomicAdd(&h[d0], 64u);
    } else {
      atomicAdd(&h[d], 1u);
    }
  }
  __syncthreads();
  hist[threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// hist scanned: the tile's items go to hist[d * gridDim.x + tile] onwards, in
// the order they stand in (round by round, wave by wave, lane by lane)
template <typename K>
__global__ void __launch_bounds__(kDsTB) k_ds_scatter(const K* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ m_p, uint32_t shift,
                                                      const uint32_t* __restrict__ hist, K* __restrict__ keys_out,
                                                      uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wc[kDsWaves][256];
  const uint32_t m = *m_p;
  const uint32_t lo = blockIdx.x * kDupsetsTile;
  if (lo >= m) return;  // uniform
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  base[tid] = hist[tid * gridDim.x + blockIdx.x];
#pragma unroll 1
  for (uint32_t r = 0; r < kDsR; ++r) {
    if (lo + r * kDsTB >= m) break;  // uniform
#pragma unroll
    for (uint32_t w = 0; w < kDsWaves; ++w) wc[w][tid] = 0;
    __syncthreads();
    const uint32_t i = lo + r * kDsTB + tid;
    const bool act = i < m;
    const K key = act ? keys[i] : (K)0;
    const uint32_t val = act ? vals[i] : 0u;
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    // the lanes of this wave that hold an item with the same digit
    uint64_t same = __ballot(act);
#pragma unroll
    for (uint32_t bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const uint64_t bal = __ballot(one);
      same &= one ? bal : ~bal;
    }
    const uint32_t below = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (act && below == 0) wc[wave][d] = (uint32_t)__popcll(same);
    __syncthreads();
    if (act) {
      uint32_t pos = base[d] + below;
#pragma unroll
      for (uint32_t w = 0; w < kDsWaves; ++w)
        if (w < wave) pos += wc[w][d];
      if (pos < m) {  // always, with a histogram of these keys
        keys_out[pos] = key;
        vals_out[pos] = val;
      }
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDsWaves; ++w) add += wc[w][tid];
    base[tid] += add;  // read again only after the next round's barrier
  }
}

// ---- exclusive scan of a[0 .. min(len, *m_p)) in place (m_p null: len) -------

__global__ void __launch_bounds__(kDsTB) k_ds_scan_reduce(const uint32_t* __restrict__ a, uint32_t len,
                                                          const uint32_t* __restrict__ m_p,
                                                          uint32_t* __restrict__ bsum) {
  const uint32_t m = m_p ? (*m_p < len ? *m_p : len) : len;
  const uint32_t lo = blockIdx.x * kDupsetsTile;
  uint32_t c = 0;
#pragma unroll 4
  for (uint32_t r = 0; r < kDsR; ++r) {
    const uint32_t i = lo + r * kDsTB + threadIdx.x;
    c += i < m ? a[i] : 0u;
  }
  ds_tile_total(c, bsum);
}

// bsum scanned; thread t of a tile scans its 16 consecutive words
__global__ void __launch_bounds__(kDsTB) k_ds_scan_apply(uint32_t* __restrict__ a, uint32_t len,
                                                         const uint32_t* __restrict__ m_p,
                                                         const uint32_t* __restrict__ bsum) {
  __shared__ uint32_t ws[kDsWaves];
  const uint32_t m = m_p ? (*m_p < len ? *m_p : len) : len;
  const uint32_t lo = blockIdx.x * kDupsetsTile + threadIdx.x * kDsR;
  if (blockIdx.x * kDupsetsTile >= m) return;  // uniform
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t v[kDsR];
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDsR; ++k) {
    v[k] = lo + k < m ? a[lo + k] : 0u;
    sum += v[k];
  }
  uint32_t inc = sum;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  uint32_t run = bsum[blockIdx.x] + inc - sum;
#pragma unroll
  for (uint32_t w = 0; w < kDsWaves; ++w)
    if (w < wave) run += ws[w];
#pragma unroll
  for (uint32_t k = 0; k < kDsR; ++k) {
    if (lo + k < m) a[lo + k] = run;
    run += v[k];
  }
}

// ---- the sets in final order, their offsets, the members ---------------------

// Final rank r holds set perm[r] of the set_rep order (perm null: r itself)
__global__ void __launch_bounds__(kDsTB) k_ds_final(const uint32_t* __restrict__ total,
                                                    const uint32_t* __restrict__ perm,
                                                    const uint32_t* __restrict__ hd_file,
                                                    const uint32_t* __restrict__ hd_cnt,
                                                    const uint32_t* __restrict__ hd_label,
                                                    const uint64_t* __restrict__ sizes, uint32_t n,
                                                    int64_t* __restrict__ set_rep, uint64_t* __restrict__ set_bytes,
                                                    uint32_t* __restrict__ fcnt, uint32_t* __restrict__ rank) {
  const uint32_t r = blockIdx.x * kDsTB + threadIdx.x;
  const uint32_t sets = *total;
  if (r >= sets) return;
  const uint32_t s = perm ? perm[r] : r;
  if (s >= sets) return;  // never, perm is a permutation of [0, sets)
  const uint32_t file = hd_file[s], label = hd_label[s];
  if (file >= n || label >= n) return;  // never, both were checked when written
  if (set_rep) set_rep[r] = (int64_t)file;
  if (set_bytes) set_bytes[r] = sizes ? sizes[file] : 0ull;
  fcnt[r] = hd_cnt[s];
  rank[label] = r;
}

__global__ void __launch_bounds__(kDsTB) k_ds_offsets(const uint32_t* __restrict__ total,
                                                      const uint32_t* __restrict__ foff,
                                                      const unsigned long long* __restrict__ counts,
                                                      uint64_t* __restrict__ set_offsets) {
  const uint32_t r = blockIdx.x * kDsTB + threadIdx.x;
  const uint32_t sets = *total;
  if (r < sets) set_offsets[r] = foff[r];
  else if (r == sets) set_offsets[r] = counts[2];
}

__global__ void __launch_bounds__(kDsTB) k_ds_mem_count(const int64_t* __restrict__ rep, uint32_t n,
                                                        const uint32_t* __restrict__ cnt,
                                                        uint32_t* __restrict__ tcnt) {
  const uint32_t lo = blockIdx.x * kDupsetsTile;
  uint32_t c = 0;
#pragma unroll 4
  for (uint32_t r = 0; r < kDsR; ++r) {
    uint32_t label;
    c += ds_is_member(rep, n, lo + r * kDsTB + threadIdx.x, cnt, label);
  }
  ds_tile_total(c, tcnt);
}

__global__ void __launch_bounds__(kDsTB) k_ds_mem_write(const int64_t* __restrict__ rep, uint32_t n,
                                                        const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ rank,
                                                        const uint32_t* __restrict__ toff,
                                                        const uint32_t* __restrict__ total,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ uint32_t ws[kDsWaves];
  const uint32_t b = blockIdx.x;
  const uint32_t mine = (b + 1 < gridDim.x ? toff[b + 1] : *total) - toff[b];
  if (mine == 0) return;  // uniform over the workgroup
  const uint32_t lo = b * kDupsetsTile;
  uint32_t run = toff[b];
#pragma unroll 1
  for (uint32_t r = 0; r < kDsR; ++r) {
    const uint32_t i = lo + r * kDsTB + threadIdx.x;
    uint32_t label = 0, all;
    const bool f = ds_is_member(rep, n, i, cnt, label);
    const uint32_t at = run + ds_round_rank(f, ws, all);
    if (f && at < n) {  // at < n always: at most n files are members
      keys[at] = rank[label];
      vals[at] = i;
    }
    run += all;
  }
}

__global__ void __launch_bounds__(kDsTB) k_ds_members_out(const uint32_t* __restrict__ vals,
                                                          const uint32_t* __restrict__ total,
                                                          int64_t* __restrict__ members) {
  const uint32_t j = blockIdx.x * kDsTB + threadIdx.x;
  if (j < *total) members[j] = (int64_t)vals[j];
}

inline uint32_t ds_blocks(uint32_t m) { return m ? (m + kDsTB - 1) / kDsTB : 1u; }

// a[0 .. min(len, *m_p)) <- its exclusive prefix sums; bsum: a tile sum per 4096
hipError_t ds_scan(uint32_t* a, uint32_t len, const uint32_t* m_p, uint32_t* bsum, uint32_t* unused_total,
                   hipStream_t st) {
  const uint32_t nb = dupsets_tiles(len);
  hipLaunchKernelGGL(k_ds_scan_reduce, dim3(nb), dim3(kDsTB), 0, st, a, len, m_p, bsum);
  hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(1024), 0, st, bsum, nb, unused_total);
  hipLaunchKernelGGL(k_ds_scan_apply, dim3(nb), dim3(kDsTB), 0, st, a, len, m_p, bsum);
  return hipGetLastError();
}

// The first *m_p of at most `bound` (key, value) pairs sorted by the keys' low
// 8 * passes bits, stable; the result is in (ka, va) after an even number of
// passes, else in (kb, vb).
template <typename K>
hipError_t ds_sort(K* ka, K* kb, uint32_t* va, uint32_t* vb, uint32_t bound, const uint32_t* m_p, uint32_t passes,
                   uint32_t* hist, uint32_t* bsum, uint32_t* unused_total, hipStream_t st) {
  const uint32_t nt = dupsets_tiles(bound);
  for (uint32_t p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(k_ds_hist<K>, dim3(nt), dim3(kDsTB), 0, st, (const K*)ka, m_p, 8 * p, hist);
    if (hipError_t e = ds_scan(hist, 256 * nt, nullptr, bsum, unused_total, st)) return e;
    hipLaunchKernelGGL(k_ds_scatter<K>, dim3(nt), dim3(kDsTB), 0, st, (const K*)ka, (const uint32_t*)va, m_p, 8 * p,
                       (const uint32_t*)hist, kb, vb);
    K* tk = ka;
    ka = kb, kb = tk;
    uint32_t* tv = va;
    va = vb, vb = tv;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t duplicate_sets(uint32_t* ws, const int64_t* rep, const uint64_t* sizes, uint32_t n, uint32_t order,
                          int64_t* set_rep, uint64_t* set_offsets, uint64_t* set_bytes, int64_t* members,
                          unsigned long long* counts, hipStream_t st) {
  const DupsetsLayout l = dupsets_layout(n);
  uint32_t* cnt = ws + l.cnt;
  uint32_t* low = ws + l.low;
  uint32_t* rank = ws + l.rank;
  uint32_t* hd_file = ws + l.hd_file;
  uint32_t* hd_cnt = ws + l.hd_cnt;
  uint32_t* hd_label = ws + l.hd_label;
  uint32_t* fcnt = ws + l.fcnt;
  uint32_t* key_a = ws + l.key_a;
  uint32_t* key_b = ws + l.key_b;
  uint32_t* val_a = ws + l.val_a;
  uint32_t* val_b = ws + l.val_b;
  uint32_t* hist = ws + l.hist;
  uint32_t* bsum = ws + l.bsum;
  uint32_t* tcnt = ws + l.tcnt;
  uint32_t* tot = ws + l.tot;  // [0] sets, [1] members, [2] the long scans' total (unused)
  unsigned long long* cts = reinterpret_cast<unsigned long long*>(ws + l.counts);
  const bool by_reclaimable = order == kDupsetsByReclaimable;
  const uint32_t nt = l.tiles, h = l.h;
  const dim3 block(kDsTB);
  hipError_t e;
  if ((e = hipMemsetAsync(cnt, 0, (size_t)n * sizeof(uint32_t), st))) return e;
  if ((e = hipMemsetAsync(low, 0xFF, (size_t)n * sizeof(uint32_t), st))) return e;
  if ((e = hipMemsetAsync(tot, 0, (l.words - l.tot) * sizeof(uint32_t), st))) return e;  // tot and counts

  // the labels' files and lowest file; the sets in set_rep order
  hipLaunchKernelGGL(k_ds_count, dim3(nt), block, 0, st, rep, n, cnt, low, cts);
  hipLaunchKernelGGL(k_ds_head_count, dim3(nt), block, 0, st, rep, n, (const uint32_t*)cnt, (const uint32_t*)low,
                     tcnt);
  hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(1024), 0, st, tcnt, nt, tot + 0);
  hipLaunchKernelGGL(k_ds_head_write, dim3(nt), block, 0, st, rep, sizes, n, (const uint32_t*)cnt,
                     (const uint32_t*)low, (const uint32_t*)tcnt, (const uint32_t*)(tot + 0), hd_file, hd_cnt,
                     hd_label, by_reclaimable ? reinterpret_cast<uint64_t*>(key_a) : nullptr, val_a, cts);
  if ((e = hipGetLastError())) return e;

  // by reclaimable bytes: the sets sorted by the complement, ties keep the set_rep order
  const uint32_t* perm = nullptr;
  if (by_reclaimable) {
    if ((e = ds_sort<uint64_t>(reinterpret_cast<uint64_t*>(key_a), reinterpret_cast<uint64_t*>(key_b), val_a, val_b,
                               h, tot + 0, 8, hist, bsum, tot + 2, st)))
      return e;
    perm = val_a;
  }
  hipLaunchKernelGGL(k_ds_final, dim3(ds_blocks(h)), block, 0, st, (const uint32_t*)(tot + 0), perm,
                     (const uint32_t*)hd_file, (const uint32_t*)hd_cnt, (const uint32_t*)hd_label, sizes, n, set_rep,
                     set_bytes, fcnt, rank);
  if ((e = hipGetLastError())) return e;

  if (set_offsets) {
    if ((e = ds_scan(fcnt, h, tot + 0, bsum, tot + 2, st))) return e;
    hipLaunchKernelGGL(k_ds_offsets, dim3(ds_blocks(h)), block, 0, st, (const uint32_t*)(tot + 0),
                       (const uint32_t*)fcnt, (const unsigned long long*)cts, set_offsets);
    if ((e = hipGetLastError())) return e;
  }

  if (members) {
    // (final rank, file) of every member in file order, sorted by the rank's bits
    hipLaunchKernelGGL(k_ds_mem_count, dim3(nt), block, 0, st, rep, n, (const uint32_t*)cnt, tcnt);
    hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(1024), 0, st, tcnt, nt, tot + 1);
    hipLaunchKernelGGL(k_ds_mem_write, dim3(nt), block, 0, st, rep, n, (const uint32_t*)cnt, (const uint32_t*)rank,
                       (const uint32_t*)tcnt, (const uint32_t*)(tot + 1), key_a, val_a);
    if ((e = hipGetLastError())) return e;
    uint32_t bits = 1;
    while (bits < 32 && (1ull << bits) < (uint64_t)n / 2) ++bits;  // ranks are below n / 2
    const uint32_t passes = (bits + 7) / 8;
    if ((e = ds_sort<uint32_t>(key_a, key_b, val_a, val_b, n, tot + 1, passes, hist, bsum, tot + 2, st))) return e;
    hipLaunchKernelGGL(k_ds_members_out, dim3(ds_blocks(n)), block, 0, st,
                       (const uint32_t*)((passes & 1) ? val_b : val_a), (const uint32_t*)(tot + 1), members);
    if ((e = hipGetLastError())) return e;
  }
  if (counts)
    return hipMemcpyAsync(counts, cts, kDupsetsCounts * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  return hipSuccess;
}

// what dirtree.hip shares (dupsets.h)
hipError_t dupsets_sort_u64(uint64_t* ka, uint64_t* kb, uint32_t* va, uint32_t* vb, uint32_t bound,
                            const uint32_t* m_p, uint32_t passes, uint32_t* hist, uint32_t* bsum,
                            uint32_t* scan_total, hipStream_t st) {
  return ds_sort<uint64_t>(ka, kb, va, vb, bound, m_p, passes, hist, bsum, scan_total, st);
}
hipError_t dupsets_sort_u32(uint32_t* ka, uint32_t* kb, uint32_t* va, uint32_t* vb, uint32_t bound,
                            const uint32_t* m_p, uint32_t passes, uint32_t* hist, uint32_t* bsum,
                            uint32_t* scan_total, hipStream_t st) {
  return ds_sort<uint32_t>(ka, kb, va, vb, bound, m_p, passes, hist, bsum, scan_total, st);
}
hipError_t dupsets_label_counts(const int64_t* rep, uint32_t n, uint32_t* cnt, uint32_t* low,
                                unsigned long long* counts, hipStream_t st) {
  hipLaunchKernelGGL(k_ds_count, dim3(dupsets_tiles(n)), dim3(kDsTB), 0, st, rep, n, cnt, low, counts);
  return hipGetLastError();
}

}  // namespace sdcas
