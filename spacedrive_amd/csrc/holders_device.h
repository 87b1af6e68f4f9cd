// holders_device.h — the device primitives the holders index
// (chunk_holders.hip) and the chunk peers (chunk_peers.hip) share: the triple
// (key, digest, value) and its order, the two searches that find a pair's run
// and a triple's place in it, the rank of a flag in its workgroup, and the
// three-level scan of per-workgroup counts (chunk_holders.h has its layout).
// The library has no relocatable device code, so the one scan kernel is
// `static`: each of the two files that include this launches its own copy of
// the one definition. Everything else is inlined into the kernel that uses it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk_holders.h"
#include "index_device.h"

namespace sdcas {

constexpr uint32_t kChTB = kHoldersTB;
static_assert(kHoldersTB == kIndexTB, "a scan tile is one workgroup's items");

struct ChTriple {
  uint64_t key;
  IxDigest dig;
  uint64_t val;
};
__device__ __forceinline__ ChTriple ch_triple(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ digests,
                                              const uint64_t* __restrict__ values, uint32_t i) {
  return ChTriple{keys[i], ix_digest(digests, i), values ? values[i] : 0ull};
}
// entry i of (keys, digests, values) against t: < 0, 0, > 0. The digest is read
// only where the keys are equal, the value only where the digests are.
__device__ __forceinline__ int ch_cmp3(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ digests,
                                       const uint64_t* __restrict__ values, uint32_t i, const ChTriple& t) {
  const uint64_t k = keys[i];
  if (k != t.key) return k < t.key ? -1 : 1;
  const int c = ix_cmp(ix_digest(digests, i), t.dig);
  if (c) return c;
  const uint64_t v = values ? values[i] : 0ull;
  return v == t.val ? 0 : (v < t.val ? -1 : 1);
}

// the first entry of [lo, hi) whose pair is not below (key, dig) — or, with
// `after`, the first whose pair is above it
__device__ __forceinline__ uint32_t ch_pair_bound(const IndexView& ix, uint32_t lo, uint32_t hi, uint64_t key,
                                                  const IxDigest& dig, bool after) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t k = ix.keys[mid];
    bool below;
    if (k != key) {
      below = k < key;
    } else {
      const int c = ix_cmp(ix_digest(ix.digests, mid), dig);
      below = after ? c <= 0 : c < 0;
    }
    if (below) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the first entry of t's bucket that is not below t; found: it is equal
__device__ __forceinline__ uint32_t ch_lower_bound3(const IndexView& ix, const ChTriple& t, bool& found) {
  found = false;
  if (!ix.n) return 0;
  uint32_t lo, hi;
  ix_bucket(ix, t.key, lo, hi);
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const int c = ch_cmp3(ix.keys, ix.digests, ix.values, mid, t);
    if (c == 0) {
      found = true;
      return mid;
    }
    if (c < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Called by every thread of a workgroup of 256: the number of lower threads
// whose flag is set; *total <- the workgroup's. s: 4 words of LDS.
__device__ __forceinline__ uint32_t ch_rank(bool flag, uint32_t* s, uint32_t* total) {
  const uint64_t bal = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kChTB / 64; ++w) {
    const uint32_t v = s[w];
    before += w < wave ? v : 0u;
    all += v;
  }
  *total = all;
  return before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}

// the counts of the workgroups before b, from the three scanned levels
__device__ __forceinline__ uint32_t ch_base(const uint32_t* __restrict__ l1, const uint32_t* __restrict__ l2,
                                            const uint32_t* __restrict__ l3, uint32_t b) {
  return l1[b] + l2[b >> 8] + l3[b >> 16];
}

// One level of the scan: every workgroup turns its 256 counts of a[0 .. n) into
// their exclusive scan and leaves their sum in up[blockIdx.x].
static __global__ void __launch_bounds__(kChTB) k_ch_scan(uint32_t* __restrict__ a, uint32_t n,
                                                          uint32_t* __restrict__ up) {
  __shared__ uint32_t s_w[kChTB / 64];
  const uint32_t i = blockIdx.x * kChTB + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t v = i < n ? a[i] : 0u;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kChTB / 64; ++w) {
    const uint32_t t = s_w[w];
    before += w < wave ? t : 0u;
    all += t;
  }
  if (i < n) a[i] = before + inc - v;
  if (threadIdx.x == 0) up[blockIdx.x] = all;
}

// the per-workgroup counts in l1 scanned; the sum of all in tot[0]
static inline void ch_scan(uint8_t* ws, const HoldersScanLayout& s, hipStream_t st) {
  uint32_t* l1 = index_at<uint32_t>(ws, s.l1);
  uint32_t* l2 = index_at<uint32_t>(ws, s.l2);
  uint32_t* l3 = index_at<uint32_t>(ws, s.l3);
  uint32_t* tot = index_at<uint32_t>(ws, s.tot);
  hipLaunchKernelGGL(k_ch_scan, dim3(s.n2), dim3(kChTB), 0, st, l1, s.n1, l2);
  hipLaunchKernelGGL(k_ch_scan, dim3(s.n3), dim3(kChTB), 0, st, l2, s.n2, l3);
  hipLaunchKernelGGL(k_ch_scan, dim3(1), dim3(kChTB), 0, st, l3, s.n3, tot);  // n3 <= 64
}

}  // namespace sdcas
