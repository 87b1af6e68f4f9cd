// index_device.h — the device primitives the chunk index (chunk_index.hip),
// the holders index (chunk_holders.hip) and the confirm group-by (confirm.hip)
// share: the 32-byte digest as two 16-byte loads, its memcmp order, the
// searches in ascending u32 arrays and a key's directory bucket. Everything
// here is inlined into the kernel that uses it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk_index.h"

namespace sdcas {

struct IxDigest {
  uint4 a, b;
};
__device__ __forceinline__ IxDigest ix_digest(const uint8_t* __restrict__ digests, uint32_t i) {
  const uint4* p = reinterpret_cast<const uint4*>(digests) + 2 * (size_t)i;
  return IxDigest{p[0], p[1]};
}
__device__ __forceinline__ void ix_store(uint8_t* __restrict__ digests, uint32_t i, const IxDigest& d) {
  uint4* p = reinterpret_cast<uint4*>(digests) + 2 * (size_t)i;
  p[0] = d.a;
  p[1] = d.b;
}
// memcmp of the 32 bytes: < 0, 0, > 0. The words are little-endian loads, so
// each is byte-swapped before it is compared.
__device__ __forceinline__ int ix_cmp(const IxDigest& x, const IxDigest& y) {
  const uint32_t xs[8] = {x.a.x, x.a.y, x.a.z, x.a.w, x.b.x, x.b.y, x.b.z, x.b.w};
  const uint32_t ys[8] = {y.a.x, y.a.y, y.a.z, y.a.w, y.b.x, y.b.y, y.b.z, y.b.w};
#pragma unroll
  for (uint32_t w = 0; w < 8; ++w) {
    if (xs[w] != ys[w]) return __builtin_bswap32(xs[w]) < __builtin_bswap32(ys[w]) ? -1 : 1;
  }
  return 0;
}

__device__ __forceinline__ uint32_t ix_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the number of a[0 .. len) that are <= v, looked for in [lo, hi] (a ascending)
__device__ __forceinline__ uint32_t ix_upper(const uint32_t* __restrict__ a, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the bucket of `key`: [lo, hi), both clamped to n
__device__ __forceinline__ void ix_bucket(const IndexView& ix, uint64_t key, uint32_t& lo, uint32_t& hi) {
  const uint32_t b = ix.bits ? (uint32_t)(key >> (64 - ix.bits)) : 0u;
  lo = ix_min(ix.dir[b], ix.n);
  hi = ix_min(ix.dir[b + 1], ix.n);
  if (hi < lo) hi = lo;
}

}  // namespace sdcas
