// family_bytes_device.h — the class table's device side, shared by
// family_bytes.hip and family_recipes.hip: who takes part, the class (label of
// the chunk's row, chunk class number) as one u64, and the insert that leaves
// in every slot its class's first occurrence. family_bytes.hip's head comment
// has the scheme and its visibility rules.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "family_bytes.h"

namespace sdcas {

constexpr uint32_t kFbNone = 0xFFFFFFFFu;

typedef unsigned long long u64a;  // what the 64-bit atomics take

__device__ __forceinline__ uint32_t fb_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t fb_load(const u64a* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t fb_mix(uint64_t x) {
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  return x;
}

__device__ __forceinline__ uint64_t fb_wave_sum(uint64_t v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor((u64a)v, d);
  return v;
}
__device__ __forceinline__ uint64_t fb_wave_max(uint64_t v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    const uint64_t t = __shfl_xor((u64a)v, d);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t fb_first(unsigned long long lanes) { return (uint32_t)__ffsll((long long)lanes) - 1; }

// the label of row i when it takes part (in [0, n)), else false
__device__ __forceinline__ bool fb_label(const int64_t* __restrict__ family, uint32_t n, uint32_t i, uint32_t& label) {
  if (i >= n) return false;
  const int64_t v = family[i];
  if (v < 0 || (uint64_t)v >= (uint64_t)n) return false;
  label = (uint32_t)v;
  return true;
}

// the row and the class of chunk c when it takes part, else false. The class
// number is a number only: rep[c] inside [0, c], else c.
__device__ __forceinline__ bool fb_class(const FamilyBytesIn& in, uint32_t c, uint32_t& row, uint64_t& cls) {
  if (c >= in.m) return false;
  row = in.chunk_file[c];
  uint32_t label;
  if (!fb_label(in.family, in.n, row, label)) return false;
  const int64_t r = in.rep[c];
  cls = (uint64_t)label << 32 | (r >= 0 && r <= (int64_t)c ? (uint32_t)r : c);
  return true;
}

// One chunk per thread of a workgroup of kFamilyBytesTB into the table
// (filled with kFbNone, mask + 1 slots, at least 2 m); slot[c] <- the slot of
// the chunk's class, kFbNone for a chunk that takes no part. Called by every
// thread of the grid.
__device__ __forceinline__ void fb_insert(const FamilyBytesIn& in, uint32_t* table, uint32_t mask,
                                          uint32_t* __restrict__ slot) {
  const uint32_t c = blockIdx.x * kFamilyBytesTB + threadIdx.x, lane = threadIdx.x & 63;
  uint32_t row = 0;
  uint64_t cls = 0;
  const bool on = fb_class(in, c, row, cls);
  const unsigned long long live = __ballot(on);
  const uint32_t lead = live ? fb_first(live) : 0u;
  // the lanes that carry the first active lane's class follow it: that lane's
  // position is their lowest, so it alone is sent
  const uint64_t lcls = __shfl((u64a)cls, lead);
  const bool follow = on && lane != lead && cls == lcls;
  uint32_t at = kFbNone;
  if (on && !follow) {
    uint32_t h = (uint32_t)fb_mix(cls) & mask;
    for (uint32_t step = 0; step <= mask; ++step) {  // ends at an empty slot: the table is never more than half full
      uint32_t cur = fb_load(&table[h]);
      if (cur == kFbNone) {
        const uint32_t prev = atomicCAS(&table[h], kFbNone, c);
        if (prev == kFbNone) {
          at = h;
          break;
        }
        cur = prev;
      }
      uint32_t orow;
      uint64_t ocls;
      if (fb_class(in, cur, orow, ocls) && ocls == cls) {
        if (cur > c) atomicMin(&table[h], c);
        at = h;
        break;
      }
      h = (h + 1) & mask;
    }
  }
  const uint32_t lat = __shfl(at, lead);
  if (follow) at = lat;
  if (c < in.m) slot[c] = at;
}

}  // namespace sdcas
