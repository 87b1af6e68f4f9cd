// wg_scan.h — the one-workgroup exclusive scan the library's ordered
// compactions and sorts share (dist_dedup.hip's k_stays_scan, dupsets.hip's
// k_ds_scan): per-workgroup counts become offsets between two launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdcas {

// Called by every thread of ONE workgroup of 1024: cnt[b] <- the sum of
// cnt[0 .. b) for b in [0, nb); *total <- the sum of all.
__device__ __forceinline__ void wg_scan_exclusive_1024(uint32_t* __restrict__ cnt, uint32_t nb,
                                                       uint32_t* __restrict__ total) {
  __shared__ uint32_t ws[16];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += 1024) {
    const uint32_t i = base + tid;
    const uint32_t v = i < nb ? cnt[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wave; ++w) before += ws[w];
    if (i < nb) cnt[i] = before + inc - v;
    __syncthreads();
    if (tid == 1023) carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// Called by every thread of ONE workgroup of at most 1024: the sums of a and b
// and the maximum of c over the workgroup, valid in thread 0 alone (families.hip's
// k_ff_write: one atomic per workgroup and count behind it).
__device__ __forceinline__ void wg_reduce_sum2_max(unsigned long long& a, unsigned long long& b,
                                                   unsigned long long& c) {
  __shared__ unsigned long long rs[3][16];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    a += __shfl_down(a, d);
    b += __shfl_down(b, d);
    const unsigned long long t = __shfl_down(c, d);
    c = t > c ? t : c;
  }
  if (lane == 0) rs[0][wave] = a, rs[1][wave] = b, rs[2][wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t waves = (blockDim.x + 63) >> 6;
    for (uint32_t w = 1; w < waves; ++w) {
      a += rs[0][w], b += rs[1][w];
      c = rs[2][w] > c ? rs[2][w] : c;
    }
  }
}

}  // namespace sdcas
