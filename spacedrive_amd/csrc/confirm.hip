// confirm.hip — duplicates confirmed by checksum: a group-by over the pair
// (cas key, 32-byte BLAKE3 digest of the whole content).
//
// A cas_id above 100 KiB hashes 57 352 bytes of the file (cas.rs:23-62), so
// two files of one length that agree in those windows share it whatever the
// rest holds. The identifier links by cas_id alone (dist_dedup.hip); this
// group-by says which of its groups are equal files (one CLASS: same key, same
// digest) and which cas keys carry more than one class (a COLLISION).
//
// The index-table scheme of k_solo_insert_idx with 40-byte keys: two
// open-addressed tables of u32 file indices, the class table hashed by key and
// digest, the key table by the key alone. A slot goes from empty to an index
// of ONE class (key) by CAS and from then on only to lower indices of that
// class (key) by atomicMin; a prober meeting an occupied slot gathers the
// occupant's key and digest from the read-only inputs, compares all 40 bytes
// (8 for the key table) and moves on when they differ. After the insert each
// slot holds its class's (key's) lowest valid file, whatever the order the
// files arrived in: the results do not depend on scheduling.
//   k_cf_insert   every valid file into both tables; remembers its two slots
//   k_cf_classes  each class's lowest file adds 1 to its key's class counter,
//                 indexed by the key's lowest file
//   k_cf_write    rep, key_rep, flags; the six counts reduced per workgroup,
//                 one atomic per counter per workgroup
// Table and counter words are touched only by device-scope atomics and atomic
// loads; keys and digests are kernel inputs (plain loads); the passes are
// separate launches.
#include <hip/hip_runtime.h>

#include "confirm.h"
#include "index_device.h"

namespace sdcas {

namespace {

constexpr uint32_t kCfTB = 256;
constexpr uint32_t kCfEmpty = 0xFFFFFFFFu;
constexpr uint8_t kCfDuplicate = 1, kCfCollision = 2, kCfSkipped = 4;  // SDCAS_CONFIRM_*

__device__ __forceinline__ uint64_t cf_mix(uint64_t x) {
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  return x;
}

// (the digest of file i as two 16-byte loads: IxDigest / ix_digest, index_device.h)
__device__ __forceinline__ bool cf_same(const IxDigest& x, const IxDigest& y) {
  return x.a.x == y.a.x && x.a.y == y.a.y && x.a.z == y.a.z && x.a.w == y.a.w && x.b.x == y.b.x && x.b.y == y.b.y &&
         x.b.z == y.b.z && x.b.w == y.b.w;
}
// every digest byte enters the class hash (digests that differ in one byte
// land in different places, not at the end of one probe chain)
__device__ __forceinline__ uint32_t cf_class_hash(uint64_t key, const IxDigest& d) {
  constexpr uint64_t P = 0x9E3779B97F4A7C15ull;
  uint64_t h = cf_mix(key);
  h = (h ^ ((uint64_t)d.a.y << 32 | d.a.x)) * P;
  h = (h ^ ((uint64_t)d.a.w << 32 | d.a.z)) * P;
  h = (h ^ ((uint64_t)d.b.y << 32 | d.b.x)) * P;
  h = (h ^ ((uint64_t)d.b.w << 32 | d.b.z)) * P;
  return (uint32_t)cf_mix(h);
}

__device__ __forceinline__ uint32_t cf_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_cf_insert(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ digests,
                            const uint8_t* __restrict__ valid, uint32_t n, uint32_t* __restrict__ tab_c,
                            uint32_t* __restrict__ tab_k, uint32_t mask, uint32_t* __restrict__ slot_c,
                            uint32_t* __restrict__ slot_k) {
  const uint32_t i = blockIdx.x * kCfTB + threadIdx.x;
  if (i >= n) return;
  if (valid && !valid[i]) {
    slot_c[i] = slot_k[i] = kCfEmpty;
    return;
  }
  const uint64_t key = keys[i];
  const IxDigest dig = ix_digest(digests, i);
  // the class table: key and digest
  uint32_t h = cf_class_hash(key, dig) & mask;
  for (;;) {
    uint32_t cur = cf_load(&tab_c[h]);
    if (cur == kCfEmpty) {
      const uint32_t prev = atomicCAS(&tab_c[h], kCfEmpty, i);
      if (prev == kCfEmpty) break;
      cur = prev;
    }
    if (keys[cur] == key && cf_same(ix_digest(digests, cur), dig)) {
      if (cur > i) atomicMin(&tab_c[h], i);
      break;
    }
    h = (h + 1) & mask;
  }
  slot_c[i] = h;
  // the key table: the key alone
  h = (uint32_t)cf_mix(key) & mask;
  for (;;) {
    uint32_t cur = cf_load(&tab_k[h]);
    if (cur == kCfEmpty) {
      const uint32_t prev = atomicCAS(&tab_k[h], kCfEmpty, i);
      if (prev == kCfEmpty) break;
      cur = prev;
    }
    if (keys[cur] == key) {
      if (cur > i) atomicMin(&tab_k[h], i);
      break;
    }
    h = (h + 1) & mask;
  }
  slot_k[i] = h;
}

__global__ void k_cf_classes(uint32_t n, const uint32_t* __restrict__ tab_c, const uint32_t* __restrict__ tab_k,
                             const uint32_t* __restrict__ slot_c, const uint32_t* __restrict__ slot_k,
                             uint32_t* __restrict__ kcnt) {
  const uint32_t i = blockIdx.x * kCfTB + threadIdx.x;
  if (i >= n) return;
  const uint32_t sc = slot_c[i];
  if (sc == kCfEmpty) return;           // skipped
  if (cf_load(&tab_c[sc]) != i) return;  // not its class's lowest file
  atomicAdd(&kcnt[cf_load(&tab_k[slot_k[i]])], 1u);
}

__global__ void k_cf_write(uint32_t n, const uint32_t* __restrict__ tab_c, const uint32_t* __restrict__ tab_k,
                           const uint32_t* __restrict__ slot_c, const uint32_t* __restrict__ slot_k,
                           const uint32_t* __restrict__ kcnt, int64_t* __restrict__ rep,
                           int64_t* __restrict__ key_rep, uint8_t* __restrict__ flags,
                           unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_cnt[kConfirmCounts];
  if (threadIdx.x < kConfirmCounts) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kCfTB + threadIdx.x;
  // files, classes, keys, collided_keys, collided_files, duplicate_files
  bool add[kConfirmCounts] = {false, false, false, false, false, false};
  if (i < n) {
    const uint32_t sc = slot_c[i];
    if (sc == kCfEmpty) {
      if (rep) rep[i] = -1;
      if (key_rep) key_rep[i] = -1;
      if (flags) flags[i] = kCfSkipped;
    } else {
      const uint32_t c = cf_load(&tab_c[sc]);
      const uint32_t k = cf_load(&tab_k[slot_k[i]]);
      const bool collided = cf_load(&kcnt[k]) >= 2;
      if (rep) rep[i] = (int64_t)c;
      if (key_rep) key_rep[i] = (int64_t)k;
      if (flags) flags[i] = (uint8_t)((c != i ? kCfDuplicate : 0) | (collided ? kCfCollision : 0));
      add[0] = true;
      add[1] = c == i;
      add[2] = k == i;
      add[3] = k == i && collided;
      add[4] = collided;
      add[5] = c != i;
    }
  }
  if (!counts) return;  // the same for every thread of the grid
#pragma unroll
  for (uint32_t w = 0; w < kConfirmCounts; ++w) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(add[w]));
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(&s_cnt[w], cnt);
  }
  __syncthreads();
  if (threadIdx.x < kConfirmCounts && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

}  // namespace

hipError_t confirm_duplicates(uint32_t* ws, const uint64_t* keys, const uint8_t* digests, const uint8_t* valid,
                              uint32_t n, int64_t* rep, int64_t* key_rep, uint8_t* flags,
                              unsigned long long* counts, hipStream_t st) {
  const uint64_t cap = confirm_table_cap(n);
  uint32_t* tab_c = ws;
  uint32_t* tab_k = tab_c + cap;
  uint32_t* kcnt = tab_k + cap;
  uint32_t* slot_c = kcnt + n;
  uint32_t* slot_k = slot_c + n;
  hipError_t e;
  if ((e = hipMemsetAsync(tab_c, 0xFF, 2 * cap * sizeof(uint32_t), st))) return e;
  if ((e = hipMemsetAsync(kcnt, 0, (size_t)n * sizeof(uint32_t), st))) return e;
  if (counts && (e = hipMemsetAsync(counts, 0, kConfirmCounts * sizeof(unsigned long long), st))) return e;
  const dim3 grid((n + kCfTB - 1) / kCfTB), block(kCfTB);
  const uint32_t mask = (uint32_t)(cap - 1);
  hipLaunchKernelGGL(k_cf_insert, grid, block, 0, st, keys, digests, valid, n, tab_c, tab_k, mask, slot_c, slot_k);
  if ((e = hipGetLastError())) return e;
  hipLaunchKernelGGL(k_cf_classes, grid, block, 0, st, n, tab_c, tab_k, slot_c, slot_k, kcnt);
  if ((e = hipGetLastError())) return e;
  if (!rep && !key_rep && !flags && !counts) return hipSuccess;
  hipLaunchKernelGGL(k_cf_write, grid, block, 0, st, n, tab_c, tab_k, slot_c, slot_k, kcnt, rep, key_rep, flags,
                     counts);
  return hipGetLastError();
}

}  // namespace sdcas
