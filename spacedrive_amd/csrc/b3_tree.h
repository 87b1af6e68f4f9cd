// b3_tree.h — the slot / tree bookkeeping shared by the batch kernels
// (b3_batch.hip) and the dual cas_id + checksum kernels (b3_dual.hip): a
// message's chunk count, the closed forms of its in-tile tree nodes, the tile
// tree's task encoding, the tail-mask table and the digest store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b3_batch.h"
#include "b3_device.h"

namespace sdcas {

using namespace b3d;

__host__ __device__ inline uint64_t chunk_count(uint64_t len) { return len == 0 ? 1 : (len + CHUNK_LEN - 1) / CHUNK_LEN; }

// Highest level k such that the node of 2^k chunks starting at chunk j is
// (a) an aligned complete block of the message, (b) not the whole message and
// (c) inside the tile that holds chunk j at slot `s`.
// Closed form (checked against the defining loop — grow k while the node of
// 2^(k+1) chunks at j is aligned, fits the message, is not the whole message
// and fits the tile — on 2 M random cases): the largest k with 2^k dividing j,
// 2^k <= C - j, 2^k < C and 2^k <= TILE - s.
__host__ __device__ inline uint32_t floor_log2(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }  // x > 0

template <uint32_t TILE>
__host__ __device__ inline uint32_t node_level_t(uint64_t j, uint64_t C, uint32_t s) {
  if (C <= 1) return 0;
  const uint32_t a = j ? (uint32_t)__builtin_ctzll(j) : 63u;
  const uint32_t b = min(floor_log2(C - j), floor_log2(C - 1));
  return min(min(a, b), floor_log2((uint64_t)TILE - s));
}

__host__ __device__ inline uint32_t node_level(uint64_t j, uint64_t C, uint32_t s) { return node_level_t<kTile>(j, C, s); }

// Is the level-k node at (j, s) consumed by a parent computed in the same tile?
template <uint32_t TILE>
__host__ __device__ inline bool parent_in_tile_t(uint64_t j, uint64_t C, uint32_t s, uint32_t k) {
  uint64_t w = 1ull << k;
  if (!((j >> k) & 1)) return false;
  return j + w <= C && 2 * w < C && s >= w && (uint64_t)s + w <= TILE;
}

__host__ __device__ inline bool parent_in_tile(uint64_t j, uint64_t C, uint32_t s, uint32_t k) {
  uint64_t w = 1ull << k;
  if (!((j >> k) & 1)) return false;  // left children's parents start at s: not computed
  return j + w <= C && 2 * w < C && s >= w && (uint64_t)s + w <= kTile;
}

// Tail masks by the length of a message's last block: row b keeps bytes
// [0, b) of a 64-byte block (word w: all ones, none, or its low 8 * (b - 4w)
// bits). Four 16-byte loads of an L1-resident 4 KiB table replace the ~100
// VALU instructions of computing the sixteen masks.
struct alignas(16) TailMasks {
  uint32_t w[BLOCK_LEN + 1][16];
};
constexpr TailMasks make_tail_masks() {
  TailMasks t{};
  for (int b = 0; b <= (int)BLOCK_LEN; ++b)
    for (int w = 0; w < 16; ++w) {
      const int r = b - 4 * w;
      t.w[b][w] = r >= 4 ? 0xFFFFFFFFu : (r <= 0 ? 0u : ((1u << (8 * r)) - 1u));
    }
  return t;
}
__device__ const TailMasks kTailMasks = make_tail_masks();

__device__ __forceinline__ void mask_tail_table(uint32_t (&m)[16], uint32_t blen) {
  const uint4* q = reinterpret_cast<const uint4*>(kTailMasks.w[blen]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 v = q[k];
    m[4 * k] &= v.x;
    m[4 * k + 1] &= v.y;
    m[4 * k + 2] &= v.z;
    m[4 * k + 3] &= v.w;
  }
}

__device__ __forceinline__ void store_digest(uint32_t m, const uint32_t (&d)[8], uint8_t* out32, uint64_t* out_keys) {
  if (out32) {
    uint4* o = reinterpret_cast<uint4*>(out32 + 32ull * m);
    o[0] = make_uint4(d[0], d[1], d[2], d[3]);
    o[1] = make_uint4(d[4], d[5], d[6], d[7]);
  }
  if (out_keys) out_keys[m] = cas_key(d);
}

// per-level task regions of the in-tile tree: level k (1..10) holds at most
// 2 * (kTile >> k) tasks (regular level-k nodes are disjoint 2^k blocks, spine
// steps consume disjoint maximal 2^(k-1) blocks), 2046 entries in all
template <uint32_t TL = kTile>
__host__ __device__ constexpr uint32_t task_base(uint32_t k) { return 2 * (TL - (TL >> (k - 1))); }
template <uint32_t TL = kTile>
constexpr uint32_t kTaskCap = 2 * (TL - 1);
constexpr uint16_t kNoMsg = 0xFFFF;

__device__ __forceinline__ uint32_t enc_task(uint32_t l, uint32_t r, uint32_t msg, bool root) {
  return l | (r << 10) | (msg << 20) | (root ? 0x80000000u : 0u);
}

}  // namespace sdcas
