// b3_dual.hip — cas_id and checksum of content-resident files from ONE pass
// over their bytes.
//
// For a file of 1..102400 bytes sd-core hashes almost the same bytes twice:
// generate_cas_id (core/src/object/cas.rs:23-62) hashes le64(len) || content,
// file_checksum (core/src/object/validation/hash.rs:11-25) hashes content.
// k_dual_leaf loads each 64-byte block of content once and feeds two chains:
//
//   content   |w0 w1 ... w13 w14 w15|w0 w1 ... w13 w14 w15|w0 ...
//   checksum  |<----- block b ----->|<---- block b+1 ---->|
//   cas    |len|<-- block b = carry(2) + w0..w13 -->|w14 w15 + w0..w13|
//
// The cas message is the content shifted by exactly two words, so its block b
// is the last two words of the previous load (the size for block 0 of chunk
// 0; the 8 bytes before the chunk, from the previous 16-byte word, for block
// 0 of a later chunk) followed by the first fourteen of this one: register
// renaming, no byte shifts. One mask — the content bytes at or past `len` —
// serves both chains. The cas message is len + 8 bytes: its last block, its
// block count and its chunk count can each exceed the checksum's by one, so a
// file owns a lane per CAS chunk (the checksum chain of the extra one is
// empty).
//
// Slots and trees are batch_hash's: the two chunk-CV streams are two planned
// batches (lens len + 8 and len; plan_slots), each lane writes its two CVs to
// its slot of each plan in the node workspace, k_dual_tree runs the in-tile
// tree of a plan over them (k_leaf_tree's phases 1, 3 and 4 with the chunk
// CVs read from the workspace instead of hashed), and finish_crossing merges
// the messages that cross a tile. The cas root keeps its key only, the
// checksum root all 32 bytes.
//
// Files above 102400 bytes share only 57,344 bytes between the two hashes and
// are not fused: k_cas_gather copies le64(len), header, four samples and
// footer into a scratch message, and batch_hash hashes that and the content.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "b3_batch.h"
#include "b3_device.h"
#include "b3_tree.h"

namespace sdcas {

constexpr uint32_t kDualWG = 256;   // k_dual_leaf: four slots per lane and tile
constexpr uint32_t kTreeWG = 512;   // k_dual_tree
constexpr uint32_t kSampledLen = 57352;
constexpr uint32_t kHeader = 8192, kSample = 10240;

static inline size_t up16(size_t x) { return (x + 15) & ~size_t(15); }

// the scratch's layout (identify_scratch_bytes)
struct IdLayout {
  uint64_t *dlA, *dlB, *SA, *SB, *totA, *totB, *ctr;
  uint32_t* sidx;
  uint64_t *goffs, *glens, *coffs, *clens, *tmpk;
  uint8_t *tmp32, *gather;
  size_t bytes;
};
static IdLayout id_layout(uint8_t* base, uint32_t n, uint32_t G) {
  IdLayout l{};
  size_t o = 0;
  auto take = [&](size_t b) {
    uint8_t* p = base + o;
    o += up16(b);
    return p;
  };
  l.dlA = (uint64_t*)take(8ull * n);
  l.dlB = (uint64_t*)take(8ull * n);
  l.SA = (uint64_t*)take(8ull * n);
  l.SB = (uint64_t*)take(8ull * n);
  l.totA = (uint64_t*)take(32);
  l.totB = (uint64_t*)take(32);
  l.ctr = (uint64_t*)take(16);
  l.sidx = (uint32_t*)take(4ull * G);
  l.goffs = (uint64_t*)take(8ull * G);
  l.glens = (uint64_t*)take(8ull * G);
  l.coffs = (uint64_t*)take(8ull * G);
  l.clens = (uint64_t*)take(8ull * G);
  l.tmpk = (uint64_t*)take(8ull * G);
  l.tmp32 = take(32ull * G);
  l.gather = take(kGatherStride * (size_t)G + 64);
  l.bytes = o;
  return l;
}

// Per file: the two plans' message lengths (a file outside the fused branch
// is an empty message of both, a slot no lane hashes), has_key, the
// empty-input digest of an empty file, and the list of files above kWholeMax.
__global__ void __launch_bounds__(256) k_dual_prep(const uint64_t* __restrict__ lens, uint32_t n,
                                                   uint64_t* __restrict__ dlA, uint64_t* __restrict__ dlB,
                                                   uint64_t* __restrict__ ctr, uint32_t* __restrict__ sidx, uint32_t G,
                                                   uint8_t* __restrict__ out32, uint8_t* __restrict__ out_has_key) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t len = lens[i];
  const bool whole = len >= 1 && len <= kWholeMax;
  dlA[i] = whole ? len + 8 : 0;
  dlB[i] = whole ? len : 0;
  if (out_has_key) out_has_key[i] = len != 0;
  if (len == 0 && out32) {
    uint32_t cv[8], m[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) m[w] = 0;
    set_iv(cv);
    compress<GSched::kCompiler>(cv, m, 0, 0, CHUNK_START | CHUNK_END | ROOT);
    store_digest(i, cv, out32, nullptr);
  }
  if (len > kWholeMax) {
    const uint32_t r = atomicAdd(reinterpret_cast<unsigned int*>(ctr), 1u);
    if (r < G) sidx[r] = i;
  }
}

__device__ __forceinline__ void store_cv(uint32_t* __restrict__ nodes, uint64_t slot, const uint32_t (&cv)[8]) {
  uint4* o = reinterpret_cast<uint4*>(nodes + 8ull * slot);
  o[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
  o[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
}

// One lane per slot of the cas plan (chunk c of the cas message of file m):
// the lane reads content [1024c, 1024c + 1024) once and runs cas chunk c —
// message bytes [1024c, 1024c + 1024), i.e. content from 1024c - 8 — and
// checksum chunk c over it. One tile of the cas plan per workgroup.
__global__ void __launch_bounds__(kDualWG, 5)
    k_dual_leaf(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs, const uint64_t* __restrict__ lens,
                uint32_t n, const uint64_t* __restrict__ SA, const uint32_t* __restrict__ tfA,
                const uint64_t* __restrict__ totA_p, const uint64_t* __restrict__ SB,
                const uint64_t* __restrict__ totB_p, uint64_t cap, uint32_t* __restrict__ nodesA,
                uint32_t* __restrict__ nodesB, uint64_t* __restrict__ out_keys, uint8_t* __restrict__ out32,
                uint64_t* __restrict__ ctr) {
  __shared__ uint64_t sS[kTile + 1];
  const uint64_t totA = *totA_p, totB = *totB_p;
  const uint32_t tid = threadIdx.x;
  if (totA > cap || totB > cap) {  // reported through ws.total[0] by k_dual_scatter
    if (blockIdx.x == 0 && tid == 0) ctr[1] = 1;
    return;
  }
  const uint64_t ntiles = (totA + kTile - 1) / kTile;
  const uint64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  const uint64_t tbase = tile * kTile;
  const uint32_t m0 = tfA[tile];
  const uint32_t m1 = (tile + 1 < ntiles) ? tfA[tile + 1] : n - 1;
  const uint32_t cnt = m1 - m0 + 1;  // <= kTile + 1
  for (uint32_t i = tid; i < cnt; i += kDualWG) sS[i] = SA[m0 + i];
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = tid; s < kTile; s += kDualWG) {
    const uint64_t g = tbase + s;
    if (g >= totA) break;
    uint32_t lo = 0, hi = cnt - 1;  // last message with S <= g
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (sS[mid] <= g) lo = mid;
      else hi = mid - 1;
    }
    const uint32_t m = m0 + lo;
    const uint64_t len = lens[m];
    if (len == 0 || len > kWholeMax) continue;  // not the fused branch: the slot stays unused
    const uint32_t c = (uint32_t)(g - sS[lo]);  // chunk of both messages
    const uint32_t L = (uint32_t)len, c0off = c * CHUNK_LEN;
    const uint8_t* p = blob + offs[m] + c0off;
    // bytes of checksum chunk c (0: the cas message's extra chunk) and of cas chunk c
    const uint32_t clenB = L > c0off ? min(CHUNK_LEN, L - c0off) : 0u;
    const uint32_t clenA = min(CHUNK_LEN, L + 8 - c0off);
    const uint32_t nbB = (clenB + BLOCK_LEN - 1) / BLOCK_LEN, nbA = (clenA + BLOCK_LEN - 1) / BLOCK_LEN;  // nbB <= nbA <= nbB + 1
    const bool rootA = L + 8 <= CHUNK_LEN, rootB = L <= CHUNK_LEN;
    // the 8 message bytes before this chunk's content
    uint32_t k0, k1;
    if (c == 0) {
      k0 = L;
      k1 = 0;
    } else {
      const uint4 t = *reinterpret_cast<const uint4*>(p - 16);
      k0 = t.z;
      k1 = t.w;
      const uint32_t v = min(8u, L + 8 - c0off);  // of them, bytes of the file (the rest lie past its end)
      if (v < 8) {
        k1 = v > 4 ? k1 & ((1u << (8 * (v - 4))) - 1u) : 0u;
        if (v < 4) k0 &= (1u << (8 * v)) - 1u;
      }
    }
    uint32_t cvA[8], cvB[8];
    set_iv(cvA);
    set_iv(cvB);
#pragma unroll 1
    for (uint32_t b = 0; b < nbA; ++b) {
      uint32_t w[16];
      const bool hasB = b < nbB;
      if (hasB) {
        load_full_block(p + b * BLOCK_LEN, w);
        const uint32_t vb = clenB - b * BLOCK_LEN;  // content bytes of this block that the file holds
        if (vb < BLOCK_LEN) mask_tail_table(w, vb);
        compress<GSched::kAsmBlocks>(cvB, w, c, min(BLOCK_LEN, vb),
                    (b == 0 ? CHUNK_START : 0u) | (b + 1 == nbB ? CHUNK_END | (rootB ? ROOT : 0u) : 0u));
      } else {
        // the cas chain's extra block: only the carried words
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = 0;
      }
      const uint32_t mA[16] = {k0, k1, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13]};
      compress<GSched::kAsmBlocks>(cvA, mA, c, min(BLOCK_LEN, clenA - b * BLOCK_LEN),
                  (b == 0 ? CHUNK_START : 0u) | (b + 1 == nbA ? CHUNK_END | (rootA ? ROOT : 0u) : 0u));
      k0 = w[14];
      k1 = w[15];
    }
    if (rootA) {
      if (out_keys) out_keys[m] = cas_key(cvA);
    } else {
      store_cv(nodesA, g, cvA);
    }
    if (nbB) {
      if (rootB) store_digest(m, cvB, out32, nullptr);
      else store_cv(nodesB, SB[m] + c, cvB);
    }
  }
}

// The in-tile tree of one plan over chunk CVs that lie in the node workspace
// at their slots: k_leaf_tree's schedule (every aligned complete power-of-two
// node inside the tile, and the spine of each message lying wholly in it),
// its levels, and the export of a crossing message's maximal nodes, in place.
__global__ void __launch_bounds__(kTreeWG) k_dual_tree(const uint64_t* __restrict__ lens, uint32_t n,
                                                       const uint64_t* __restrict__ S,
                                                       const uint32_t* __restrict__ tile_first,
                                                       const uint64_t* __restrict__ total_p, uint64_t cap,
                                                       uint32_t* __restrict__ nodes, uint8_t* __restrict__ out32,
                                                       uint64_t* __restrict__ out_keys) {
  __shared__ uint32_t cvs[kTile][8];
  __shared__ uint64_t sS[kTile + 1];
  __shared__ uint16_t smsg[kTile];
  __shared__ uint32_t task[kTaskCap<kTile>];
  __shared__ uint32_t ntask[12];
  const uint64_t total = *total_p;
  if (total > cap) return;
  const uint64_t ntiles = (total + kTile - 1) / kTile;
  const uint64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  const uint32_t tid = threadIdx.x;
  const uint64_t tbase = tile * kTile;
  const uint32_t m0 = tile_first[tile];
  const uint32_t m1 = (tile + 1 < ntiles) ? tile_first[tile + 1] : n - 1;
  const uint32_t cnt = m1 - m0 + 1;
  for (uint32_t i = tid; i < cnt; i += kTreeWG) sS[i] = S[m0 + i];
  if (tid < 12) ntask[tid] = 0;
  __syncthreads();
  // (1) slot -> message, the chunk CVs, and the tree schedule
#pragma unroll 1
  for (uint32_t s = tid; s < kTile; s += kTreeWG) {
    const uint64_t g = tbase + s;
    if (g >= total) {
      smsg[s] = kNoMsg;
      continue;
    }
    uint32_t lo = 0, hi = cnt - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (sS[mid] <= g) lo = mid;
      else hi = mid - 1;
    }
    smsg[s] = (uint16_t)lo;
    const uint64_t j = g - sS[lo];
    const uint64_t C = chunk_count(lens[m0 + lo]);
    if (C == 1) continue;  // finished by its leaf
    const uint4* q = reinterpret_cast<const uint4*>(nodes + 8ull * g);
    const uint4 a = q[0], b = q[1];
    cvs[s][0] = a.x; cvs[s][1] = a.y; cvs[s][2] = a.z; cvs[s][3] = a.w;
    cvs[s][4] = b.x; cvs[s][5] = b.y; cvs[s][6] = b.z; cvs[s][7] = b.w;
    const uint32_t K = node_level_t<kTile>(j, C, s);
    for (uint32_t k = 1; k <= K; ++k)
      task[task_base<kTile>(k) + atomicAdd(&ntask[k], 1u)] = enc_task(s, s + (1u << (k - 1)), 0, false);
  }
#pragma unroll 1
  for (uint32_t i = tid; i < cnt; i += kTreeWG) {
    const uint64_t S0 = sS[i];
    if (S0 < tbase) continue;
    const uint64_t C = chunk_count(lens[m0 + i]);
    if (C == 1 || S0 + C > tbase + kTile) continue;
    const uint32_t s0 = (uint32_t)(S0 - tbase), c = (uint32_t)C;
    if (!(c & (c - 1))) {
      const uint32_t k = 31 - __clz(c);
      task[task_base<kTile>(k) + atomicAdd(&ntask[k], 1u)] = enc_task(s0, s0 + (c >> 1), i, true);
    } else {
      uint32_t rem = c, part = rem & (0u - rem);
      uint32_t pos = c - part, acc = pos;
      rem -= part;
      while (rem) {
        part = rem & (0u - rem);
        pos -= part;
        const uint32_t k = 32 - __clz(part);  // log2(part) + 1
        task[task_base<kTile>(k) + atomicAdd(&ntask[k], 1u)] = enc_task(s0 + pos, s0 + acc, i, rem == part);
        acc = pos;
        rem -= part;
      }
    }
  }
  __syncthreads();
  // (3) the tree, level by level
  for (uint32_t k = 1; k <= 10; ++k) {
    const uint32_t T = ntask[k];
    if (T == 0) continue;
#pragma unroll 1
    for (uint32_t t = tid; t < T; t += kTreeWG) {
      const uint32_t e = task[task_base<kTile>(k) + t];
      const uint32_t l = e & 1023u, r = (e >> 10) & 1023u;
      const bool root = e >> 31;
      uint32_t a[8], b[8], o[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        a[q] = cvs[l][q];
        b[q] = cvs[r][q];
      }
      parent<GSched::kAsmBlocks>(a, b, root, o);
      if (root) {
        store_digest(m0 + ((e >> 20) & 2047u), o, out32, out_keys);
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) cvs[l][q] = o[q];
      }
    }
    __syncthreads();
  }
  // (4) messages crossing a tile boundary: their maximal in-tile nodes, for the finish
#pragma unroll 1
  for (uint32_t s = tid; s < kTile; s += kTreeWG) {
    const uint32_t mi = smsg[s];
    if (mi == kNoMsg) continue;
    const uint64_t S0 = sS[mi];
    const uint64_t C = chunk_count(lens[m0 + mi]);
    if (C == 1 || (S0 >= tbase && S0 + C <= tbase + kTile)) continue;
    const uint64_t j = tbase + s - S0;
    const uint32_t k = node_level_t<kTile>(j, C, s);
    if (parent_in_tile_t<kTile>(j, C, s, k)) continue;
    uint4* o = reinterpret_cast<uint4*>(nodes + 8ull * (tbase + s));
    o[0] = make_uint4(cvs[s][0], cvs[s][1], cvs[s][2], cvs[s][3]);
    o[1] = make_uint4(cvs[s][4], cvs[s][5], cvs[s][6], cvs[s][7]);
  }
}

// The sampled branch's cas message of listed file r (cas.rs:31-58): le64(len),
// the header, four samples at 8192 + k * ((len - 16384) / 4) and the footer,
// copied into gather + r * kGatherStride eight bytes at a time (every piece
// starts and ends on a multiple of 8 message bytes), and the two message
// lists the batch kernels hash: the gathered messages and the files' contents.
// Entries past the list are empty messages at a readable address.
__global__ void __launch_bounds__(256) k_cas_gather(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs,
                                                    const uint64_t* __restrict__ lens,
                                                    const uint64_t* __restrict__ ctr,
                                                    const uint32_t* __restrict__ sidx, uint32_t G,
                                                    uint8_t* __restrict__ gather, uint64_t* __restrict__ goffs,
                                                    uint64_t* __restrict__ glens, uint64_t* __restrict__ coffs,
                                                    uint64_t* __restrict__ clens) {
  const uint32_t r = blockIdx.x, tid = threadIdx.x;
  const uint32_t cnt = min(*reinterpret_cast<const unsigned int*>(ctr), G);
  if (r >= G) return;
  if (r >= cnt) {
    if (tid == 0) {
      goffs[r] = 0;
      glens[r] = 0;
      coffs[r] = offs[0];
      clens[r] = 0;
    }
    return;
  }
  const uint32_t i = sidx[r];
  const uint64_t len = lens[i];
  const uint8_t* src = blob + offs[i];
  uint64_t* dst = reinterpret_cast<uint64_t*>(gather + (uint64_t)r * kGatherStride);
  if (tid == 0) {
    goffs[r] = (uint64_t)r * kGatherStride;
    glens[r] = kSampledLen;
    coffs[r] = offs[i];
    clens[r] = len;
  }
  const uint64_t jump = (len - 2 * kHeader) / 4;
  for (uint32_t q = tid; q < kGatherStride / 8; q += 256) {
    uint64_t v = 0;
    if (q == 0) {
      v = len;
    } else if (q < kSampledLen / 8) {
      const uint32_t x = 8 * q - 8;  // offset in header || samples || footer
      uint64_t so;
      if (x < kHeader) {
        so = x;
      } else if (x < kHeader + 4 * kSample) {
        const uint32_t k = (x - kHeader) / kSample;
        so = kHeader + k * jump + (x - kHeader - k * kSample);
      } else {
        so = len - kHeader + (x - kHeader - 4 * kSample);
      }
      __builtin_memcpy(&v, src + so, 8);
    }
    dst[q] = v;
  }
}

// The sampled files' results to their caller indices, and the call's
// capacity verdict: more files above kWholeMax than the scratch lists, or a
// plan past its half of the slots, leave UINT64_MAX in the workspace's total.
__global__ void __launch_bounds__(256) k_dual_scatter(const uint64_t* __restrict__ ctr,
                                                      const uint32_t* __restrict__ sidx, uint32_t G,
                                                      const uint64_t* __restrict__ tmpk,
                                                      const uint8_t* __restrict__ tmp32,
                                                      uint64_t* __restrict__ out_keys, uint8_t* __restrict__ out32,
                                                      uint64_t* __restrict__ ws_total) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t listed = *reinterpret_cast<const unsigned int*>(ctr);
  if (r == 0 && (listed > G || ctr[1])) ws_total[0] = ~0ull;
  if (r >= min(listed, G)) return;
  const uint32_t i = sidx[r];
  if (out_keys) out_keys[i] = tmpk[r];
  if (out32) {
    const uint4* s = reinterpret_cast<const uint4*>(tmp32 + 32ull * r);
    uint4* o = reinterpret_cast<uint4*>(out32 + 32ull * i);
    o[0] = s[0];
    o[1] = s[1];
  }
}

size_t identify_scratch_bytes(uint32_t n, uint32_t sampled_cap) { return id_layout(nullptr, n, sampled_cap).bytes; }

hipError_t identify_hash(const BatchWorkspace& ws, const IdentifyScratch& sc, const uint8_t* blob,
                         const uint64_t* offs, const uint64_t* lens, uint32_t n, uint32_t G, uint64_t* out_keys,
                         uint8_t* out32, uint8_t* out_has_key, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const IdLayout l = id_layout(sc.p, n, G);
  // each plan takes half of the workspace's slots (whole tiles)
  const uint64_t half_tiles = ws.cap_slots / kTile / 2;
  const uint64_t cap = half_tiles * kTile;
  if (!sc.p || l.bytes > sc.bytes || n > ws.cap_msgs || G > ws.cap_msgs || !half_tiles) return hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(l.ctr, 0, 16, st))) return e;
  hipLaunchKernelGGL(k_dual_prep, dim3((n + 255) / 256), dim3(256), 0, st, lens, n, l.dlA, l.dlB, l.ctr, l.sidx, G,
                     out32, out_has_key);
  uint32_t* tfA = ws.tile_first;
  uint32_t* tfB = ws.tile_first + half_tiles;
  uint32_t* nodesA = ws.nodes;
  uint32_t* nodesB = ws.nodes + 8 * cap;
  if ((e = plan_slots(l.dlA, n, ws.scan_tmp, ws.scan_tmp_bytes, cap, l.SA, tfA, l.totA, st))) return e;
  if ((e = plan_slots(l.dlB, n, ws.scan_tmp, ws.scan_tmp_bytes, cap, l.SB, tfB, l.totB, st))) return e;
  // the host never sees the lengths: grids cover what n files of the fused
  // branch can fill (101 cas chunks, 100 checksum chunks each)
  const uint32_t tilesA = (uint32_t)std::min<uint64_t>(half_tiles, (101ull * n + kTile - 1) / kTile);
  const uint32_t tilesB = (uint32_t)std::min<uint64_t>(half_tiles, (100ull * n + kTile - 1) / kTile);
  hipLaunchKernelGGL(k_dual_leaf, dim3(tilesA), dim3(kDualWG), 0, st, blob, offs, lens, n, l.SA, tfA, l.totA, l.SB,
                     l.totB, cap, nodesA, nodesB, out_keys, out32, l.ctr);
  if (out_keys) {
    hipLaunchKernelGGL(k_dual_tree, dim3(tilesA), dim3(kTreeWG), 0, st, l.dlA, n, l.SA, tfA, l.totA, cap, nodesA,
                       (uint8_t*)nullptr, out_keys);
    if ((e = finish_crossing(tilesA + 1, l.dlA, n, l.SA, tfA, l.totA, cap, nodesA, nullptr, out_keys, st))) return e;
  }
  if (out32) {
    hipLaunchKernelGGL(k_dual_tree, dim3(tilesB), dim3(kTreeWG), 0, st, l.dlB, n, l.SB, tfB, l.totB, cap, nodesB,
                       out32, (uint64_t*)nullptr);
    if ((e = finish_crossing(tilesB + 1, l.dlB, n, l.SB, tfB, l.totB, cap, nodesB, out32, nullptr, st))) return e;
  }
  if (G) {
    hipLaunchKernelGGL(k_cas_gather, dim3(G), dim3(256), 0, st, blob, offs, lens, l.ctr, l.sidx, G, l.gather, l.goffs,
                       l.glens, l.coffs, l.clens);
    if (out_keys && (e = batch_hash(ws, l.gather, l.goffs, l.glens, G, nullptr, l.tmpk, st))) return e;
    if (out32 && (e = batch_hash(ws, blob, l.coffs, l.clens, G, l.tmp32, nullptr, st))) return e;
  }
  hipLaunchKernelGGL(k_dual_scatter, dim3(std::max(1u, (G + 255) / 256)), dim3(256), 0, st, l.ctr, l.sidx, G, l.tmpk,
                     l.tmp32, out_keys, out32, ws.total);
  return hipGetLastError();
}

}  // namespace sdcas
