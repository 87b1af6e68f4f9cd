// cdc.hip — content-defined chunking of file contents resident in HBM, and the
// sharing pass over the chunks. Definitions: include/sdcas.h, DESIGN.md §3.5.
//
// The window hash h(p) depends on the 32 bytes ending at p, so every position
// is computed on its own: nothing is carried from tile to tile or from strip
// to strip but a warm-up over the 32 bytes before a strip.
//   k_cdc_sizes   per file: its bitmap slots, gear tiles and chunk bound
//   k_cdc_scan    one workgroup per array: the exclusive scans of those
//   k_cdc_gear    THE pass over every content byte. A workgroup takes a tile of
//                 kCdcTile bytes of one file into LDS with coalesced 16-byte
//                 loads; each lane runs a strip of kCdcStrip bytes (after the
//                 32 bytes before it, which lie in the file) through
//                 h = (h << 1) + G[byte], G in LDS (a unit's 16 entries read
//                 before the first is used, no branch per byte), and writes the strip's
//                 LOOSE and STRICT bits: a bitmap of 2 bits per position, so
//                 that memory is bounded whatever the content holds
//   k_cdc_cut     one wave per file walks its chain of cuts: 64 bitmap words
//                 (4096 positions) per step, the first lane with a candidate
//                 wins. Writes the file's ends and its chunk count
//   k_cdc_scan    the chunk counts become the files' first chunks
//   k_cdc_emit    chunks in file order: file_chunks, chunk_off, chunk_len,
//                 chunk_file (and the copies the pack and the host plan read)
//   k_cdc_pack    a batch's chunks copied to 16-byte aligned places for the
//                 batch hash (cut points fall on any byte)
// windows (a file chunked piece by piece, a long piece cut by many waves;
// DESIGN.md §3.6), in place of k_cdc_cut:
//   k_cdc_cut_seg one wave per segment: the chain from the segment's start
//   k_cdc_cut_win one wave per window below two segments: the whole chain
//   k_cdc_stitch  one wave per longer window: the true chain, walked only
//                 until it lands on a cut of the segment's own chain
//   k_cdc_gather  the cuts taken from the segments' lists, to their places
// sharing:
//   k_cs_accum    per chunk: new / self / other bytes of its file and, for a
//                 chunk first seen in another file, the bytes added to the
//                 pair's slot of an open-addressed table keyed (file, origin)
//   k_cs_max      per slot: the file's largest pair
//   k_cs_min      per slot equal to that maximum: the lowest origin
//   k_cs_write    per file: the outputs and files_with_peer
// Workgroups hand data to each other only across launches; within a launch the
// words another workgroup may touch are integer atomics whose result does not
// depend on order.
#include <hip/hip_runtime.h>

#include "../../include/sdcas_synth.h"
#include "cdc.h"
#include "wg_scan.h"

namespace sdcas {

// ---- host ------------------------------------------------------------------------------

CdcPlanError cdc_plan(const uint64_t* lens, size_t n, const CdcParams& p, uint64_t* max_chunks, uint64_t* max_slots) {
  if (!cdc_params_valid(p) || (n && !lens)) return kCdcInvalid;
  uint64_t chunks = 0, slots = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t len = lens[i];
    chunks += len / p.min_len + (len % p.min_len != 0);
    slots += len / kCdcSlot + (len % kCdcSlot != 0);
    if (chunks > kCdcMaxChunks) return kCdcCapacity;  // (no sum wraps: each term is below 2^59)
  }
  if (max_chunks) *max_chunks = chunks;
  if (max_slots) *max_slots = slots + chunks;
  return kCdcOk;
}

CdcLayout cdc_layout(uint64_t n, uint64_t max_chunks, uint64_t file_slots) {
  CdcLayout l{};
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  l.sb = take(4 * (n + 1)), l.tb = take(4 * (n + 1)), l.mcb = take(4 * (n + 1)), l.fcnt = take(4 * (n + 1));
  l.counts = take(64);
  l.ends = take(8 * max_chunks), l.woff = take(8 * max_chunks), l.wlen = take(8 * max_chunks);
  l.po = take(8 * max_chunks);
  l.bitmap = take(256 * file_slots);
  l.bytes = o;
  return l;
}

namespace {

constexpr uint32_t kStripUnits = kCdcStrip / 16;     // 16-byte units per strip
constexpr uint32_t kStripStride = kStripUnits + 1;    // in LDS, padded by one unit: ds_read_b128 at a
                                                      // lane stride of 144 B touches every bank once
constexpr uint32_t kUnitsPerSlot = kCdcSlot / kCdcStrip;
constexpr uint32_t kCutTB = 256;                      // the cut pass: 4 files per workgroup

inline uint32_t blocks_of(uint64_t m, uint32_t tb) { return m ? (uint32_t)((m + tb - 1) / tb) : 1u; }

template <typename T>
inline T* at(uint8_t* ws, uint64_t off) {
  return reinterpret_cast<T*>(ws + off);
}

// the largest i in [0, n) with base[i] <= x (base ascending, base[0] == 0)
__device__ __forceinline__ uint32_t cdc_owner(const uint32_t* __restrict__ base, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;  // base[lo] <= x < base[hi] (base[n] taken as above x)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (base[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t cdc_ceil_u32(uint64_t len, uint32_t d) {
  const uint64_t q = len / d + (len % d != 0);
  return q > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q;
}

__global__ void __launch_bounds__(256) k_cdc_sizes(const uint64_t* __restrict__ lens, uint32_t n, uint32_t min_len,
                                                   uint32_t* __restrict__ sb, uint32_t* __restrict__ tb,
                                                   uint32_t* __restrict__ mcb) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t len = lens[i];
  sb[i] = cdc_ceil_u32(len, kCdcSlot);
  tb[i] = cdc_ceil_u32(len, kCdcTile);
  mcb[i] = cdc_ceil_u32(len, min_len);
}

// workgroup b scans array b in place: a[i] <- the sum of a[0 .. i), a[n] <- the sum of all
__global__ void __launch_bounds__(1024) k_cdc_scan(uint32_t* __restrict__ a0, uint32_t* __restrict__ a1,
                                                    uint32_t* __restrict__ a2, uint32_t n) {
  uint32_t* a = blockIdx.x == 0 ? a0 : blockIdx.x == 1 ? a1 : a2;
  wg_scan_exclusive_1024(a, n, a + n);
}

// the table entries of a 16-byte unit, read before any of them is used: 16
// LDS reads in flight instead of one waited for per byte
__device__ __forceinline__ void cdc_gather(const uint32_t* sG, const uint4 v, uint32_t (&g)[16]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d)
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) g[4 * d + k] = sG[(w[d] >> (8 * k)) & 255u];
}

__global__ void __launch_bounds__(kCdcTB) k_cdc_gear(const uint8_t* __restrict__ blob,
                                                     const uint64_t* __restrict__ offs,
                                                     const uint64_t* __restrict__ lens, uint32_t n,
                                                     const uint32_t* __restrict__ tb,
                                                     const uint32_t* __restrict__ sb, uint64_t cap_units,
                                                     uint32_t loose_lim, uint32_t strict_lim,
                                                     uint4* __restrict__ bitmap) {
  __shared__ uint32_t sG[256];
  __shared__ uint4 sT[(kCdcTB + 1) * kStripStride];  // strip 0: the 32 bytes before the tile, in its last two units
  const uint32_t tid = threadIdx.x;
  sG[tid] = (uint32_t)(sds_mix64(kCdcGearSeed + tid) >> 32);
  const uint32_t tiles = tb[n];
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    __syncthreads();  // the table is written; the tile before is read
    const uint32_t i = cdc_owner(tb, n, t);
    const uint64_t tf = t - tb[i];  // the tile's index in its file
    const uint64_t len = lens[i];
    const uint64_t tile_at = tf * kCdcTile;
    if (tile_at >= len) continue;  // never: the tile counts come from these lengths (uniform over the workgroup)
    const uint64_t rem = len - tile_at;
    const uint32_t tile_bytes = rem < kCdcTile ? (uint32_t)rem : kCdcTile;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(blob + offs[i] + tile_at);
    const uint32_t units = (tile_bytes + 15) / 16;  // the last one may end up to 15 bytes past the file
#pragma unroll
    for (uint32_t it = 0; it < kCdcTile / 16 / kCdcTB; ++it) {
      const uint32_t g = it * kCdcTB + tid;
      if (g < units) sT[(1 + g / kStripUnits) * kStripStride + g % kStripUnits] = src[g];
    }
    if (tf > 0 && tid < 2) sT[kStripUnits - 2 + tid] = src[(int)tid - 2];  // inside the file: tile_at >= kCdcTile
    __syncthreads();
    const uint32_t p0 = tid * kCdcStrip;
    uint32_t lo[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0};
    if (p0 < tile_bytes) {
      uint32_t h = 0;
      if (tf > 0 || tid > 0) {
        // the 32 bytes before the strip: after them h holds what it holds
        // when run from the file's start
#pragma unroll
        for (uint32_t u = kStripUnits - 2; u < kStripUnits; ++u) {
          uint32_t g[16];
          cdc_gather(sG, sT[tid * kStripStride + u], g);
#pragma unroll
          for (uint32_t k = 0; k < 16; ++k) h = (h << 1) + g[k];
        }
      }
      // No branch per byte: the two tests shift into accumulators, the first
      // position of a word ending in its top bit; 32 positions later the word
      // is reversed into place.
      uint32_t la = 0, sa = 0;
#pragma unroll
      for (uint32_t u = 0; u < kStripUnits; ++u) {
        uint32_t g[16];
        cdc_gather(sG, sT[(tid + 1) * kStripStride + u], g);
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
          h = (h << 1) + g[k];
          la = (la << 1) | (h < loose_lim ? 1u : 0u);
          sa = (sa << 1) | (h < strict_lim ? 1u : 0u);
        }
        if (u % 2) lo[u / 2] = __brev(la), sr[u / 2] = __brev(sa);  // (la and sa need no clearing: 32 shifts empty them)
      }
      // positions at or past the file's end are no candidates
      const uint32_t valid = tile_bytes - p0;
      if (valid < kCdcStrip) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          const uint32_t keep = valid >= 32 * (q + 1) ? 0xFFFFFFFFu : valid <= 32 * q ? 0u : (1u << (valid - 32 * q)) - 1;
          lo[q] &= keep, sr[q] &= keep;
        }
      }
    }
    // every unit of the file's slots is written, so that the cut pass reads no stale word
    const uint64_t unit = tf * kCdcTB + tid;
    if (unit < (uint64_t)kUnitsPerSlot * (sb[i + 1] - sb[i])) {
      const uint64_t at = (uint64_t)kUnitsPerSlot * sb[i] + unit;
      if (at < cap_units) {
        bitmap[2 * at] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        bitmap[2 * at + 1] = make_uint4(sr[0], sr[1], sr[2], sr[3]);
      }
    }
  }
}

// the bits of 64-position word w that lie in [a, b)
__device__ __forceinline__ uint64_t cdc_range(uint64_t w, uint64_t a, uint64_t b) {
  const uint64_t w0 = 64 * w;
  const uint64_t from = a > w0 ? a : w0, to = b < w0 + 64 ? b : w0 + 64;
  if (from >= to) return 0;
  return (~0ull << (from - w0)) & (~0ull >> (64 - (to - w0)));
}

__global__ void __launch_bounds__(kCutTB) k_cdc_cut(const uint64_t* __restrict__ lens, uint32_t n,
                                                    const uint32_t* __restrict__ sb,
                                                    const uint32_t* __restrict__ mcb,
                                                    const uint64_t* __restrict__ bitmap, uint64_t cap_units,
                                                    uint32_t min_len, uint32_t avg_bits, uint32_t max_len,
                                                    uint64_t max_chunks, uint64_t* __restrict__ ends,
                                                    uint32_t* __restrict__ fcnt,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_bytes;
  __shared__ uint32_t s_kind[3];
  if (threadIdx.x == 0) s_bytes = 0;
  if (threadIdx.x < 3) s_kind[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * (kCutTB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i < n) {  // the same for the whole wave
    const uint64_t L = lens[i], avg = 1ull << avg_bits;
    const uint64_t base = mcb[i];
    uint64_t room = mcb[i + 1] - base;
    if (base + room > max_chunks) room = base < max_chunks ? max_chunks - base : 0;  // never, with a true plan
    const uint64_t ubase = (uint64_t)kUnitsPerSlot * sb[i];
    uint32_t cnt = 0, n_end = 0, n_hash = 0, n_max = 0;
    uint64_t s = 0;
    while (s < L && cnt < room) {
      uint64_t e = L;
      bool found = false;
      if (L - s > min_len) {
        const uint64_t hi = s + max_len < L ? s + max_len : L;
        // candidate positions q = e - 1 in [q_lo, hi): STRICT below q_mid, LOOSE from there on
        const uint64_t q_lo = s + min_len - 1, q_mid = s + avg - 1;
        const uint64_t strict_to = q_mid < hi ? q_mid : hi;
        e = hi;
        for (uint64_t w0 = q_lo / 64; 64 * w0 < hi; w0 += 64) {
          const uint64_t w = w0 + lane;
          uint64_t word = 0;
          const uint64_t unit = ubase + w / 2;
          if (64 * w < hi && unit < cap_units) {
            const uint64_t* p = bitmap + 4 * unit + (w & 1);
            word = (p[2] & cdc_range(w, q_lo, strict_to)) | (p[0] & cdc_range(w, q_mid, hi));
          }
          const uint64_t any = __ballot(word != 0);
          if (any) {
            const uint32_t first = (uint32_t)__builtin_ctzll(any);
            const uint32_t wl = __shfl((uint32_t)word, first), wh = __shfl((uint32_t)(word >> 32), first);
            const uint64_t hit = (uint64_t)wh << 32 | wl;
            e = 64 * (w0 + first) + (uint32_t)__builtin_ctzll(hit) + 1;
            found = true;
            break;
          }
        }
      }
      if (lane == 0) ends[base + cnt] = e;
      if (e == L) ++n_end; else if (found) ++n_hash; else ++n_max;
      ++cnt;
      s = e;
    }
    if (lane == 0) {
      fcnt[i] = cnt;
      if (s < L) atomicOr(&counts[7], 1ull);  // never: a file has at most ceil(L / min_len) chunks
      atomicAdd(&s_bytes, (unsigned long long)L);
      if (n_hash) atomicAdd(&s_kind[0], n_hash);
      if (n_max) atomicAdd(&s_kind[1], n_max);
      if (n_end) atomicAdd(&s_kind[2], n_end);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_bytes) atomicAdd(&counts[2], s_bytes);
  // counts [3..5]: hash_cuts, max_cuts, end_chunks
  if (threadIdx.x < 3 && s_kind[threadIdx.x]) atomicAdd(&counts[3 + threadIdx.x], (unsigned long long)s_kind[threadIdx.x]);
}

// slot k of the ends array belongs to the file owning it by mcb; its chunk, if
// it holds one, goes to fcnt[file] + its place in the file
__global__ void __launch_bounds__(256) k_cdc_emit(const uint64_t* __restrict__ offs, uint32_t n,
                                                  const uint32_t* __restrict__ mcb,
                                                  const uint32_t* __restrict__ fcnt,
                                                  const uint64_t* __restrict__ ends, uint64_t max_chunks,
                                                  uint64_t* __restrict__ woff, uint64_t* __restrict__ wlen,
                                                  uint64_t* __restrict__ file_chunks, uint64_t* __restrict__ chunk_off,
                                                  uint64_t* __restrict__ chunk_len, uint32_t* __restrict__ chunk_file,
                                                  unsigned long long* __restrict__ counts) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k == 0) counts[0] = n, counts[1] = fcnt[n];
  if (k <= n && file_chunks) file_chunks[k] = fcnt[k];
  if (n == 0 || k >= mcb[n] || k >= max_chunks) return;
  const uint32_t i = cdc_owner(mcb, n, (uint32_t)k);
  const uint32_t j = (uint32_t)k - mcb[i];
  if (j >= fcnt[i + 1] - fcnt[i]) return;
  const uint64_t c = (uint64_t)fcnt[i] + j;
  if (c >= max_chunks) return;  // never
  const uint64_t s = j ? ends[k - 1] : 0ull, e = ends[k];
  woff[c] = offs[i] + s;
  wlen[c] = e - s;
  if (chunk_off) chunk_off[c] = offs[i] + s;
  if (chunk_len) chunk_len[c] = e - s;
  if (chunk_file) chunk_file[c] = i;
}

constexpr uint32_t kPackPer = 8;  // 16-byte units per thread, kCdcTB apart

__global__ void __launch_bounds__(256) k_cdc_pack(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ woff,
                                                  const uint64_t* __restrict__ po, uint32_t nb, uint64_t units,
                                                  uint4* __restrict__ scratch) {
  uint64_t u = (uint64_t)blockIdx.x * (256 * kPackPer) + threadIdx.x;
  uint32_t c = 0;
  for (uint32_t it = 0; it < kPackPer && u < units; ++it, u += 256) {
    const uint64_t x = 16 * u;
    if (it == 0) {  // the largest c in [0, nb) with po[c] <= x
      uint32_t hi = nb;
      while (hi - c > 1) {
        const uint32_t mid = c + (hi - c) / 2;
        if (po[mid] <= x) c = mid; else hi = mid;
      }
    } else {
      while (c + 1 < nb && po[c + 1] <= x) ++c;
    }
    // 16 bytes from any address: the two aligned units around them. Both lie
    // at or above the chunk's file's start (16-byte aligned) and end less
    // than 32 bytes past the chunk's end.
    const uintptr_t src = (uintptr_t)blob + woff[c] + (x - po[c]);
    const uint4* al = reinterpret_cast<const uint4*>(src & ~(uintptr_t)15);
    const uint32_t mis = (uint32_t)(src & 15);
    const uint4 a = al[0];
    uint4 out = a;
    if (mis) {
      const uint4 b = al[1];
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      const uint32_t d = mis >> 2, sh = mis & 3;
      uint32_t t[5];
#pragma unroll
      for (uint32_t k = 0; k < 5; ++k) t[k] = d == 0 ? w[k] : d == 1 ? w[k + 1] : d == 2 ? w[k + 2] : w[k + 3];
      out.x = __builtin_amdgcn_alignbyte(t[1], t[0], sh);
      out.y = __builtin_amdgcn_alignbyte(t[2], t[1], sh);
      out.z = __builtin_amdgcn_alignbyte(t[3], t[2], sh);
      out.w = __builtin_amdgcn_alignbyte(t[4], t[3], sh);
    }
    scratch[u] = out;
  }
}

}  // namespace

hipError_t cdc_chunk(const CdcLayout& l, const CdcArgs& a, hipStream_t st) {
  const uint32_t n = a.n;
  uint32_t* sb = at<uint32_t>(a.ws, l.sb);
  uint32_t* tb = at<uint32_t>(a.ws, l.tb);
  uint32_t* mcb = at<uint32_t>(a.ws, l.mcb);
  uint32_t* fcnt = at<uint32_t>(a.ws, l.fcnt);
  unsigned long long* counts = at<unsigned long long>(a.ws, l.counts);
  const uint64_t cap_units = (uint64_t)kUnitsPerSlot * a.file_slots;
  hipError_t e;
  if ((e = hipMemsetAsync(counts, 0, 64, st))) return e;
  hipLaunchKernelGGL(k_cdc_sizes, dim3(blocks_of(n, 256)), dim3(256), 0, st, a.lens, n, a.p.min_len, sb, tb, mcb);
  hipLaunchKernelGGL(k_cdc_scan, dim3(3), dim3(1024), 0, st, sb, tb, mcb, n);
  // tiles <= file_slots / (kCdcTile / kCdcSlot) + n; the workgroups stride over them
  const uint64_t tiles_bound = a.file_slots / (kCdcTile / kCdcSlot) + n;
  const uint32_t gear_grid = (uint32_t)(tiles_bound < 8192 ? (tiles_bound ? tiles_bound : 1) : 8192);
  hipLaunchKernelGGL(k_cdc_gear, dim3(gear_grid), dim3(kCdcTB), 0, st, a.blob, a.offs, a.lens, n, (const uint32_t*)tb,
                     (const uint32_t*)sb, cap_units, 1u << (33 - a.p.avg_bits), 1u << (31 - a.p.avg_bits),
                     at<uint4>(a.ws, l.bitmap));
  hipLaunchKernelGGL(k_cdc_cut, dim3(blocks_of((uint64_t)n * 64, kCutTB)), dim3(kCutTB), 0, st, a.lens, n,
                     (const uint32_t*)sb, (const uint32_t*)mcb, at<const uint64_t>(a.ws, l.bitmap), cap_units,
                     a.p.min_len, a.p.avg_bits, a.p.max_len, a.max_chunks, at<uint64_t>(a.ws, l.ends), fcnt, counts);
  hipLaunchKernelGGL(k_cdc_scan, dim3(1), dim3(1024), 0, st, fcnt, fcnt, fcnt, n);
  const uint64_t slots = a.max_chunks > (uint64_t)n + 1 ? a.max_chunks : (uint64_t)n + 1;
  hipLaunchKernelGGL(k_cdc_emit, dim3(blocks_of(slots, 256)), dim3(256), 0, st, a.offs, n, (const uint32_t*)mcb,
                     (const uint32_t*)fcnt, at<const uint64_t>(a.ws, l.ends), a.max_chunks, at<uint64_t>(a.ws, l.woff),
                     at<uint64_t>(a.ws, l.wlen), a.file_chunks, a.chunk_off, a.chunk_len, a.chunk_file, counts);
  return hipGetLastError();
}

hipError_t cdc_pack(const CdcLayout& l, const CdcArgs& a, uint64_t c0, uint32_t nb, uint64_t total_bytes,
                    uint8_t* scratch, hipStream_t st) {
  const uint64_t units = total_bytes / 16;
  if (!nb || !units) return hipSuccess;
  hipLaunchKernelGGL(k_cdc_pack, dim3(blocks_of(units, 256 * kPackPer)), dim3(256), 0, st, a.blob,
                     at<const uint64_t>(a.ws, l.woff) + c0, at<const uint64_t>(a.ws, l.po) + c0, nb, units,
                     reinterpret_cast<uint4*>(scratch));
  return hipGetLastError();
}

// ---- windows ---------------------------------------------------------------------------
// A window begins at a cut of its file and, unless it is final, ends before the
// file does: its chain stops where the bytes it holds cannot decide the next
// cut. A window of 2 * seg bytes or more is cut by one wave per segment of seg
// bytes, each running the chain from its segment's start (the chain from a
// position is a function of that position alone), and stitched by one wave
// per file, which walks the true chain only until it lands on a cut the
// segment's wave made too.
//   k_cdc_cut_seg one wave per (file, segment): the cuts from the segment's
//                 start up to and including the first at or past its end, into
//                 the segment's own list, each with its kind
//   k_cdc_cut_win one wave per window without segments: k_cdc_cut's chain
//                 with the stop rule, into ends
//   k_cdc_stitch  one wave per window with segments (the wave of its first
//                 segment's slot). Segment by segment, from the true entry cut
//                 c: c at the segment's start takes the whole list; otherwise
//                 the chain is walked from c (its cuts go straight into ends)
//                 until a cut equals a listed one, whose followers are then
//                 taken, or until the segment's end. Writes per segment where
//                 its chunks begin in the file, the walked cuts, the merge
//                 index and the cuts taken from the list
//   k_cdc_gather  one wave per segment: the cuts taken from its list, to
//                 their places in ends; their kinds are counted
// The wave that stitches a file goes over its segments in order, so the running
// chunk count is the scan of the segments' counts. The true entry cut of
// segment j + 1 is below (j + 1) * seg + max_len, and seg >= 2 * max_len, so
// the chain never jumps a whole segment; k_cdc_stitch takes s / seg all the
// same and leaves a jumped segment's record at zero.

CdcWinLayout cdc_win_layout(uint64_t n, uint64_t max_chunks, uint64_t file_slots, const CdcParams& p, uint64_t seg) {
  CdcWinLayout w{};
  w.l = cdc_layout(n, max_chunks, file_slots);
  const uint64_t bound = (uint64_t)kCdcSlot * file_slots;  // the bytes of all windows, each rounded up to a slot
  w.max_segs = bound >= 2 * seg ? 3 * bound / (2 * seg) + 1 : 0;
  w.spl = w.max_segs ? seg / p.min_len + (seg % p.min_len != 0) : 0;
  uint64_t o = w.l.bytes;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 15) & ~15ull;
    return at;
  };
  w.gb = take(4 * (n + 1));
  w.scnt = take(4 * w.max_segs);
  w.srec = take(16 * w.max_segs);
  w.spec = take(8 * w.max_segs * w.spl);
  w.bytes = o;
  return w;
}

namespace {

constexpr uint32_t kStepHash = 0, kStepMax = 1, kStepEnd = 2, kStepStop = 3;  // the first three in counts[3..5]'s order
constexpr uint64_t kCutMask = (1ull << 62) - 1;                                 // a listed cut without its kind

// k_cdc_sizes and the windows' segment counts in one launch
__global__ void __launch_bounds__(256) k_cdc_win_sizes(const uint64_t* __restrict__ lens, uint32_t n, uint32_t min_len,
                                                       uint64_t seg, uint32_t* __restrict__ sb,
                                                       uint32_t* __restrict__ tb, uint32_t* __restrict__ mcb,
                                                       uint32_t* __restrict__ gb) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t len = lens[i];
  sb[i] = cdc_ceil_u32(len, kCdcSlot);
  tb[i] = cdc_ceil_u32(len, kCdcTile);
  mcb[i] = cdc_ceil_u32(len, min_len);
  const uint64_t q = len / seg + (len % seg != 0);
  gb[i] = len < 2 * seg ? 0u : q > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q;
}

// k_cdc_scan over four arrays
__global__ void __launch_bounds__(1024) k_cdc_win_scan(uint32_t* __restrict__ a0, uint32_t* __restrict__ a1,
                                                        uint32_t* __restrict__ a2, uint32_t* __restrict__ a3,
                                                        uint32_t n) {
  uint32_t* a = blockIdx.x == 0 ? a0 : blockIdx.x == 1 ? a1 : blockIdx.x == 2 ? a2 : a3;
  wg_scan_exclusive_1024(a, n, a + n);
}

struct CdcChain {
  const uint64_t* __restrict__ bitmap;
  uint64_t ubase, cap_units, L, avg;
  uint32_t min_len, max_len;
  bool fin;
};

// The cut after s (< L), by every lane of one wave: k_cdc_cut's step with the
// stop rule of a window that is not final. -> the kind; *out_e the cut unless
// the kind is kStepStop.
__device__ __forceinline__ uint32_t cdc_step(const CdcChain& c, uint64_t s, uint32_t lane, uint64_t* out_e) {
  const uint64_t left = c.L - s;
  *out_e = c.L;
  if (c.fin ? left <= c.min_len : left < c.min_len) return c.fin ? kStepEnd : kStepStop;
  const uint64_t hi = s + c.max_len < c.L ? s + c.max_len : c.L;
  // candidate positions q = e - 1 in [q_lo, hi): STRICT below q_mid, LOOSE from there on
  const uint64_t q_lo = s + c.min_len - 1, q_mid = s + c.avg - 1;
  const uint64_t strict_to = q_mid < hi ? q_mid : hi;
  for (uint64_t w0 = q_lo / 64; 64 * w0 < hi; w0 += 64) {
    const uint64_t w = w0 + lane;
    uint64_t word = 0;
    const uint64_t unit = c.ubase + w / 2;
    if (64 * w < hi && unit < c.cap_units) {
      const uint64_t* p = c.bitmap + 4 * unit + (w & 1);
      word = (p[2] & cdc_range(w, q_lo, strict_to)) | (p[0] & cdc_range(w, q_mid, hi));
    }
    const uint64_t any = __ballot(word != 0);
    if (any) {
      // (the ballot is the same in every lane: the winner's word comes down a scalar path)
      const uint32_t first = (uint32_t)__builtin_ctzll(any);
      const uint32_t wl = __builtin_amdgcn_readlane((uint32_t)word, first);
      const uint32_t wh = __builtin_amdgcn_readlane((uint32_t)(word >> 32), first);
      const uint64_t hit = (uint64_t)wh << 32 | wl;
      const uint64_t e = 64 * (w0 + first) + (uint32_t)__builtin_ctzll(hit) + 1;
      *out_e = e;
      return c.fin && e == c.L ? kStepEnd : kStepHash;
    }
  }
  if (s + c.max_len <= c.L) {
    *out_e = s + c.max_len;
    return c.fin && s + c.max_len == c.L ? kStepEnd : kStepMax;
  }
  return c.fin ? kStepEnd : kStepStop;  // the window ends before max_len does
}

struct CdcWinParams {
  uint32_t min_len, avg_bits, max_len;
  uint64_t seg, max_segs, spl, cap_units, max_chunks;
};

__device__ __forceinline__ CdcChain cdc_chain_of(const CdcWinParams& p, const uint64_t* __restrict__ bitmap,
                                                 const uint32_t* __restrict__ sb, const uint64_t* __restrict__ lens,
                                                 const uint8_t* __restrict__ final, uint32_t i) {
  return CdcChain{bitmap, (uint64_t)kUnitsPerSlot * sb[i], p.cap_units, lens[i], 1ull << p.avg_bits,
                  p.min_len, p.max_len, final ? final[i] != 0 : true};
}

__global__ void __launch_bounds__(kCutTB) k_cdc_cut_seg(const uint64_t* __restrict__ lens,
                                                        const uint8_t* __restrict__ final, uint32_t n,
                                                        const uint32_t* __restrict__ sb,
                                                        const uint32_t* __restrict__ gb,
                                                        const uint64_t* __restrict__ bitmap, CdcWinParams p,
                                                        uint64_t* __restrict__ spec, uint32_t* __restrict__ scnt,
                                                        uint4* __restrict__ srec,
                                                        unsigned long long* __restrict__ counts) {
  const uint64_t g = (uint64_t)blockIdx.x * (kCutTB / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t segs = gb[n] < p.max_segs ? gb[n] : p.max_segs;
  if (g >= segs) return;  // the same for the whole wave
  const uint32_t i = cdc_owner(gb, n, (uint32_t)g);
  const CdcChain c = cdc_chain_of(p, bitmap, sb, lens, final, i);
  uint64_t s = (g - gb[i]) * p.seg;
  const uint64_t limit = s + p.seg;
  uint64_t* __restrict__ list = spec + g * p.spl;
  uint32_t cnt = 0;
  while (s < c.L) {
    uint64_t e;
    const uint32_t kind = cdc_step(c, s, lane, &e);
    if (kind == kStepStop) break;
    if (cnt >= p.spl) {  // never: a list holds ceil(seg / min_len) cuts
      if (lane == 0) atomicOr(&counts[7], 1ull);
      break;
    }
    if (lane == 0) list[cnt] = e | (uint64_t)kind << 62;
    ++cnt;
    s = e;
    if (e >= limit) break;
  }
  if (lane == 0) {
    scnt[g] = cnt;
    srec[g] = make_uint4(0, 0, 0, 0);
  }
}

// what a window's wave leaves behind (lane 0) and the workgroup's sums
struct CdcWinSums {
  unsigned long long bytes;
  uint32_t kind[3], open;  // open: the windows that are not final
};
__device__ __forceinline__ void cdc_window_done(const CdcChain& c, uint32_t i, uint64_t s, uint32_t cnt, bool bad,
                                                uint32_t n_hash, uint32_t n_max, uint32_t n_end,
                                                uint32_t* __restrict__ fcnt, uint64_t* __restrict__ consumed,
                                                unsigned long long* __restrict__ counts, CdcWinSums* sums) {
  const uint64_t used = c.fin ? c.L : s;
  fcnt[i] = cnt;
  if (consumed) consumed[i] = used;
  if (bad || (c.fin && s < c.L)) atomicOr(&counts[7], 1ull);  // never: a window has at most ceil(L / min_len) chunks
  atomicAdd(&sums->bytes, (unsigned long long)used);
  if (!c.fin) atomicAdd(&sums->open, 1u);
  if (n_hash) atomicAdd(&sums->kind[kStepHash], n_hash);
  if (n_max) atomicAdd(&sums->kind[kStepMax], n_max);
  if (n_end) atomicAdd(&sums->kind[kStepEnd], n_end);
}
__device__ __forceinline__ void cdc_sums_clear(CdcWinSums* sums) {
  if (threadIdx.x == 0) sums->bytes = 0, sums->open = 0;
  if (threadIdx.x < 3) sums->kind[threadIdx.x] = 0;
  __syncthreads();
}
__device__ __forceinline__ void cdc_sums_add(const CdcWinSums* sums, unsigned long long* __restrict__ counts) {
  __syncthreads();
  if (threadIdx.x == 0 && sums->bytes) atomicAdd(&counts[2], sums->bytes);
  // (every add here goes to one word of all workgroups: the windows that are not final are counted, which
  // are none in a call over whole files, so that such a call adds to the words k_cdc_cut adds to and no more)
  if (threadIdx.x == 0 && sums->open) atomicAdd(&counts[6], (unsigned long long)sums->open);
  if (threadIdx.x < 3 && sums->kind[threadIdx.x]) atomicAdd(&counts[3 + threadIdx.x], (unsigned long long)sums->kind[threadIdx.x]);
}

// a window without segments: k_cdc_cut's one-wave chain with the stop rule
__global__ void __launch_bounds__(kCutTB) k_cdc_cut_win(const uint64_t* __restrict__ lens,
                                                        const uint8_t* __restrict__ final, uint32_t n,
                                                        const uint32_t* __restrict__ sb,
                                                        const uint32_t* __restrict__ mcb,
                                                        const uint32_t* __restrict__ gb,
                                                        const uint64_t* __restrict__ bitmap, CdcWinParams p,
                                                        uint64_t* __restrict__ ends, uint32_t* __restrict__ fcnt,
                                                        uint64_t* __restrict__ consumed,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ CdcWinSums sums;
  cdc_sums_clear(&sums);
  const uint32_t i = blockIdx.x * (kCutTB / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i < n && gb[i + 1] == gb[i]) {  // the same for the whole wave
    const CdcChain c = cdc_chain_of(p, bitmap, sb, lens, final, i);
    const uint64_t base = mcb[i];
    uint64_t room = mcb[i + 1] - base;
    if (base + room > p.max_chunks) room = base < p.max_chunks ? p.max_chunks - base : 0;  // never, with a true plan
    uint32_t cnt = 0, n_hash = 0, n_max = 0, n_end = 0;
    uint64_t s = 0;
    bool bad = false;
    while (s < c.L) {
      uint64_t e;
      const uint32_t kind = cdc_step(c, s, lane, &e);
      if (kind == kStepStop) break;
      if (cnt >= room) {
        bad = true;
        break;
      }
      if (lane == 0) ends[base + cnt] = e;
      if (kind == kStepHash) ++n_hash; else if (kind == kStepMax) ++n_max; else ++n_end;
      ++cnt;
      s = e;
    }
    if (lane == 0) cdc_window_done(c, i, s, cnt, bad, n_hash, n_max, n_end, fcnt, consumed, counts, &sums);
  } else if (i < n && gb[i + 1] > p.max_segs && lane == 0) {
    // never, with a true plan: segments past the workspace's, which no wave stitches
    fcnt[i] = 0;
    if (consumed) consumed[i] = 0;
    atomicOr(&counts[7], 1ull);
  }
  cdc_sums_add(&sums, counts);
}

// a window with segments: the wave of its first segment's slot stitches it
__global__ void __launch_bounds__(kCutTB) k_cdc_stitch(const uint64_t* __restrict__ lens,
                                                       const uint8_t* __restrict__ final, uint32_t n,
                                                       const uint32_t* __restrict__ sb,
                                                       const uint32_t* __restrict__ mcb,
                                                       const uint32_t* __restrict__ gb,
                                                       const uint64_t* __restrict__ bitmap, CdcWinParams p,
                                                       const uint64_t* __restrict__ spec,
                                                       const uint32_t* __restrict__ scnt, uint4* __restrict__ srec,
                                                       uint64_t* __restrict__ ends, uint32_t* __restrict__ fcnt,
                                                       uint64_t* __restrict__ consumed,
                                                       unsigned long long* __restrict__ counts) {
  __shared__ CdcWinSums sums;
  cdc_sums_clear(&sums);
  const uint64_t g0 = (uint64_t)blockIdx.x * (kCutTB / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t segs = gb[n] < p.max_segs ? gb[n] : p.max_segs;
  const uint32_t i = g0 < segs ? cdc_owner(gb, n, (uint32_t)g0) : 0u;
  if (g0 < segs && gb[i] == g0 && gb[i + 1] <= p.max_segs) {  // the same for the whole wave
    const CdcChain c = cdc_chain_of(p, bitmap, sb, lens, final, i);
    const uint64_t base = mcb[i];
    uint64_t room = mcb[i + 1] - base;
    if (base + room > p.max_chunks) room = base < p.max_chunks ? p.max_chunks - base : 0;  // never, with a true plan
    uint32_t cnt = 0, n_hash = 0, n_max = 0, n_end = 0;
    uint64_t s = 0;
    bool bad = false;
    while (s < c.L && !bad) {
      const uint64_t j = s / p.seg;
      const uint64_t g = g0 + j, limit = (j + 1) * p.seg;
      if (g >= segs) {  // never, with a true plan
        bad = true;
        break;
      }
      const uint64_t* __restrict__ list = spec + g * p.spl;
      const uint32_t sc = scnt[g] < p.spl ? scnt[g] : (uint32_t)p.spl;
      const uint32_t start = cnt;
      uint32_t walk = 0, merge = 0, take = 0;
      bool stopped = false;
      if (s == j * p.seg) {
        take = sc;  // the segment's wave began where the true chain enters
      } else {
        uint32_t k = 0;
        for (;;) {
          uint64_t e;
          const uint32_t kind = cdc_step(c, s, lane, &e);
          if (kind == kStepStop) {
            stopped = true;
            break;
          }
          if (cnt >= room) {
            bad = true;
            break;
          }
          if (lane == 0) ends[base + cnt] = e;
          if (kind == kStepHash) ++n_hash; else if (kind == kStepMax) ++n_max; else ++n_end;
          ++cnt, ++walk;
          s = e;
          while (k < sc && (list[k] & kCutMask) < e) ++k;
          if (k < sc && (list[k] & kCutMask) == e) {  // from here on the list is the true chain
            merge = k + 1, take = sc - merge;
            break;
          }
          if (e >= limit) break;
        }
      }
      if (take > room - cnt) take = (uint32_t)(room - cnt), bad = true;
      if (take) s = list[merge + take - 1] & kCutMask, cnt += take;
      if (lane == 0) srec[g] = make_uint4(start, walk, merge, take);
      if (stopped || s < limit) break;  // the chain stopped, or ended, inside this segment
    }
    if (lane == 0) cdc_window_done(c, i, s, cnt, bad, n_hash, n_max, n_end, fcnt, consumed, counts, &sums);
  }
  cdc_sums_add(&sums, counts);
}

__global__ void __launch_bounds__(kCutTB) k_cdc_gather(uint32_t n, const uint32_t* __restrict__ mcb,
                                                       const uint32_t* __restrict__ gb, CdcWinParams p,
                                                       const uint64_t* __restrict__ spec,
                                                       const uint4* __restrict__ srec, uint64_t* __restrict__ ends,
                                                       unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_kind[3];
  if (threadIdx.x < 3) s_kind[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t g = (uint64_t)blockIdx.x * (kCutTB / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t segs = gb[n] < p.max_segs ? gb[n] : p.max_segs;
  if (g < segs) {  // the same for the whole wave
    const uint4 rec = srec[g];  // start, walk, merge, take
    if (rec.w) {
      const uint32_t i = cdc_owner(gb, n, (uint32_t)g);
      const uint64_t base = mcb[i];
      uint64_t room = mcb[i + 1] - base;
      if (base + room > p.max_chunks) room = base < p.max_chunks ? p.max_chunks - base : 0;
      const uint64_t first = (uint64_t)rec.x + rec.y;  // the segment's taken cuts follow its walked ones
      uint32_t kinds[3] = {0, 0, 0};
      for (uint32_t k0 = 0; k0 < rec.w; k0 += 64) {
        const uint32_t k = k0 + lane;
        uint32_t kind = kStepStop;
        if (k < rec.w && (uint64_t)rec.z + k < p.spl && first + k < room) {
          const uint64_t v = spec[g * p.spl + rec.z + k];
          ends[base + first + k] = v & kCutMask;
          kind = (uint32_t)(v >> 62);
        }
#pragma unroll
        for (uint32_t t = 0; t < 3; ++t) kinds[t] += (uint32_t)__popcll(__ballot(kind == t));
      }
      if (lane == 0) {
#pragma unroll
        for (uint32_t t = 0; t < 3; ++t)
          if (kinds[t]) atomicAdd(&s_kind[t], kinds[t]);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_kind[threadIdx.x]) atomicAdd(&counts[3 + threadIdx.x], (unsigned long long)s_kind[threadIdx.x]);
}

// after k_cdc_emit, which counts every entry as a file: `files` counts the final windows
__global__ void k_cdc_win_finish(uint32_t n, unsigned long long* __restrict__ counts) { counts[0] = n - counts[6]; }

}  // namespace

hipError_t cdc_chunk_windows(const CdcWinLayout& w, const CdcArgs& a, const CdcWinArgs& wa, hipStream_t st) {
  const CdcLayout& l = w.l;
  const uint32_t n = a.n;
  uint32_t* sb = at<uint32_t>(a.ws, l.sb);
  uint32_t* tb = at<uint32_t>(a.ws, l.tb);
  uint32_t* mcb = at<uint32_t>(a.ws, l.mcb);
  uint32_t* fcnt = at<uint32_t>(a.ws, l.fcnt);
  uint32_t* gb = at<uint32_t>(a.ws, w.gb);
  uint32_t* scnt = at<uint32_t>(a.ws, w.scnt);
  uint4* srec = at<uint4>(a.ws, w.srec);
  uint64_t* spec = at<uint64_t>(a.ws, w.spec);
  unsigned long long* counts = at<unsigned long long>(a.ws, l.counts);
  const uint64_t* bitmap = at<const uint64_t>(a.ws, l.bitmap);
  const uint64_t cap_units = (uint64_t)kUnitsPerSlot * a.file_slots;
  const CdcWinParams p{a.p.min_len, a.p.avg_bits, a.p.max_len, wa.seg, w.max_segs, w.spl, cap_units, a.max_chunks};
  hipError_t e;
  if ((e = hipMemsetAsync(counts, 0, 64, st))) return e;
  hipLaunchKernelGGL(k_cdc_win_sizes, dim3(blocks_of(n, 256)), dim3(256), 0, st, a.lens, n, a.p.min_len, wa.seg, sb, tb,
                     mcb, gb);
  hipLaunchKernelGGL(k_cdc_win_scan, dim3(4), dim3(1024), 0, st, sb, tb, mcb, gb, n);
  const uint64_t tiles_bound = a.file_slots / (kCdcTile / kCdcSlot) + n;
  const uint32_t gear_grid = (uint32_t)(tiles_bound < 8192 ? (tiles_bound ? tiles_bound : 1) : 8192);
  hipLaunchKernelGGL(k_cdc_gear, dim3(gear_grid), dim3(kCdcTB), 0, st, a.blob, a.offs, a.lens, n, (const uint32_t*)tb,
                     (const uint32_t*)sb, cap_units, 1u << (33 - a.p.avg_bits), 1u << (31 - a.p.avg_bits),
                     at<uint4>(a.ws, l.bitmap));
  const dim3 seg_grid(blocks_of(w.max_segs * 64, kCutTB));
  if (w.max_segs)
    hipLaunchKernelGGL(k_cdc_cut_seg, seg_grid, dim3(kCutTB), 0, st, a.lens, wa.final, n, (const uint32_t*)sb,
                       (const uint32_t*)gb, bitmap, p, spec, scnt, srec, counts);
  hipLaunchKernelGGL(k_cdc_cut_win, dim3(blocks_of((uint64_t)n * 64, kCutTB)), dim3(kCutTB), 0, st, a.lens, wa.final, n,
                     (const uint32_t*)sb, (const uint32_t*)mcb, (const uint32_t*)gb, bitmap, p,
                     at<uint64_t>(a.ws, l.ends), fcnt, wa.consumed, counts);
  if (w.max_segs)
    hipLaunchKernelGGL(k_cdc_stitch, seg_grid, dim3(kCutTB), 0, st, a.lens, wa.final, n, (const uint32_t*)sb,
                       (const uint32_t*)mcb, (const uint32_t*)gb, bitmap, p, (const uint64_t*)spec,
                       (const uint32_t*)scnt, srec, at<uint64_t>(a.ws, l.ends), fcnt, wa.consumed, counts);
  if (w.max_segs)
    hipLaunchKernelGGL(k_cdc_gather, seg_grid, dim3(kCutTB), 0, st, n, (const uint32_t*)mcb, (const uint32_t*)gb, p,
                       (const uint64_t*)spec, (const uint4*)srec, at<uint64_t>(a.ws, l.ends), counts);
  hipLaunchKernelGGL(k_cdc_scan, dim3(1), dim3(1024), 0, st, fcnt, fcnt, fcnt, n);
  const uint64_t slots = a.max_chunks > (uint64_t)n + 1 ? a.max_chunks : (uint64_t)n + 1;
  hipLaunchKernelGGL(k_cdc_emit, dim3(blocks_of(slots, 256)), dim3(256), 0, st, a.offs, n, (const uint32_t*)mcb,
                     (const uint32_t*)fcnt, at<const uint64_t>(a.ws, l.ends), a.max_chunks, at<uint64_t>(a.ws, l.woff),
                     at<uint64_t>(a.ws, l.wlen), a.file_chunks, a.chunk_off, a.chunk_len, a.chunk_file, counts);
  hipLaunchKernelGGL(k_cdc_win_finish, dim3(1), dim3(1), 0, st, n, counts);
  return hipGetLastError();
}

// ---- sharing ---------------------------------------------------------------------------

namespace {

constexpr uint32_t kCsTB = 256;
constexpr unsigned long long kCsEmpty = ~0ull;

__device__ __forceinline__ uint64_t cs_mix(uint64_t x) {
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  return x;
}
__device__ __forceinline__ unsigned long long cs_wave_sum(unsigned long long v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ unsigned long long cs_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A chunk whose file lies outside [0, n_files) takes no part. rep outside
// [0, c], or naming such a chunk, counts as c; it is never used as an index
// otherwise.
__global__ void __launch_bounds__(kCsTB) k_cs_accum(const uint32_t* __restrict__ chunk_file,
                                                    const uint64_t* __restrict__ chunk_len,
                                                    const int64_t* __restrict__ rep, uint32_t m, uint32_t n_files,
                                                    unsigned long long* __restrict__ acc_new,
                                                    unsigned long long* __restrict__ acc_self,
                                                    unsigned long long* __restrict__ acc_other,
                                                    unsigned long long* __restrict__ tab_key,
                                                    unsigned long long* __restrict__ tab_val, uint32_t mask,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_sum[4];  // chunks, distinct_chunks, total_bytes, stored_bytes
  if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * kCsTB + threadIdx.x;
  uint32_t f = 0xFFFFFFFFu, o = 0xFFFFFFFFu;
  unsigned long long len = 0;
  bool act = false, first = false;
  if (c < m) {
    f = chunk_file[c];
    act = f < n_files;
  }
  if (act) {
    len = chunk_len[c];
    const int64_t r = rep[c];
    first = true;
    if (r >= 0 && r < (int64_t)c) {
      o = chunk_file[r];
      first = o >= n_files;
    }
  }
  const unsigned long long add_new = act && first ? len : 0ull;
  const unsigned long long add_self = act && !first && o == f ? len : 0ull;
  const unsigned long long add_other = act && !first && o != f ? len : 0ull;
  // one file over the whole wave (any file of 64 chunks or more): one add per
  // word instead of 64 on the same word
  const uint32_t f0 = __builtin_amdgcn_readfirstlane(f);
  if (__all(f == f0)) {
    const unsigned long long a = cs_wave_sum(add_new), b = cs_wave_sum(add_self), d = cs_wave_sum(add_other);
    if ((threadIdx.x & 63) == 0 && f0 < n_files) {
      if (a) atomicAdd(&acc_new[f0], a);
      if (b) atomicAdd(&acc_self[f0], b);
      if (d) atomicAdd(&acc_other[f0], d);
    }
  } else if (act) {
    if (add_new) atomicAdd(&acc_new[f], add_new);
    if (add_self) atomicAdd(&acc_self[f], add_self);
    if (add_other) atomicAdd(&acc_other[f], add_other);
  }
  // the pair's slot: claimed by CAS, then the bytes added (zero bytes too: the
  // slot's value stays 0 and is no peer)
  if (act && !first && o != f) {
    const unsigned long long key = (unsigned long long)f << 32 | o;
    uint32_t h = (uint32_t)cs_mix(key) & mask;
    for (;;) {
      unsigned long long cur = cs_load(&tab_key[h]);
      if (cur == kCsEmpty) {
        const unsigned long long prev = atomicCAS(&tab_key[h], kCsEmpty, key);
        cur = prev == kCsEmpty ? key : prev;
      }
      if (cur == key) break;
      h = (h + 1) & mask;
    }
    if (len) atomicAdd(&tab_val[h], len);
  }
  const unsigned long long sums[4] = {act ? 1ull : 0ull, act && first ? 1ull : 0ull, act ? len : 0ull, add_new};
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const unsigned long long v = cs_wave_sum(sums[k]);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_sum[k], v);
  }
  __syncthreads();
  // counts: files, chunks, distinct_chunks, total_bytes, stored_bytes, files_with_peer
  if (threadIdx.x < 4 && s_sum[threadIdx.x]) atomicAdd(&counts[1 + threadIdx.x], s_sum[threadIdx.x]);
}

__global__ void __launch_bounds__(kCsTB) k_cs_max(const unsigned long long* __restrict__ tab_key,
                                                  const unsigned long long* __restrict__ tab_val, uint64_t cap,
                                                  uint32_t n_files, unsigned long long* __restrict__ pmax) {
  const uint64_t h = (uint64_t)blockIdx.x * kCsTB + threadIdx.x;
  if (h >= cap) return;
  const unsigned long long key = tab_key[h], val = tab_val[h];
  const uint32_t f = (uint32_t)(key >> 32);
  if (key == kCsEmpty || !val || f >= n_files) return;
  if (cs_load(&pmax[f]) < val) atomicMax(&pmax[f], val);
}

__global__ void __launch_bounds__(kCsTB) k_cs_min(const unsigned long long* __restrict__ tab_key,
                                                  const unsigned long long* __restrict__ tab_val, uint64_t cap,
                                                  uint32_t n_files, const unsigned long long* __restrict__ pmax,
                                                  uint32_t* __restrict__ pmin) {
  const uint64_t h = (uint64_t)blockIdx.x * kCsTB + threadIdx.x;
  if (h >= cap) return;
  const unsigned long long key = tab_key[h], val = tab_val[h];
  const uint32_t f = (uint32_t)(key >> 32);
  if (key == kCsEmpty || !val || f >= n_files) return;
  if (val == pmax[f]) atomicMin(&pmin[f], (uint32_t)key);
}

__global__ void __launch_bounds__(kCsTB) k_cs_write(uint32_t n_files, const unsigned long long* __restrict__ acc_new,
                                                    const unsigned long long* __restrict__ acc_self,
                                                    const unsigned long long* __restrict__ acc_other,
                                                    const unsigned long long* __restrict__ pmax,
                                                    const uint32_t* __restrict__ pmin, uint64_t* __restrict__ new_bytes,
                                                    uint64_t* __restrict__ self_bytes, uint64_t* __restrict__ other_bytes,
                                                    int64_t* __restrict__ peer, uint64_t* __restrict__ peer_bytes,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_peers;
  if (threadIdx.x == 0) s_peers = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kCsTB + threadIdx.x;
  bool has = false;
  if (i < n_files) {
    const uint32_t p = pmin[i];
    has = p != 0xFFFFFFFFu;
    if (new_bytes) new_bytes[i] = acc_new[i];
    if (self_bytes) self_bytes[i] = acc_self[i];
    if (other_bytes) other_bytes[i] = acc_other[i];
    if (peer) peer[i] = has ? (int64_t)p : -1;
    if (peer_bytes) peer_bytes[i] = has ? pmax[i] : 0ull;
  }
  const uint32_t cnt = (uint32_t)__popcll(__ballot(has));
  if (cnt && (threadIdx.x & 63) == 0) atomicAdd(&s_peers, cnt);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_peers) atomicAdd(&counts[5], (unsigned long long)s_peers);
    if (blockIdx.x == 0) atomicAdd(&counts[0], (unsigned long long)n_files);
  }
}

}  // namespace

hipError_t cdc_sharing(uint8_t* ws, const uint32_t* chunk_file, const uint64_t* chunk_len, const int64_t* rep,
                       uint32_t m, uint32_t n_files, uint64_t* new_bytes, uint64_t* self_bytes,
                       uint64_t* other_bytes, int64_t* peer, uint64_t* peer_bytes, unsigned long long* counts,
                       hipStream_t st) {
  const uint64_t cap = cdc_share_cap(m), nf = ((uint64_t)n_files + 1) & ~1ull;
  unsigned long long* tab_key = at<unsigned long long>(ws, 0);
  unsigned long long* tab_val = tab_key + cap;
  unsigned long long* acc_new = tab_val + cap;
  unsigned long long* acc_self = acc_new + nf;
  unsigned long long* acc_other = acc_self + nf;
  unsigned long long* pmax = acc_other + nf;
  uint32_t* pmin = reinterpret_cast<uint32_t*>(pmax + nf);
  unsigned long long* cts = reinterpret_cast<unsigned long long*>(pmin + 2 * nf);  // (pmin takes 4 of its 8 bytes per file)
  hipError_t e;
  if ((e = hipMemsetAsync(tab_key, 0xFF, 8 * cap, st))) return e;
  if ((e = hipMemsetAsync(tab_val, 0, 8 * (cap + 4 * nf), st))) return e;  // the values, the three sums, the maxima
  if ((e = hipMemsetAsync(pmin, 0xFF, 8 * nf, st))) return e;
  if ((e = hipMemsetAsync(cts, 0, 64, st))) return e;
  if (m)
    hipLaunchKernelGGL(k_cs_accum, dim3(blocks_of(m, kCsTB)), dim3(kCsTB), 0, st, chunk_file, chunk_len, rep, m, n_files,
                       acc_new, acc_self, acc_other, tab_key, tab_val, (uint32_t)(cap - 1), cts);
  if (m) {
    hipLaunchKernelGGL(k_cs_max, dim3(blocks_of(cap, kCsTB)), dim3(kCsTB), 0, st, (const unsigned long long*)tab_key,
                       (const unsigned long long*)tab_val, cap, n_files, pmax);
    hipLaunchKernelGGL(k_cs_min, dim3(blocks_of(cap, kCsTB)), dim3(kCsTB), 0, st, (const unsigned long long*)tab_key,
                       (const unsigned long long*)tab_val, cap, n_files, (const unsigned long long*)pmax, pmin);
  }
  hipLaunchKernelGGL(k_cs_write, dim3(blocks_of(n_files, kCsTB)), dim3(kCsTB), 0, st, n_files,
                     (const unsigned long long*)acc_new, (const unsigned long long*)acc_self,
                     (const unsigned long long*)acc_other, (const unsigned long long*)pmax, (const uint32_t*)pmin,
                     new_bytes, self_bytes, other_bytes, peer, peer_bytes, cts);
  if ((e = hipGetLastError())) return e;
  if (counts) return hipMemcpyAsync(counts, cts, kCdcCounts * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  return hipSuccess;
}

}  // namespace sdcas
