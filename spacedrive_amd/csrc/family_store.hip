// family_store.hip — the family store: the literal ranges of the family recipes
// gathered into one dense store, every op pointed at its place there, and the
// byte mover between file windows and the store (include/sdcas.h has the
// definition; family_store.h the workspace).
// The layout:
//   k_fs_sum      per workgroup of ops the sum of its literal ops' lengths; the
//                 literal and copy ops counted
//   k_fs_scan     the workgroup sums become offsets (one workgroup, u64), their
//                 total the store's bytes
//   k_fs_literal  a literal op's offset: its workgroup's plus the literal bytes
//                 before it there
//   k_fs_copy     a copy op through chunk_op to the literal op that holds its
//                 source; covered or not
//   k_fs_counts   the counts
// The mover, one form for both directions:
//   k_fs_clip     per op: bad or not, its range clipped to its row's window, its
//                 tiles; where the clipped bytes come from and go to
//   k_fs_scan     the workgroup tile counts become offsets
//   k_fs_starts   per op the tiles before it
//   k_fs_move     a constant grid; every workgroup takes a contiguous share of
//                 the tiles, finds its first tile's op by a search in the tile
//                 starts and walks on from there (a galloping search from the
//                 op it is at: two loads where every tile is an op of its own)
//   k_fs_moved    the counts
// A tile is kFamilyStoreTile destination bytes cut at 16-byte aligned
// destination addresses, so only an op's first and last 16-byte unit can be
// partial. A thread moves whole units: the source through the aligned
// granules around them, shifted into place as k_cdc_pack does, one 16-byte
// store for a full unit and byte stores for a partial one. A granule is read
// only when it holds a source byte; a byte is written only when it is a
// destination byte. One unaligned 16-byte load per full unit in place of the
// two granules and the shift was measured and lost.
//
// Visibility as in family_recipes.hip: the counters are touched only by
// agent-scope atomics and relaxed agent-scope atomic loads; every phase is a
// launch of its own; arrays that one launch writes with plain stores are read by
// later launches with plain loads. No thread waits for another. The sums are
// integer and every op's offset is a function of the ops below it: results do
// not depend on scheduling.
#include <hip/hip_runtime.h>

#include "chunk_index.h"
#include "family_bytes_device.h"
#include "family_store.h"

namespace sdcas {

namespace {

constexpr uint32_t kTB = kFamilyStoreTB;
constexpr uint32_t kWaves = kTB / 64;
constexpr uint64_t kNone = kFamilyStoreNone;
constexpr uint64_t kTile = kFamilyStoreTile;
enum { kScLitOps, kScCopyOps, kScUncOps, kScUncBytes, kScMoved, kScMovedBytes, kScBad };

__device__ __forceinline__ u64a* fs_sc(u64a* sc, uint32_t k) {
  return &sc[(blockIdx.x & (kFamilyStoreScCopies - 1)) * 16 + k];
}
__device__ __forceinline__ uint64_t fs_fold(const u64a* sc, uint32_t k) {
  uint64_t v = 0;
  for (uint32_t r = 0; r < kFamilyStoreScCopies; ++r) v += fb_load(&sc[r * 16 + k]);
  return v;
}

__device__ __forceinline__ uint32_t fs_ops(const FamilyStoreOps& in) {
  const uint64_t n = in.d_ops[0];
  return n < in.max_ops ? (uint32_t)n : in.max_ops;
}

// Called by every thread of a workgroup of kTB: the sum of v over the
// workgroup, valid in thread 0; excl <- the sum over the threads below.
__device__ __forceinline__ uint64_t fs_wg_scan(uint64_t v, uint64_t& excl) {
  __shared__ u64a s_w[kWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up((u64a)inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    if (w < wave) before += s_w[w];
    all += s_w[w];
  }
  excl = before + inc - v;
  return all;
}

// wg_scan.h's scan over u64: cnt[b] <- the sum of cnt[0 .. b); *total <- the sum of all
__global__ void __launch_bounds__(1024) k_fs_scan(uint64_t* __restrict__ cnt, uint32_t nb,
                                                  uint64_t* __restrict__ total) {
  __shared__ u64a ws[16];
  __shared__ u64a carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += 1024) {
    const uint32_t i = base + tid;
    const uint64_t v = i < nb ? cnt[i] : 0ull;
    uint64_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint64_t t = __shfl_up((u64a)inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint64_t before = carry;
    for (uint32_t w = 0; w < wave; ++w) before += ws[w];
    if (i < nb) cnt[i] = before + inc - v;
    __syncthreads();
    if (tid == 1023) carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// ---- the layout ----------------------------------------------------------------------

__device__ __forceinline__ bool fs_literal(const FamilyStoreOps& in, uint32_t o) {
  return in.op_chunk[o] == in.op_src_chunk[o];
}

__global__ void __launch_bounds__(kTB) k_fs_sum(FamilyStoreOps in, uint64_t* __restrict__ gsum, u64a* sc) {
  __shared__ uint32_t s_lit[kWaves], s_on[kWaves];
  const uint32_t o = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool on = o < fs_ops(in), lit = on && fs_literal(in, o);
  uint64_t excl;
  const uint64_t all = fs_wg_scan(lit ? in.op_len[o] : 0ull, excl);
  const uint32_t wl = (uint32_t)__popcll(__ballot(lit)), wo = (uint32_t)__popcll(__ballot(on));
  if (lane == 0) s_lit[wave] = wl, s_on[wave] = wo;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t l = 0, n = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) l += s_lit[w], n += s_on[w];
    gsum[blockIdx.x] = all;  // one writer: the grid is family_store_groups(max_ops) workgroups
    if (l) atomicAdd(fs_sc(sc, kScLitOps), (u64a)l);
    if (n - l) atomicAdd(fs_sc(sc, kScCopyOps), (u64a)(n - l));
  }
}

__global__ void __launch_bounds__(kTB) k_fs_literal(FamilyStoreOps in, const uint64_t* __restrict__ gsum,
                                                    uint64_t* __restrict__ store_off) {
  const uint32_t o = blockIdx.x * kTB + threadIdx.x;
  const bool lit = o < fs_ops(in) && fs_literal(in, o);
  uint64_t excl;
  fs_wg_scan(lit ? in.op_len[o] : 0ull, excl);
  if (lit) store_off[o] = gsum[blockIdx.x] + excl;
}

__global__ void __launch_bounds__(kTB) k_fs_copy(FamilyStoreOps in, const uint32_t* __restrict__ chunk_op, uint32_t m,
                                                 uint64_t* store_off, u64a* sc) {
  __shared__ u64a s_sum[2];
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t o = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  const uint32_t ops = fs_ops(in);
  bool unc = false;
  uint64_t len = 0;
  if (o < ops && !fs_literal(in, o)) {
    len = in.op_len[o];
    uint64_t at = kNone;
    const uint32_t s = in.op_src_chunk[o];
    if (s < m) {
      const uint32_t l = chunk_op[s];
      if (l < ops && fs_literal(in, l) && in.op_row[l] == in.op_src_row[o]) {
        const uint64_t so = in.op_src_off[o], lo = in.op_dst_off[l], ll = in.op_len[l];
        // l is a literal: its offset is from k_fs_literal, never from this launch
        if (so >= lo && so - lo <= ll && len <= ll - (so - lo)) at = store_off[l] + (so - lo);
      }
    }
    // a covered op whose offset comes out as 2^64 - 1 reads as uncovered to the mover; it is counted so here
    unc = at == kNone;
    store_off[o] = at;
  }
  const uint32_t wu = (uint32_t)__popcll(__ballot(unc));
  const uint64_t wb = fb_wave_sum(unc ? len : 0ull);
  if (lane == 0 && wu) {
    atomicAdd(&s_sum[0], (u64a)wu);
    if (wb) atomicAdd(&s_sum[1], (u64a)wb);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_sum[threadIdx.x]) atomicAdd(fs_sc(sc, kScUncOps + threadIdx.x), s_sum[threadIdx.x]);
}

// ops, literal_ops, copy_ops, uncovered_ops, store_bytes, uncovered_bytes
__global__ void k_fs_counts(const u64a* sc, const uint64_t* __restrict__ tot, u64a* __restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint64_t lit = fs_fold(sc, kScLitOps), cp = fs_fold(sc, kScCopyOps);
  counts[0] = lit + cp, counts[1] = lit, counts[2] = cp;
  counts[3] = fs_fold(sc, kScUncOps), counts[4] = tot[0], counts[5] = fs_fold(sc, kScUncBytes);
}

// ---- the mover -----------------------------------------------------------------------

__device__ __forceinline__ uint64_t fs_tiles(uint64_t dst, uint64_t len) {
  return len ? ((dst & 15) + len + kTile - 1) / kTile : 0ull;
}

__global__ void __launch_bounds__(kTB) k_fs_clip(FamilyStoreOps in, const uint64_t* __restrict__ store_off,
                                                 FamilyStoreRows rows, uint64_t blob_bytes, uint64_t store_bytes,
                                                 bool restore, uint64_t* __restrict__ start,
                                                 uint64_t* __restrict__ dst, uint64_t* __restrict__ src,
                                                 uint64_t* __restrict__ len, uint64_t* __restrict__ gsum, u64a* sc) {
  __shared__ u64a s_sum[3];
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  // the barrier of fs_wg_scan below orders this before the adds
  const uint32_t o = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  uint64_t tiles = 0, moved = 0;
  bool bad = false;
  if (o < fs_ops(in)) {
    const uint64_t so = store_off[o];
    if (so != kNone && (restore || fs_literal(in, o))) {
      const uint32_t row = in.op_row[o];
      const uint64_t d = in.op_dst_off[o], l = in.op_len[o];
      bad = row >= rows.n || d + l < d || so > store_bytes || l > store_bytes - so;
      if (!bad) {
        const uint64_t rl = rows.row_len[row];
        if (rl) {  // the row is in the blob
          const uint64_t at = rows.row_at[row], base = rows.row_base ? rows.row_base[row] : 0ull;
          bad = at > blob_bytes || rl > blob_bytes - at || base + rl < base;
          if (!bad) {
            const uint64_t lo = d > base ? d : base, hi = d + l < base + rl ? d + l : base + rl;
            if (hi > lo) {
              const uint64_t b = at + (lo - base), s = so + (lo - d);
              moved = hi - lo;
              dst[o] = restore ? b : s;
              src[o] = restore ? s : b;
              len[o] = moved;
              tiles = fs_tiles(restore ? b : s, moved);
            }
          }
        }
      }
    }
  }
  if (o < in.max_ops) start[o] = tiles;
  uint64_t excl;
  const uint64_t all = fs_wg_scan(tiles, excl);
  const uint32_t wm = (uint32_t)__popcll(__ballot(moved != 0)), wbad = (uint32_t)__popcll(__ballot(bad));
  const uint64_t wb = fb_wave_sum(moved);
  if (lane == 0) {
    if (wm) atomicAdd(&s_sum[0], (u64a)wm), atomicAdd(&s_sum[1], (u64a)wb);
    if (wbad) atomicAdd(&s_sum[2], (u64a)wbad);
  }
  __syncthreads();
  if (threadIdx.x == 0) gsum[blockIdx.x] = all;
  if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(fs_sc(sc, kScMoved + threadIdx.x), s_sum[threadIdx.x]);
}

__global__ void __launch_bounds__(kTB) k_fs_starts(uint32_t max_ops, const uint64_t* __restrict__ gsum,
                                                   uint64_t* __restrict__ start) {
  const uint32_t o = blockIdx.x * kTB + threadIdx.x;
  uint64_t excl;
  fs_wg_scan(o < max_ops ? start[o] : 0ull, excl);
  if (o < max_ops) start[o] = gsum[blockIdx.x] + excl;
}

// the largest o' in [o, n) with start[o'] <= t, given start[o] <= t: doubling steps, then halving
__device__ __forceinline__ uint32_t fs_find(const uint64_t* __restrict__ start, uint32_t n, uint32_t o, uint64_t t) {
  uint64_t lo = o, hi = (uint64_t)o + 1, step = 1;
  while (hi < n && start[hi] <= t) {
    lo = hi;
    hi += step;
    step <<= 1;
  }
  if (hi > n) hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (start[mid] <= t) lo = mid; else hi = mid;
  }
  return (uint32_t)lo;
}

// The 16-byte unit at destination offset u (a multiple of 16) of an op whose
// `len` bytes go to dbuf + d from sbuf + s. Both buffers are 16-byte aligned.
__device__ __forceinline__ void fs_unit(uint8_t* __restrict__ dbuf, const uint8_t* __restrict__ sbuf, uint64_t d,
                                        uint64_t s, uint64_t len, uint64_t u) {
  if (u + 16 <= d || u >= d + len) return;
  const uint32_t vlo = u < d ? (uint32_t)(d - u) : 0u;                   // the unit's destination bytes are
  const uint32_t vhi = d + len - u < 16 ? (uint32_t)(d + len - u) : 16u;  // [vlo, vhi) of its 16
  // the source of the unit's byte 0 (before the source's first byte when vlo != 0: never read there)
  // as an offset in sbuf, itself 16-byte aligned; modulo 2^64, and then al[0] is not read
  const uint64_t sp = s + (u - d);
  const uint4* al = reinterpret_cast<const uint4*>(sbuf + (sp & ~15ull));
  const uint32_t mis = (uint32_t)(sp & 15);
  // byte i of the unit lies in al[0] when i + mis < 16, else in al[1]
  uint4 a = make_uint4(0, 0, 0, 0), b = a;
  if (vlo + mis < 16) a = al[0];
  if (vhi - 1 + mis >= 16) b = al[1];
  uint4 out = a;
  if (mis) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t q = mis >> 2, sh = mis & 3;
    uint32_t t[5];
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) t[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
    out.x = __builtin_amdgcn_alignbyte(t[1], t[0], sh);
    out.y = __builtin_amdgcn_alignbyte(t[2], t[1], sh);
    out.z = __builtin_amdgcn_alignbyte(t[3], t[2], sh);
    out.w = __builtin_amdgcn_alignbyte(t[4], t[3], sh);
  }
  if (vlo == 0 && vhi == 16) {
    *reinterpret_cast<uint4*>(dbuf + u) = out;
  } else {
    const uint32_t w[4] = {out.x, out.y, out.z, out.w};
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
      if (i >= vlo && i < vhi) dbuf[u + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

__global__ void __launch_bounds__(kTB) k_fs_move(const uint64_t* __restrict__ start, const uint64_t* __restrict__ dst,
                                                 const uint64_t* __restrict__ src, const uint64_t* __restrict__ len,
                                                 uint32_t max_ops, const uint64_t* __restrict__ tot,
                                                 uint8_t* __restrict__ dbuf, const uint8_t* __restrict__ sbuf) {
  const uint64_t total = tot[0];
  const uint64_t per = (total + gridDim.x - 1) / gridDim.x;
  const uint64_t t0 = blockIdx.x * per, t1 = t0 + per < total ? t0 + per : total;
  uint32_t o = 0;
  uint64_t first = 0, end = 0, d = 0, s = 0, l = 0;  // the op's tiles are [first, end)
  for (uint64_t t = t0; t < t1; ++t) {
    if (t >= end) {
      o = fs_find(start, max_ops, o, t);
      first = start[o], d = dst[o], s = src[o], l = len[o];
      end = first + fs_tiles(d, l);
      if (t >= end) return;  // never: every tile below the total belongs to an op
    }
    const uint64_t u0 = (d & ~15ull) + (t - first) * kTile + 16ull * threadIdx.x;
#pragma unroll
    for (uint32_t j = 0; j < kFamilyStorePer; ++j) fs_unit(dbuf, sbuf, d, s, l, u0 + 16ull * kTB * j);
  }
}

// ops_moved, bytes_moved, bad_ops, tiles
__global__ void k_fs_moved(const u64a* sc, const uint64_t* __restrict__ tot, u64a* __restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  counts[0] = fs_fold(sc, kScMoved), counts[1] = fs_fold(sc, kScMovedBytes);
  counts[2] = fs_fold(sc, kScBad), counts[3] = tot[0];
}

}  // namespace

hipError_t family_store_offsets(uint8_t* ws, const FamilyStoreOps& ops, const uint32_t* chunk_op, uint32_t m,
                                uint64_t* store_off, unsigned long long* counts, hipStream_t st) {
  const FamilyStoreLayout l = family_store_layout(ops.max_ops);
  u64a* sc = index_at<u64a>(ws, l.sc);
  uint64_t* tot = index_at<uint64_t>(ws, l.tot);
  uint64_t* gsum = index_at<uint64_t>(ws, l.gsum);
  if (!store_off) store_off = index_at<uint64_t>(ws, l.start);  // the copies read the literals' offsets
  hipError_t e;
  if ((e = hipMemsetAsync(ws + l.sc, 0, l.gsum - l.sc, st))) return e;  // sc, tot
  if (ops.max_ops) {
    const uint32_t groups = (uint32_t)family_store_groups(ops.max_ops);
    const dim3 grid(groups), block(kTB);
    hipLaunchKernelGGL(k_fs_sum, grid, block, 0, st, ops, gsum, sc);
    hipLaunchKernelGGL(k_fs_scan, dim3(1), dim3(1024), 0, st, gsum, groups, tot);
    hipLaunchKernelGGL(k_fs_literal, grid, block, 0, st, ops, (const uint64_t*)gsum, store_off);
    hipLaunchKernelGGL(k_fs_copy, grid, block, 0, st, ops, chunk_op, m, store_off, sc);
    if ((e = hipGetLastError())) return e;
  }
  if (counts) {
    hipLaunchKernelGGL(k_fs_counts, dim3(1), dim3(64), 0, st, (const u64a*)sc, (const uint64_t*)tot, counts);
    if ((e = hipGetLastError())) return e;
  }
  return hipSuccess;
}

hipError_t family_store_move(uint8_t* ws, const FamilyStoreOps& ops, const uint64_t* store_off,
                             const FamilyStoreRows& rows, uint8_t* blob, uint64_t blob_bytes, uint8_t* store,
                             uint64_t store_bytes, bool restore, unsigned long long* counts, hipStream_t st) {
  const FamilyStoreLayout l = family_store_layout(ops.max_ops);
  u64a* sc = index_at<u64a>(ws, l.sc);
  uint64_t* tot = index_at<uint64_t>(ws, l.tot);
  uint64_t* gsum = index_at<uint64_t>(ws, l.gsum);
  uint64_t* start = index_at<uint64_t>(ws, l.start);
  uint64_t* dst = index_at<uint64_t>(ws, l.dst);
  uint64_t* src = index_at<uint64_t>(ws, l.src);
  uint64_t* len = index_at<uint64_t>(ws, l.len);
  hipError_t e;
  if ((e = hipMemsetAsync(ws + l.sc, 0, l.gsum - l.sc, st))) return e;  // sc, tot
  if (ops.max_ops) {
    const uint32_t groups = (uint32_t)family_store_groups(ops.max_ops);
    const dim3 grid(groups), block(kTB);
    hipLaunchKernelGGL(k_fs_clip, grid, block, 0, st, ops, store_off, rows, blob_bytes, store_bytes, restore, start,
                       dst, src, len, gsum, sc);
    hipLaunchKernelGGL(k_fs_scan, dim3(1), dim3(1024), 0, st, gsum, groups, tot);
    hipLaunchKernelGGL(k_fs_starts, grid, block, 0, st, ops.max_ops, (const uint64_t*)gsum, start);
    hipLaunchKernelGGL(k_fs_move, dim3(kFamilyStoreGrid), block, 0, st, (const uint64_t*)start, (const uint64_t*)dst,
                       (const uint64_t*)src, (const uint64_t*)len, ops.max_ops, (const uint64_t*)tot,
                       restore ? blob : store, (const uint8_t*)(restore ? store : blob));
    if ((e = hipGetLastError())) return e;
  }
  if (counts) {
    hipLaunchKernelGGL(k_fs_moved, dim3(1), dim3(64), 0, st, (const u64a*)sc, (const uint64_t*)tot, counts);
    if ((e = hipGetLastError())) return e;
  }
  return hipSuccess;
}

}  // namespace sdcas
