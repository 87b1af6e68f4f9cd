// family_forget.hip — a family store that forgets rows (include/sdcas.h has the
// definition; family_forget.h the workspace). Two calls around the recipes and
// the layout, which run unchanged over what the first one leaves.
// keep, the chunk arrays of the rows that stay:
//   k_fg_rows          per row: kept or not; the kept of every workgroup counted;
//                      a kept row that takes part into its label's word (atomicMin)
//   k_fg_chunks        per chunk: survives or not; the survivors of every workgroup
//                      counted; a survivor into its class number's word (atomicMin)
//   k_fg_scan          the workgroup counts become offsets (wg_scan.h), once for
//                      the rows and once for the chunks
//   k_fg_row_scatter   a kept row's new number: its workgroup's offset plus its
//                      rank there; row_new, row_from
//   k_fg_row_family    a kept row's label: the new number of its label's lowest row
//   k_fg_chunk_scatter a survivor's new position; chunk_from, chunk_file through
//                      row_new, offsets and lengths copied
//   k_fg_chunk_rep     a survivor's rep: the new position of its class's lowest
//   k_fg_keep_counts   the counts
// moves, the literal chunks of the new recipes found in the old store:
//   k_fg_flag          per new chunk: a literal or not, old_at, and whether it
//                      continues the chunk below, from the two chunks alone (the
//                      lower one's old_at is computed again, not awaited); the
//                      heads of every workgroup counted
//   k_fg_scan          the heads become offsets, their sum the moves
//   k_fg_emit          a head's move: where it lands and where it comes from
//   k_fg_close         where a run ends: the move's length is the end's old_at
//                      plus length minus the head's (old_at inside a run is
//                      contiguous by the continuation rule, modulo 2^64)
//   k_fg_moves_counts  the counts
// The bytes then go through family_store.hip's mover; there is no copy kernel here.
//
// The lanes of a wave that carry its first live lane's label or class follow
// that lane, whose position is their lowest: one label on every row, or one
// class in every chunk, sends one atomicMin per wave and not sixty-four.
//
// Visibility as in family_recipes.hip: table words and the counters are touched
// only by agent-scope atomics and relaxed agent-scope atomic loads; every phase
// is a launch of its own; arrays that one launch writes with plain stores
// (row_new, chunk_new, the counts per workgroup, at, flag, start) are read by
// later launches with plain loads. No thread waits for another. A minimum over
// positions, ranks and sums modulo 2^64: results do not depend on scheduling.
#include <hip/hip_runtime.h>

#include "chunk_index.h"
#include "family_bytes_device.h"
#include "family_forget.h"
#include "wg_scan.h"

namespace sdcas {

namespace {

constexpr uint32_t kTB = kFamilyForgetTB;
constexpr uint32_t kWaves = kTB / 64;
constexpr uint32_t kNone = kFbNone;
constexpr uint64_t kNoAt = ~0ull;  // SDCAS_STORE_NONE
enum { kScRows, kScChunks, kScBytesKept, kScBytesRemoved };
enum { kScLit, kScLost, kScLostBytes, kScMoved, kScLongest };

__device__ __forceinline__ u64a* fg_sc(u64a* sc, uint32_t k) {
  return &sc[(blockIdx.x & (kFamilyForgetScCopies - 1)) * 16 + k];
}
__device__ __forceinline__ uint64_t fg_fold(const u64a* sc, uint32_t k, bool max = false) {
  uint64_t v = 0;
  for (uint32_t r = 0; r < kFamilyForgetScCopies; ++r) {
    const uint64_t x = fb_load(&sc[r * 16 + k]);
    v = max ? (x > v ? x : v) : v + x;
  }
  return v;
}

// Called ONCE by every thread of a workgroup of kTB: the flagged threads below
// this one; all <- the flagged threads of the workgroup.
__device__ __forceinline__ uint32_t fg_rank(bool f, uint32_t& all) {
  __shared__ uint32_t s_w[kWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(f);
  if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t before = (uint32_t)__popcll(b & ((1ull << lane) - 1));
  all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    if (w < wave) before += s_w[w];
    all += s_w[w];
  }
  return before;
}

// atomicMin(&tab[key], pos) for the lanes that are `on`; the lanes that carry the first live lane's key follow it
__device__ __forceinline__ void fg_min(uint32_t* tab, bool on, uint32_t key, uint32_t pos) {
  const unsigned long long live = __ballot(on);
  const uint32_t lead = live ? fb_first(live) : 0u, lane = threadIdx.x & 63;
  const uint32_t lkey = __shfl(key, lead);
  if (on && (lane == lead || key != lkey)) atomicMin(&tab[key], pos);
}

// ---- keep ----------------------------------------------------------------------------

__device__ __forceinline__ bool fg_kept(const FamilyKeepIn& in, uint32_t i) { return i < in.n && in.keep[i] != 0; }
// the chunk survives; r <- its class number, a number below m
__device__ __forceinline__ bool fg_survives(const FamilyKeepIn& in, uint32_t c, uint32_t& r) {
  if (c >= in.m) return false;
  const int64_t v = in.rep[c];
  r = v >= 0 && v <= (int64_t)c ? (uint32_t)v : c;
  return fg_kept(in, in.chunk_file[c]);
}

__global__ void __launch_bounds__(kTB) k_fg_rows(FamilyKeepIn in, uint32_t* ltab, uint32_t* __restrict__ rcnt, u64a* sc) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  const bool kept = fg_kept(in, i);
  uint32_t label = 0;
  const bool on = kept && fb_label(in.family, in.n, i, label);
  fg_min(ltab, on, label, i);
  uint32_t all;
  fg_rank(kept, all);
  if (threadIdx.x == 0) {
    rcnt[blockIdx.x] = all;  // one writer: the grid is family_forget_groups(n) workgroups
    if (all) atomicAdd(fg_sc(sc, kScRows), (u64a)all);
  }
}

__global__ void __launch_bounds__(kTB) k_fg_chunks(FamilyKeepIn in, uint32_t* rtab, uint32_t* __restrict__ ccnt,
                                                   u64a* sc) {
  __shared__ u64a s_sum[2];
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  // the barrier of fg_rank below orders this before the adds
  const uint32_t c = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  uint32_t r = 0;
  const bool sv = fg_survives(in, c, r);
  fg_min(rtab, sv, r, c);
  const uint64_t len = c < in.m ? in.chunk_len[c] : 0ull;
  uint32_t all;
  fg_rank(sv, all);
  const uint64_t kb = fb_wave_sum(sv ? len : 0ull), rb = fb_wave_sum(sv ? 0ull : len);
  if (lane == 0) {
    if (kb) atomicAdd(&s_sum[0], (u64a)kb);
    if (rb) atomicAdd(&s_sum[1], (u64a)rb);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ccnt[blockIdx.x] = all;
    if (all) atomicAdd(fg_sc(sc, kScChunks), (u64a)all);
  }
  if (threadIdx.x < 2 && s_sum[threadIdx.x]) atomicAdd(fg_sc(sc, kScBytesKept + threadIdx.x), s_sum[threadIdx.x]);
}

__global__ void __launch_bounds__(1024) k_fg_scan(uint32_t* __restrict__ cnt, uint32_t nb, uint32_t* __restrict__ total) {
  wg_scan_exclusive_1024(cnt, nb, total);
}

__global__ void __launch_bounds__(kTB) k_fg_row_scatter(FamilyKeepIn in, const uint32_t* __restrict__ rcnt,
                                                        uint32_t* __restrict__ row_new, FamilyKeepOut out) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  const bool kept = fg_kept(in, i);
  uint32_t all;
  const uint32_t j = rcnt[blockIdx.x] + fg_rank(kept, all);
  if (i >= in.n) return;
  const uint32_t to = kept && j < in.n ? j : kNone;  // j < n: always, a kept row below i per number
  row_new[i] = to;
  if (out.row_new) out.row_new[i] = to;
  if (to != kNone && out.row_from) out.row_from[to] = i;
}

__global__ void __launch_bounds__(kTB) k_fg_row_family(FamilyKeepIn in, const uint32_t* ltab,
                                                       const uint32_t* __restrict__ row_new,
                                                       int64_t* __restrict__ out_family) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  if (i >= in.n) return;
  const uint32_t j = row_new[i];
  if (j >= in.n) return;
  int64_t v = -1;
  uint32_t label;
  if (fb_label(in.family, in.n, i, label)) {
    const uint32_t low = fb_load(&ltab[label]);  // at most i: this row went in
    if (low < in.n && row_new[low] < in.n) v = (int64_t)row_new[low];
  }
  out_family[j] = v;
}

__global__ void __launch_bounds__(kTB) k_fg_chunk_scatter(FamilyKeepIn in, const uint32_t* __restrict__ ccnt,
                                                          const uint32_t* __restrict__ row_new,
                                                          uint32_t* __restrict__ chunk_new, FamilyKeepOut out) {
  const uint32_t c = blockIdx.x * kTB + threadIdx.x;
  uint32_t r, all;
  const bool sv = fg_survives(in, c, r);
  const uint32_t j = ccnt[blockIdx.x] + fg_rank(sv, all);
  if (c >= in.m) return;
  const uint32_t to = sv && j < in.m ? j : kNone;  // j < m: always
  chunk_new[c] = to;
  if (to == kNone) return;
  if (out.chunk_from) out.chunk_from[to] = c;
  if (out.chunk_file) out.chunk_file[to] = row_new[in.chunk_file[c]];  // a kept row: it has a number
  if (out.chunk_off) out.chunk_off[to] = in.chunk_off[c];
  if (out.chunk_len) out.chunk_len[to] = in.chunk_len[c];
}

__global__ void __launch_bounds__(kTB) k_fg_chunk_rep(FamilyKeepIn in, const uint32_t* rtab,
                                                      const uint32_t* __restrict__ chunk_new,
                                                      int64_t* __restrict__ out_rep) {
  const uint32_t c = blockIdx.x * kTB + threadIdx.x;
  if (c >= in.m) return;
  const uint32_t to = chunk_new[c];
  if (to >= in.m) return;
  uint32_t r;
  fg_survives(in, c, r);
  const uint32_t low = fb_load(&rtab[r]);  // at most c: this chunk went in
  out_rep[to] = low < in.m && chunk_new[low] < in.m ? (int64_t)chunk_new[low] : (int64_t)to;  // always the first
}

// rows_kept, rows_removed, chunks_kept, chunks_removed, bytes_kept, bytes_removed
__global__ void k_fg_keep_counts(const u64a* sc, uint32_t m, uint32_t n, u64a* __restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint64_t rows = fg_fold(sc, kScRows), chunks = fg_fold(sc, kScChunks);
  counts[0] = rows, counts[1] = n - rows, counts[2] = chunks, counts[3] = m - chunks;
  counts[4] = fg_fold(sc, kScBytesKept), counts[5] = fg_fold(sc, kScBytesRemoved);
}

// ---- moves ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t fg_least(const uint64_t* d, uint32_t cap) {
  if (!cap) return 0;
  const uint64_t v = d[0];
  return v < cap ? (uint32_t)v : cap;
}

// new chunk c (below the new chunks): a literal chunk or not; o <- its new op
__device__ __forceinline__ bool fg_literal(const FamilyMovesIn& in, uint32_t nops, uint32_t c, uint32_t& o) {
  o = in.nchunk_op[c];
  return o < nops && in.nop_chunk[o] == in.nop_src_chunk[o];
}
// where new chunk c's bytes lie in the old store, or none
__device__ __forceinline__ uint64_t fg_old_at(const FamilyMovesIn& in, uint32_t ops, uint32_t c) {
  const uint32_t oc = in.nchunk_from[c];
  if (oc >= in.m) return kNoAt;
  const uint32_t o = in.chunk_op[oc];
  if (o >= ops) return kNoAt;  // 0xFFFFFFFF too
  const uint64_t so = in.op_store_off[o], off = in.chunk_off[oc], d = in.op_dst_off[o];
  if (so == kNoAt || off < d) return kNoAt;
  return so + (off - d);  // a place that comes out as 2^64 - 1 reads as none
}

__global__ void __launch_bounds__(kTB) k_fg_flag(FamilyMovesIn in, uint64_t* __restrict__ at, uint8_t* __restrict__ flag,
                                                 uint32_t* __restrict__ gcnt, u64a* sc) {
  __shared__ u64a s_sum[3];
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  // the barrier of fg_rank below orders this before the adds
  const uint32_t c = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  const uint32_t chunks = fg_least(in.d_chunks, in.max_chunks);
  const uint32_t ops = fg_least(in.d_ops, in.max_ops), nops = fg_least(in.d_nops, in.max_nops);
  bool lit = false, head = false, cont = false;
  uint64_t a = kNoAt, len = 0;
  if (c < chunks) {
    uint32_t o;
    lit = fg_literal(in, nops, c, o);
    if (lit) {
      a = fg_old_at(in, ops, c);
      len = in.nchunk_len[c];
      if (a != kNoAt) {
        uint32_t op;
        if (c >= 1 && fg_literal(in, nops, c - 1, op) && op == o) {
          const uint64_t ap = fg_old_at(in, ops, c - 1);
          cont = ap != kNoAt && a == ap + in.nchunk_len[c - 1];
        }
        head = !cont;
      }
    }
  }
  if (c < in.max_chunks) {
    at[c] = a;
    flag[c] = head ? 1 : cont ? 2 : 0;
  }
  const bool lost = lit && a == kNoAt;
  uint32_t heads;
  fg_rank(head, heads);
  const uint32_t wl = (uint32_t)__popcll(__ballot(lit)), wlost = (uint32_t)__popcll(__ballot(lost));
  const uint64_t wb = fb_wave_sum(lost ? len : 0ull);
  if (lane == 0) {
    if (wl) atomicAdd(&s_sum[0], (u64a)wl);
    if (wlost) atomicAdd(&s_sum[1], (u64a)wlost);
    if (wb) atomicAdd(&s_sum[2], (u64a)wb);
  }
  __syncthreads();
  if (threadIdx.x == 0) gcnt[blockIdx.x] = heads;  // one writer: the grid is family_forget_groups(max_chunks)
  if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(fg_sc(sc, kScLit + threadIdx.x), s_sum[threadIdx.x]);
}

__global__ void __launch_bounds__(kTB) k_fg_emit(FamilyMovesIn in, const uint64_t* __restrict__ at,
                                                 const uint8_t* __restrict__ flag, const uint32_t* __restrict__ gcnt,
                                                 uint64_t* __restrict__ start, uint64_t* __restrict__ move_dst,
                                                 uint64_t* __restrict__ move_src) {
  const uint32_t c = blockIdx.x * kTB + threadIdx.x;
  const bool head = c < in.max_chunks && flag[c] == 1;
  uint32_t all;
  const uint32_t j = gcnt[blockIdx.x] + fg_rank(head, all);
  if (!head || j >= in.max_chunks) return;  // j < max_chunks: a head per chunk at most
  const uint32_t o = in.nchunk_op[c];       // a literal chunk's op: below the new ops
  const uint64_t a = at[c];
  start[j] = a;
  if (move_dst) move_dst[j] = in.nop_store_off[o] + (in.nchunk_off[c] - in.nop_dst_off[o]);
  if (move_src) move_src[j] = a;
}

__global__ void __launch_bounds__(kTB) k_fg_close(FamilyMovesIn in, const uint64_t* __restrict__ at,
                                                  const uint8_t* __restrict__ flag, const uint32_t* __restrict__ gcnt,
                                                  const uint64_t* __restrict__ start, uint64_t* __restrict__ move_len,
                                                  u64a* sc) {
  __shared__ u64a s_sum[2];
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  // the barrier of fg_rank below orders this before the adds
  const uint32_t c = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  const uint8_t f = c < in.max_chunks ? flag[c] : 0;
  const bool head = f == 1;
  uint32_t all;
  const uint32_t upto = gcnt[blockIdx.x] + fg_rank(head, all) + (head ? 1u : 0u);  // the heads at or before c
  uint64_t len = 0;
  // a chunk of a move follows a head or is one: upto >= 1
  if (f && upto >= 1 && upto <= in.max_chunks && (c + 1 >= in.max_chunks || flag[c + 1] != 2)) {
    len = at[c] + in.nchunk_len[c] - start[upto - 1];
    if (move_len) move_len[upto - 1] = len;
  }
  const uint64_t wb = fb_wave_sum(len), wm = fb_wave_max(len);
  if (lane == 0) {
    if (wb) atomicAdd(&s_sum[0], (u64a)wb);
    if (wm) atomicMax(&s_sum[1], (u64a)wm);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_sum[0]) atomicAdd(fg_sc(sc, kScMoved), s_sum[0]);
  if (threadIdx.x == 1 && s_sum[1]) atomicMax(fg_sc(sc, kScLongest), s_sum[1]);
}

// moves, literal_chunks, moved_bytes, lost_chunks, lost_bytes, longest_move
__global__ void k_fg_moves_counts(const u64a* sc, const uint32_t* __restrict__ tot, u64a* __restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  counts[0] = tot[0], counts[1] = fg_fold(sc, kScLit), counts[2] = fg_fold(sc, kScMoved);
  counts[3] = fg_fold(sc, kScLost), counts[4] = fg_fold(sc, kScLostBytes), counts[5] = fg_fold(sc, kScLongest, true);
}

}  // namespace

hipError_t family_chunks_keep(uint8_t* ws, const FamilyKeepIn& in, const FamilyKeepOut& out,
                              unsigned long long* counts, hipStream_t st) {
  const uint32_t m = in.m, n = in.n;
  const FamilyKeepLayout l = family_keep_layout(m, n);
  uint32_t* rtab = index_at<uint32_t>(ws, l.rtab);
  uint32_t* ltab = index_at<uint32_t>(ws, l.ltab);
  u64a* sc = index_at<u64a>(ws, l.sc);
  uint32_t* tot = index_at<uint32_t>(ws, l.tot);
  uint32_t* row_new = index_at<uint32_t>(ws, l.row_new);
  uint32_t* chunk_new = index_at<uint32_t>(ws, l.chunk_new);
  uint32_t* rcnt = index_at<uint32_t>(ws, l.rcnt);
  uint32_t* ccnt = index_at<uint32_t>(ws, l.ccnt);
  hipError_t e;
  if (l.sc != l.rtab && (e = hipMemsetAsync(ws + l.rtab, 0xFF, l.sc - l.rtab, st))) return e;  // rtab, ltab
  if ((e = hipMemsetAsync(ws + l.sc, 0, l.row_new - l.sc, st))) return e;     // sc, tot
  const dim3 block(kTB);
  if (n) {
    const uint32_t groups = (uint32_t)family_forget_groups(n);
    const dim3 rows(groups);
    hipLaunchKernelGGL(k_fg_rows, rows, block, 0, st, in, ltab, rcnt, sc);
    hipLaunchKernelGGL(k_fg_scan, dim3(1), dim3(1024), 0, st, rcnt, groups, tot);
    hipLaunchKernelGGL(k_fg_row_scatter, rows, block, 0, st, in, (const uint32_t*)rcnt, row_new, out);
    if (out.family)
      hipLaunchKernelGGL(k_fg_row_family, rows, block, 0, st, in, (const uint32_t*)ltab, (const uint32_t*)row_new,
                         out.family);
    if ((e = hipGetLastError())) return e;
  }
  if (m) {  // without rows no chunk survives: all of them are counted as removed
    const uint32_t groups = (uint32_t)family_forget_groups(m);
    const dim3 chunks(groups);
    hipLaunchKernelGGL(k_fg_chunks, chunks, block, 0, st, in, rtab, ccnt, sc);
    hipLaunchKernelGGL(k_fg_scan, dim3(1), dim3(1024), 0, st, ccnt, groups, tot + 1);
    hipLaunchKernelGGL(k_fg_chunk_scatter, chunks, block, 0, st, in, (const uint32_t*)ccnt, (const uint32_t*)row_new,
                       chunk_new, out);
    if (out.rep)
      hipLaunchKernelGGL(k_fg_chunk_rep, chunks, block, 0, st, in, (const uint32_t*)rtab, (const uint32_t*)chunk_new,
                         out.rep);
    if ((e = hipGetLastError())) return e;
  }
  if (counts) {
    hipLaunchKernelGGL(k_fg_keep_counts, dim3(1), dim3(64), 0, st, (const u64a*)sc, m, n, counts);
    if ((e = hipGetLastError())) return e;
  }
  return hipSuccess;
}

hipError_t family_store_moves(uint8_t* ws, const FamilyMovesIn& in, uint64_t* move_dst, uint64_t* move_src,
                              uint64_t* move_len, unsigned long long* counts, hipStream_t st) {
  const FamilyMovesLayout l = family_moves_layout(in.max_chunks);
  u64a* sc = index_at<u64a>(ws, l.sc);
  uint32_t* tot = index_at<uint32_t>(ws, l.tot);
  uint64_t* at = index_at<uint64_t>(ws, l.at);
  uint64_t* start = index_at<uint64_t>(ws, l.start);
  uint8_t* flag = index_at<uint8_t>(ws, l.flag);
  uint32_t* gcnt = index_at<uint32_t>(ws, l.gcnt);
  hipError_t e;
  if ((e = hipMemsetAsync(ws + l.sc, 0, l.at - l.sc, st))) return e;  // sc, tot
  if (in.max_chunks) {
    const uint32_t groups = (uint32_t)family_forget_groups(in.max_chunks);
    const dim3 grid(groups), block(kTB);
    hipLaunchKernelGGL(k_fg_flag, grid, block, 0, st, in, at, flag, gcnt, sc);
    hipLaunchKernelGGL(k_fg_scan, dim3(1), dim3(1024), 0, st, gcnt, groups, tot);
    hipLaunchKernelGGL(k_fg_emit, grid, block, 0, st, in, (const uint64_t*)at, (const uint8_t*)flag,
                       (const uint32_t*)gcnt, start, move_dst, move_src);
    hipLaunchKernelGGL(k_fg_close, grid, block, 0, st, in, (const uint64_t*)at, (const uint8_t*)flag,
                       (const uint32_t*)gcnt, (const uint64_t*)start, move_len, sc);
    if ((e = hipGetLastError())) return e;
  }
  if (counts) {
    hipLaunchKernelGGL(k_fg_moves_counts, dim3(1), dim3(64), 0, st, (const u64a*)sc, (const uint32_t*)tot, counts);
    if ((e = hipGetLastError())) return e;
  }
  return hipSuccess;
}

}  // namespace sdcas
