// family_recipes.hip — the family recipes: per row the byte ranges (ops) that
// rebuild it from what its family stores (include/sdcas.h has the definition;
// family_recipes.h the workspace). The classes and their first occurrences are
// family_bytes.hip's, by the same table (family_bytes_device.h); what follows is
// a run-head flag per chunk, a scan of the heads and an ordered compaction.
//   k_fr_insert   one chunk per thread into the class table; remembers its slot
//   k_fr_source   f(c) through the table; whether c continues c - 1, from c and
//                 c - 1 alone (c - 1's source is looked up again, not awaited);
//                 the heads of every workgroup counted
//   k_fr_scan     the workgroup counts become offsets (wg_scan.h), their sum
//                 the number of ops
//   k_fr_emit     a head's op is its workgroup's offset plus its rank there; it
//                 writes the op's fields but the length. Every chunk learns its
//                 op: the heads at or before it, minus one
//   k_fr_close    where a run ends: the op's length is the end's offset plus
//                 length minus the head's offset (offsets inside a run are
//                 contiguous by the continuation rule, modulo 2^64), one store
//                 per op and no add per chunk. The op into its row's count and
//                 lowest op, and into the counts
//   k_fr_rows     the per-row outputs; the rows that take part
//   k_fr_totals   the counts
// One file with very many ops: the run ends of a wave that share the first
// one's row add up in the wave, and the waves of a workgroup that share wave
// 0's row once more in LDS, as in k_fb_classify: one add per workgroup. Ops
// ascend with the chunk position, so the first of them is the lowest.
//
// The counters are 64 copies of a line, a workgroup adding to the copy of its
// number, folded by k_fr_totals: one line for all was the call's largest part.
//
// Visibility as in family_bytes.hip: table words, per-row words and the
// counters are touched only by agent-scope atomics and relaxed agent-scope
// atomic loads; every phase is a launch of its own; arrays that one launch
// writes with plain stores (slot, first, head, gcnt, op_start) are read by
// later launches with plain loads. No thread waits for another.
#include <hip/hip_runtime.h>

#include "chunk_index.h"
#include "family_bytes_device.h"
#include "family_recipes.h"
#include "wg_scan.h"

namespace sdcas {

namespace {

constexpr uint32_t kTB = kFamilyBytesTB;
constexpr uint32_t kWaves = kTB / 64;
constexpr uint32_t kNone = kFbNone;
enum { kRcFiles, kRcChunks, kRcOps, kRcLitOps, kRcCopyOps, kRcLitBytes, kRcCopyBytes, kRcLongest, kRcWords };
static_assert(kRcWords == kFamilyRecipesCounts, "sdcas_family_recipes_counts' order");

// the workgroup's copy of counter k
__device__ __forceinline__ u64a* fr_sc(u64a* sc, uint32_t k) {
  return &sc[(blockIdx.x & (kFamilyRecipesScCopies - 1)) * 16 + k];
}

__global__ void __launch_bounds__(kTB) k_fr_insert(FamilyBytesIn in, uint32_t* table, uint32_t mask,
                                                   uint32_t* __restrict__ slot) {
  fb_insert(in, table, mask, slot);
}

// f(c) of a chunk whose slot is s, when it takes part (always below m then)
__device__ __forceinline__ bool fr_first(const uint32_t* table, uint32_t mask, uint32_t m, uint32_t s, uint32_t& f) {
  if (s > mask) return false;  // kNone: the chunk takes no part
  f = fb_load(&table[s]);
  return f < m;  // always
}

__global__ void __launch_bounds__(kTB) k_fr_source(FamilyRecipesIn in, const uint32_t* table, uint32_t mask,
                                                   const uint32_t* __restrict__ slot, uint32_t* __restrict__ first,
                                                   uint8_t* __restrict__ head, uint32_t* __restrict__ gcnt, u64a* sc) {
  __shared__ uint32_t s_heads[kWaves], s_on[kWaves];
  const uint32_t c = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t m = in.fb.m;
  bool on = false, hd = false;
  uint32_t f = kNone;
  if (c < m) {
    on = fr_first(table, mask, m, slot[c], f);
    if (on) {
      hd = true;
      uint32_t fp;
      if (c >= 1 && fr_first(table, mask, m, slot[c - 1], fp)) {
        const uint64_t lp = in.fb.chunk_len[c - 1];
        hd = !(in.fb.chunk_file[c - 1] == in.fb.chunk_file[c] && (f == c) == (fp == c - 1) &&
               in.chunk_off[c] == in.chunk_off[c - 1] + lp && in.fb.chunk_file[f] == in.fb.chunk_file[fp] &&
               in.chunk_off[f] == in.chunk_off[fp] + lp);
      }
    }
    first[c] = on ? f : kNone;
    head[c] = hd ? 1 : 0;
  }
  const uint32_t wh = (uint32_t)__popcll(__ballot(hd)), wo = (uint32_t)__popcll(__ballot(on));
  if (lane == 0) s_heads[wave] = wh, s_on[wave] = wo;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t h = 0, o = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) h += s_heads[w], o += s_on[w];
    gcnt[blockIdx.x] = h;  // one writer: the grid is family_recipes_groups(m) workgroups
    if (o) atomicAdd(fr_sc(sc, kRcChunks), (u64a)o);
  }
}

// one workgroup: gcnt[b] <- the heads before workgroup b; *total <- the ops
__global__ void __launch_bounds__(1024) k_fr_scan(uint32_t* __restrict__ gcnt, uint32_t nb,
                                                  uint32_t* __restrict__ total) {
  wg_scan_exclusive_1024(gcnt, nb, total);
}

__global__ void __launch_bounds__(kTB) k_fr_emit(FamilyRecipesIn in, const uint32_t* __restrict__ first,
                                                 const uint8_t* __restrict__ head, const uint32_t* __restrict__ gcnt,
                                                 uint32_t* __restrict__ chunk_op, uint64_t* __restrict__ op_start,
                                                 FamilyRecipesOut out) {
  __shared__ uint32_t s_heads[kWaves];
  const uint32_t c = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t m = in.fb.m;
  uint32_t f = kNone;
  bool hd = false;
  if (c < m) f = first[c], hd = head[c] != 0;
  const bool on = f < m;
  const unsigned long long heads = __ballot(hd);
  if (lane == 0) s_heads[wave] = (uint32_t)__popcll(heads);
  __syncthreads();
  uint32_t upto = gcnt[blockIdx.x] + (uint32_t)__popcll(heads & (~0ull >> (63 - lane)));  // the heads at or before c
  for (uint32_t w = 0; w < wave; ++w) upto += s_heads[w];
  // a chunk that takes part follows a head or is one: upto >= 1
  const uint32_t op = on && upto >= 1 && upto <= m ? upto - 1 : kNone;
  if (c < m) {
    chunk_op[c] = op;
    if (out.chunk_op) out.chunk_op[c] = op;
  }
  if (hd && op < m) {  // op < m: a head per chunk at most
    const uint32_t row = in.fb.chunk_file[c], srow = in.fb.chunk_file[f];
    const uint64_t dst = in.chunk_off[c];
    op_start[op] = dst;
    if (out.op_chunk) out.op_chunk[op] = c;
    if (out.op_src_chunk) out.op_src_chunk[op] = f;
    if (out.op_row) out.op_row[op] = row;
    if (out.op_src_row) out.op_src_row[op] = srow;
    if (out.op_dst_off) out.op_dst_off[op] = dst;
    if (out.op_src_off) out.op_src_off[op] = in.chunk_off[f];
  }
}

__global__ void __launch_bounds__(kTB) k_fr_close(FamilyRecipesIn in, const uint32_t* __restrict__ first,
                                                  const uint8_t* __restrict__ head,
                                                  const uint32_t* __restrict__ chunk_op,
                                                  const uint64_t* __restrict__ op_start, uint64_t* __restrict__ op_len,
                                                  uint32_t* row_ops, uint32_t* row_first, u64a* sc) {
  __shared__ u64a s_sum[5];              // literal ops, copy ops, literal bytes, copy bytes, longest op
  __shared__ uint32_t s_row[kWaves];     // per wave: its first run end's row
  __shared__ uint32_t s_cnt[kWaves];     // per wave: the run ends of that row
  if (threadIdx.x < 5) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t m = in.fb.m, n = in.fb.n;
  bool end = false, lit = false;
  uint32_t op = kNone, row = 0;
  uint64_t len = 0;
  if (c < m && first[c] < m) {
    op = chunk_op[c];
    row = in.fb.chunk_file[c];
    if (op < m && row < n && (c + 1 == m || first[c + 1] >= m || head[c + 1])) {  // op, row in range: always
      end = true;
      lit = first[c] == c;  // as the head is: a run is of one kind
      len = in.chunk_off[c] + in.fb.chunk_len[c] - op_start[op];
      if (op_len) op_len[op] = len;
    }
  }
  // per row: its ops and its lowest op. The run ends of the wave that share
  // the first one's row count once, and that one's op is their lowest; the
  // waves whose row is wave 0's are added by wave 0.
  const unsigned long long live = __ballot(end);
  const uint32_t lead = live ? fb_first(live) : 0u;
  const uint32_t lrow = __shfl(row, lead);
  const bool same = end && row == lrow;
  const uint32_t cnt = (uint32_t)__popcll(__ballot(same));
  if (end && !same) {
    atomicAdd(&row_ops[row], 1u);
    atomicMin(&row_first[row], op);
  }
  const unsigned long long lits = __ballot(end && lit);
  const uint64_t lb = fb_wave_sum(end && lit ? len : 0ull), cb = fb_wave_sum(end && !lit ? len : 0ull);
  const uint64_t lg = fb_wave_max(len);
  if (lane == lead) {
    s_row[wave] = live ? lrow : kNone;
    s_cnt[wave] = cnt;
    if (live) {
      const uint32_t nl = (uint32_t)__popcll(lits), nc = (uint32_t)__popcll(live) - nl;
      if (nl) atomicAdd(&s_sum[0], (u64a)nl);
      if (nc) atomicAdd(&s_sum[1], (u64a)nc);
      if (lb) atomicAdd(&s_sum[2], (u64a)lb);
      if (cb) atomicAdd(&s_sum[3], (u64a)cb);
      if (lg) atomicMax(&s_sum[4], (u64a)lg);
    }
  }
  __syncthreads();
  if (live && lane == lead) {
    const uint32_t row0 = s_row[0];  // kNone when wave 0 has no run end: no row is that
    uint32_t total = cnt;
    if (wave == 0) {
      for (uint32_t w = 1; w < kWaves; ++w)
        if (s_row[w] == row0) total += s_cnt[w];
    }
    if (wave == 0 || lrow != row0) {  // the other waves of wave 0's row were added by it, and its op is lower
      atomicAdd(&row_ops[lrow], total);
      atomicMin(&row_first[lrow], op);
    }
  }
  if (threadIdx.x < 4 && s_sum[threadIdx.x]) atomicAdd(fr_sc(sc, kRcLitOps + threadIdx.x), s_sum[threadIdx.x]);
  if (threadIdx.x == 4 && s_sum[4]) atomicMax(fr_sc(sc, kRcLongest), s_sum[4]);
}

__global__ void __launch_bounds__(kTB) k_fr_rows(const int64_t* __restrict__ family, uint32_t n,
                                                 const uint32_t* row_ops, const uint32_t* row_first,
                                                 uint32_t* __restrict__ out_ops, uint32_t* __restrict__ out_first,
                                                 u64a* sc) {
  __shared__ uint32_t s_on[kWaves];
  const uint32_t i = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t label;
  const bool on = fb_label(family, n, i, label);
  if (i < n) {
    if (out_ops) out_ops[i] = fb_load(&row_ops[i]);
    if (out_first) out_first[i] = fb_load(&row_first[i]);
  }
  const uint32_t wo = (uint32_t)__popcll(__ballot(on));
  if (lane == 0) s_on[wave] = wo;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t o = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) o += s_on[w];
    if (o) atomicAdd(fr_sc(sc, kRcFiles), (u64a)o);
  }
}

// files, chunks, ops, literal_ops, copy_ops, literal_bytes, copy_bytes, longest_op: the copies of each counter
// folded, the ops from the scan
__global__ void k_fr_totals(const u64a* sc, const uint32_t* __restrict__ tot, u64a* __restrict__ counts) {
  const uint32_t k = threadIdx.x;
  if (blockIdx.x != 0 || k >= kRcWords) return;
  uint64_t v = 0;
  for (uint32_t r = 0; r < kFamilyRecipesScCopies; ++r) {
    const uint64_t x = fb_load(&sc[r * 16 + k]);
    v = k == kRcLongest ? (x > v ? x : v) : v + x;
  }
  counts[k] = k == kRcOps ? (u64a)tot[0] : (u64a)v;
}

}  // namespace

hipError_t family_recipes(uint8_t* ws, const FamilyRecipesIn& in, const FamilyRecipesOut& out,
                          unsigned long long* counts, hipStream_t st) {
  const uint32_t m = in.fb.m, n = in.fb.n;
  const FamilyRecipesLayout l = family_recipes_layout(m, n);
  uint32_t* table = index_at<uint32_t>(ws, l.table);
  uint32_t* row_first = index_at<uint32_t>(ws, l.row_first);
  uint32_t* row_ops = index_at<uint32_t>(ws, l.row_ops);
  u64a* sc = index_at<u64a>(ws, l.sc);
  uint32_t* tot = index_at<uint32_t>(ws, l.tot);
  uint32_t* slot = index_at<uint32_t>(ws, l.slot);
  uint32_t* first = index_at<uint32_t>(ws, l.first);
  uint8_t* head = index_at<uint8_t>(ws, l.head);
  uint32_t* gcnt = index_at<uint32_t>(ws, l.gcnt);
  uint64_t* op_start = index_at<uint64_t>(ws, l.op_start);
  const uint32_t mask = (uint32_t)(l.slots - 1);
  hipError_t e;
  if ((e = hipMemsetAsync(ws + l.table, 0xFF, l.row_ops - l.table, st))) return e;  // table, row_first
  if ((e = hipMemsetAsync(ws + l.row_ops, 0, l.slot - l.row_ops, st))) return e;    // row_ops, sc, tot
  const dim3 block(kTB);
  if (m) {  // without rows no chunk takes part, and every chunk_op says so
    const uint32_t groups = (uint32_t)family_recipes_groups(m);
    const dim3 chunks(groups);
    hipLaunchKernelGGL(k_fr_insert, chunks, block, 0, st, in.fb, table, mask, slot);
    hipLaunchKernelGGL(k_fr_source, chunks, block, 0, st, in, (const uint32_t*)table, mask, (const uint32_t*)slot,
                       first, head, gcnt, sc);
    hipLaunchKernelGGL(k_fr_scan, dim3(1), dim3(1024), 0, st, gcnt, groups, tot);
    hipLaunchKernelGGL(k_fr_emit, chunks, block, 0, st, in, (const uint32_t*)first, (const uint8_t*)head,
                       (const uint32_t*)gcnt, slot, op_start, out);
    hipLaunchKernelGGL(k_fr_close, chunks, block, 0, st, in, (const uint32_t*)first, (const uint8_t*)head,
                       (const uint32_t*)slot, (const uint64_t*)op_start, out.op_len, row_ops, row_first, sc);
    if ((e = hipGetLastError())) return e;
  }
  if (n) {
    hipLaunchKernelGGL(k_fr_rows, dim3((n + kTB - 1) / kTB), block, 0, st, in.fb.family, n, (const uint32_t*)row_ops,
                       (const uint32_t*)row_first, out.row_ops, out.row_first_op, sc);
    if ((e = hipGetLastError())) return e;
  }
  if (counts) {
    hipLaunchKernelGGL(k_fr_totals, dim3(1), dim3(64), 0, st, (const u64a*)sc, (const uint32_t*)tot, counts);
    if ((e = hipGetLastError())) return e;
  }
  return hipSuccess;
}

}  // namespace sdcas
