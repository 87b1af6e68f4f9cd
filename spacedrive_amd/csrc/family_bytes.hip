// family_bytes.hip — the family bytes: chunk_sharing's accounting inside every
// family of rows (include/sdcas.h has the definition; family_bytes.h the
// workspace). A group-by over the class (label of the chunk's row, chunk class
// number), one u64, by confirm.hip's index-table scheme: an open-addressed
// table of u32 chunk positions. A slot goes from empty to a position of ONE
// class by compare-and-swap and from then on only to lower positions of that
// class by atomic min; a prober that meets an occupant recomputes the
// occupant's class from the read-only inputs and moves on when it differs.
// After the insert each slot holds its class's first occurrence, whatever the
// order the chunks arrived in: the results do not depend on scheduling.
//   k_fb_insert    one chunk per thread into the table; remembers its slot (the
//                  class and the insert are family_bytes_device.h's, which
//                  family_recipes.hip shares)
//   k_fb_classify  the chunk's length into its row's delta, self or inherited
//                  sum, by where its class's first occurrence lies
//   k_fb_rows      the row's four outputs; its sums into its label's total,
//                  stored, row count and lowest row
//   k_fb_heads     per row: it is the lowest row of a label with two rows or
//                  more (a set), and that set's reclaimable bytes
//   k_fb_merge     the rows ordered by (head first, reclaimable descending,
//                  row ascending): chunk_peers.hip's merge pass, ceil_log2(n)
//                  launches whatever the data
//   k_fb_write     the first `sets` rows of that order as the set arrays
//   k_fb_totals    the counts
// Two inputs aim everything at one word. One class many times in one family
// (the zero chunk of sparse images): the lanes of a wave that carry its first
// active lane's class send only their lowest position. One file with very many
// chunks, or one family of everything: the lanes of a wave that share the first
// lane's row (label) add up in the wave and add once; in k_fb_classify the
// waves of a workgroup that share wave 0's row add up once more in LDS.
//
// The per-XCD L2s are not coherent with each other and a CU's L1 is never
// refreshed by another CU's stores: table words, per-row and per-label sums and
// the counters are touched only by agent-scope atomics and relaxed agent-scope
// atomic loads, and every phase is a launch of its own. The inputs are plain
// loads. No thread waits for a value another thread has yet to write.
#include <hip/hip_runtime.h>

#include "chunk_index.h"
#include "family_bytes.h"
#include "family_bytes_device.h"

namespace sdcas {

namespace {

constexpr uint32_t kTB = kFamilyBytesTB;
constexpr uint32_t kNone = kFbNone;
enum { kScFiles, kScChunks, kScClasses, kScTotal, kScStored, kScSets, kScMembers, kScSetReclaimable, kScLargest, kScWords };
static_assert(kScWords == kFamilyBytesCounts, "sdcas_family_bytes_counts' order");

__global__ void __launch_bounds__(kTB) k_fb_insert(FamilyBytesIn in, uint32_t* table, uint32_t mask,
                                                   uint32_t* __restrict__ slot) {
  fb_insert(in, table, mask, slot);  // family_bytes_device.h, shared with family_recipes.hip
}

__global__ void __launch_bounds__(kTB) k_fb_classify(FamilyBytesIn in, const uint32_t* table, uint32_t mask,
                                                     const uint32_t* __restrict__ slot, u64a* row_sum, u64a* sc) {
  __shared__ u64a s_cnt[2];  // chunks, classes
  __shared__ uint32_t s_row[kTB / 64];   // per wave: its first participating chunk's row
  __shared__ u64a s_part[kTB / 64][3];  // per wave: that row's delta, self and inherited bytes
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool on = false;
  uint32_t row = 0, kind = 0;  // 0 delta, 1 self, 2 inherited
  uint64_t len = 0;
  if (c < in.m) {
    const uint32_t s = slot[c];
    if (s <= mask) {  // not kNone: the chunk takes part
      const uint32_t first = fb_load(&table[s]);
      row = in.chunk_file[c];
      if (first < in.m && row < in.n) {  // always
        on = true;
        len = in.chunk_len[c];
        kind = first == c ? 0u : in.chunk_file[first] == row ? 1u : 2u;
      }
    }
  }
  // The lanes that share the first active lane's row add up in the wave, and
  // the waves whose row is wave 0's add up in the workgroup: a file of very
  // many chunks is one add per kind and workgroup, not 256 to one word. The
  // other lanes add their own.
  const unsigned long long live = __ballot(on);
  const uint32_t lead = live ? fb_first(live) : 0u;
  const uint32_t lrow = __shfl(row, lead);
  const bool same = on && row == lrow;
  uint64_t sum[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) sum[k] = fb_wave_sum(same && kind == k ? len : 0ull);
  if (on && !same && len) atomicAdd(&row_sum[kind * (size_t)in.n + row], (u64a)len);
  const uint32_t firsts = (uint32_t)__popcll(__ballot(on && kind == 0));
  if (lane == lead) {
    s_row[wave] = live ? lrow : kNone;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) s_part[wave][k] = sum[k];
    if (live) atomicAdd(&s_cnt[0], (u64a)__popcll(live));
    if (firsts) atomicAdd(&s_cnt[1], (u64a)firsts);
  }
  __syncthreads();
  if (live && lane == lead) {
    const uint32_t row0 = s_row[0];  // kNone when wave 0 holds no participating chunk: no row is that
    if (wave == 0) {
      for (uint32_t w = 1; w < kTB / 64; ++w)
        if (s_row[w] == row0) {
#pragma unroll
          for (uint32_t k = 0; k < 3; ++k) sum[k] += s_part[w][k];
        }
    }
    if (wave == 0 || lrow != row0) {  // the other waves of wave 0's row were added by it
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k)
        if (sum[k]) atomicAdd(&row_sum[k * (size_t)in.n + lrow], (u64a)sum[k]);
    }
  }
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&sc[kScChunks + threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(kTB) k_fb_rows(const int64_t* __restrict__ family, uint32_t n, const u64a* row_sum,
                                                 FamilyBytesOut out, u64a* lab_total, u64a* lab_stored,
                                                 uint32_t* lab_rows, uint32_t* lab_low, u64a* sc) {
  __shared__ u64a s_sum[3];  // files, total, stored
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  uint32_t label = 0;
  const bool on = fb_label(family, n, i, label);
  uint64_t delta = 0, own = 0, inherited = 0;
  if (on) {
    delta = fb_load(&row_sum[i]);
    own = fb_load(&row_sum[(size_t)n + i]);
    inherited = fb_load(&row_sum[2 * (size_t)n + i]);
  }
  const uint64_t file = delta + own + inherited;
  if (i < n) {
    if (out.file_bytes) out.file_bytes[i] = file;
    if (out.delta_bytes) out.delta_bytes[i] = delta;
    if (out.self_bytes) out.self_bytes[i] = own;
    if (out.inherited_bytes) out.inherited_bytes[i] = inherited;
  }
  const unsigned long long live = __ballot(on);
  if (live) {  // the whole wave alike
    // the rows that share the first participating row's label add once, and
    // that row is their lowest
    const uint32_t lead = fb_first(live);
    const uint32_t ll = __shfl(label, lead);
    const bool same = on && label == ll;
    const uint64_t t = fb_wave_sum(same ? file : 0ull), s = fb_wave_sum(same ? delta : 0ull);
    const uint32_t rows = (uint32_t)__popcll(__ballot(same));
    if (lane == lead) {
      if (t) atomicAdd(&lab_total[ll], (u64a)t);
      if (s) atomicAdd(&lab_stored[ll], (u64a)s);
      atomicAdd(&lab_rows[ll], rows);
      atomicMin(&lab_low[ll], i);
    } else if (on && !same) {
      if (file) atomicAdd(&lab_total[label], (u64a)file);
      if (delta) atomicAdd(&lab_stored[label], (u64a)delta);
      atomicAdd(&lab_rows[label], 1u);
      atomicMin(&lab_low[label], i);
    }
    const uint64_t wt = fb_wave_sum(file), wsd = fb_wave_sum(delta);
    if (lane == 0) {
      atomicAdd(&s_sum[0], (u64a)__popcll(live));
      if (wt) atomicAdd(&s_sum[1], (u64a)wt);
      if (wsd) atomicAdd(&s_sum[2], (u64a)wsd);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_sum[0]) atomicAdd(&sc[kScFiles], s_sum[0]);
  if (threadIdx.x == 1 && s_sum[1]) atomicAdd(&sc[kScTotal], s_sum[1]);
  if (threadIdx.x == 2 && s_sum[2]) atomicAdd(&sc[kScStored], s_sum[2]);
}

__global__ void __launch_bounds__(kTB) k_fb_heads(const int64_t* __restrict__ family, uint32_t n, const u64a* lab_total,
                                                  const u64a* lab_stored, const uint32_t* lab_rows,
                                                  const uint32_t* lab_low, uint64_t* __restrict__ rec,
                                                  uint8_t* __restrict__ head, uint32_t* __restrict__ ord, u64a* sc) {
  __shared__ u64a s_sum[4];  // sets, members, set reclaimable, largest
  if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  uint32_t label = 0;
  uint64_t members = 0, back = 0;
  bool hd = false;
  if (fb_label(family, n, i, label)) {
    const uint32_t rows = fb_load(&lab_rows[label]);
    hd = rows >= 2 && fb_load(&lab_low[label]) == i;
    if (hd) {
      members = rows;
      back = fb_load(&lab_total[label]) - fb_load(&lab_stored[label]);
    }
  }
  if (i < n) rec[i] = back, head[i] = hd ? 1 : 0, ord[i] = i;
  const unsigned long long heads = __ballot(hd);
  if (heads) {  // the whole wave alike
    const uint64_t wm = fb_wave_sum(members), wb = fb_wave_sum(back), wl = fb_wave_max(back);
    if (lane == 0) {
      atomicAdd(&s_sum[0], (u64a)__popcll(heads));
      atomicAdd(&s_sum[1], (u64a)wm);
      if (wb) atomicAdd(&s_sum[2], (u64a)wb);
      if (wl) atomicMax(&s_sum[3], (u64a)wl);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&sc[kScSets + threadIdx.x], s_sum[threadIdx.x]);
  if (threadIdx.x == 3 && s_sum[3]) atomicMax(&sc[kScLargest], s_sum[3]);
}

// row a orders before row b: the heads first, by reclaimable bytes descending,
// then by row; a total order
__device__ __forceinline__ bool fb_less(const uint64_t* __restrict__ rec, const uint8_t* __restrict__ head, uint32_t a,
                                        uint32_t b) {
  const bool ha = head[a], hb = head[b];
  if (ha != hb) return ha;
  if (ha) {
    const uint64_t ra = rec[a], rb = rec[b];
    if (ra != rb) return ra > rb;
  }
  return a < b;
}

// One pass of the merge sort over the n rows (chunk_peers.hip's k_cp_merge with
// the count on the host): `in` holds the rows in runs of w places, each run in
// order; every pair of neighbouring runs is merged into `out`. A row goes to
// its rank in its own run plus the number of the sibling run's rows before it,
// found by halving: at most 30 steps per thread and pass, whatever the data.
__global__ void __launch_bounds__(kTB) k_fb_merge(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                  const uint64_t* __restrict__ rec, const uint8_t* __restrict__ head,
                                                  uint32_t w, uint32_t n) {
  const uint32_t p = blockIdx.x * kTB + threadIdx.x;
  if (p >= n) return;
  const uint32_t c = in[p];
  if (c >= n) return;  // never: `in` holds row numbers
  const uint64_t first64 = (uint64_t)p / (2ull * w) * (2ull * w);
  const uint32_t first = (uint32_t)first64;
  const uint32_t mid = (uint32_t)(first64 + w < n ? first64 + w : n);
  const uint32_t end = (uint32_t)(first64 + 2ull * w < n ? first64 + 2ull * w : n);
  const bool left = p < mid;
  uint32_t lo = left ? mid : first, hi = left ? end : mid;
  const uint32_t sib = lo;
  while (lo < hi) {  // the sibling run's rows before c
    const uint32_t q = lo + ((hi - lo) >> 1);
    const uint32_t e = in[q];
    if (e < n && fb_less(rec, head, e, c)) lo = q + 1;
    else hi = q;
  }
  const uint32_t at = first + (p - (left ? first : mid)) + (lo - sib);
  if (at < n) out[at] = c;  // always: a rank among the pair's end - first places
}

__global__ void __launch_bounds__(kTB) k_fb_write(const uint32_t* __restrict__ ord, const int64_t* __restrict__ family,
                                                  uint32_t n, uint32_t half, const u64a* lab_total,
                                                  const u64a* lab_stored, const uint32_t* lab_rows, const u64a* sc,
                                                  FamilyBytesOut out) {
  const uint32_t p = blockIdx.x * kTB + threadIdx.x;
  const uint64_t sets = fb_load(&sc[kScSets]);
  if (p >= half || p >= sets) return;  // the set arrays hold n / 2 entries
  const uint32_t r = ord[p];
  uint32_t label;
  if (!fb_label(family, n, r, label)) return;  // never: a head takes part
  if (out.set_rep) out.set_rep[p] = (int64_t)r;
  if (out.set_files) out.set_files[p] = fb_load(&lab_rows[label]);
  if (out.set_total) out.set_total[p] = fb_load(&lab_total[label]);
  if (out.set_stored) out.set_stored[p] = fb_load(&lab_stored[label]);
}

// files, chunks, classes, total_bytes, stored_bytes, sets, members, set_reclaimable_bytes, largest_reclaimable
__global__ void k_fb_totals(const u64a* sc, u64a* __restrict__ counts) {
  if (blockIdx.x == 0 && threadIdx.x < kScWords) counts[threadIdx.x] = fb_load(&sc[threadIdx.x]);
}

}  // namespace

hipError_t family_bytes(uint8_t* ws, const FamilyBytesIn& in, const FamilyBytesOut& out, unsigned long long* counts,
                        hipStream_t st) {
  const FamilyBytesLayout l = family_bytes_layout(in.m, in.n);
  uint32_t* table = index_at<uint32_t>(ws, l.table);
  uint32_t* lab_low = index_at<uint32_t>(ws, l.lab_low);
  u64a* row_sum = index_at<u64a>(ws, l.row_sum);
  u64a* lab_total = index_at<u64a>(ws, l.lab_total);
  u64a* lab_stored = index_at<u64a>(ws, l.lab_stored);
  uint32_t* lab_rows = index_at<uint32_t>(ws, l.lab_rows);
  u64a* sc = index_at<u64a>(ws, l.sc);
  uint32_t* slot = index_at<uint32_t>(ws, l.slot);
  uint64_t* rec = index_at<uint64_t>(ws, l.rec);
  uint8_t* head = index_at<uint8_t>(ws, l.head);
  uint32_t* src = index_at<uint32_t>(ws, l.ord0);
  uint32_t* dst = index_at<uint32_t>(ws, l.ord1);
  const uint32_t m = in.m, n = in.n, mask = (uint32_t)(l.slots - 1);
  hipError_t e;
  if ((e = hipMemsetAsync(ws + l.table, 0xFF, l.row_sum - l.table, st))) return e;  // table, lab_low
  if ((e = hipMemsetAsync(ws + l.row_sum, 0, l.slot - l.row_sum, st))) return e;    // the sums and sc
  const dim3 block(kTB);
  if (n) {  // without rows no chunk takes part
    const dim3 rows((n + kTB - 1) / kTB);
    if (m) {
      const dim3 chunks((m + kTB - 1) / kTB);
      hipLaunchKernelGGL(k_fb_insert, chunks, block, 0, st, in, table, mask, slot);
      hipLaunchKernelGGL(k_fb_classify, chunks, block, 0, st, in, (const uint32_t*)table, mask, (const uint32_t*)slot,
                         row_sum, sc);
      if ((e = hipGetLastError())) return e;
    }
    hipLaunchKernelGGL(k_fb_rows, rows, block, 0, st, in.family, n, (const u64a*)row_sum, out, lab_total, lab_stored,
                       lab_rows, lab_low, sc);
    hipLaunchKernelGGL(k_fb_heads, rows, block, 0, st, in.family, n, (const u64a*)lab_total, (const u64a*)lab_stored,
                       (const uint32_t*)lab_rows, (const uint32_t*)lab_low, rec, head, src, sc);
    if ((e = hipGetLastError())) return e;
    const uint32_t half = n / 2;
    if (half && (out.set_rep || out.set_files || out.set_total || out.set_stored)) {
      const uint32_t passes = family_bytes_passes(n);
      for (uint32_t p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(k_fb_merge, rows, block, 0, st, (const uint32_t*)src, dst, (const uint64_t*)rec,
                           (const uint8_t*)head, 1u << p, n);
        uint32_t* t = src;
        src = dst, dst = t;
      }
      hipLaunchKernelGGL(k_fb_write, dim3((half + kTB - 1) / kTB), block, 0, st, (const uint32_t*)src, in.family, n,
                         half, (const u64a*)lab_total, (const u64a*)lab_stored, (const uint32_t*)lab_rows,
                         (const u64a*)sc, out);
      if ((e = hipGetLastError())) return e;
    }
  }
  if (counts) {
    hipLaunchKernelGGL(k_fb_totals, dim3(1), dim3(64), 0, st, (const u64a*)sc, counts);
    if ((e = hipGetLastError())) return e;
  }
  return hipSuccess;
}

}  // namespace sdcas
