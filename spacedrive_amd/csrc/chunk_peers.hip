// chunk_peers.hip — the chunk peers: for a batch's chunks, per file, the bytes
// it shares with every file that holds any of them in a holders index
// (chunk_holders.hip), and the top k of those files (include/sdcas.h has the
// definition; chunk_peers.h the workspace).
//
// The counted holders of a chunk are a contiguous piece of its pair's run: in
// EARLIER mode the entries below the file's own id, in ALL mode the run without
// the file's own entry. As in the holders index no thread's work follows the
// length of a run — not a pair's run in the index, not a file's run of equal
// (file, holder) pairs, not a file's run of edges: run ends are found by
// halving, orders by merging, sums by scan differences. Every grid is sized
// from m, n_files or max_pairs; P (the pairs) and the edges stay on the device.
//   k_cp_runs      one chunk per thread: its bucket, the pair's two bounds and
//                  the lower bound of (key, digest, file id): first, cnt (0 when
//                  common or no part), self's place; the per-file shared /
//                  unique / common bytes by u64 atomic adds (sums modulo 2^64:
//                  the order is free); P, the chunks and the common chunks
//   k_ch_scan      cnt scanned in tiles of 256 and the three levels above
//                  (holders_device.h); k_cp_offsets adds the levels: off[c]
//   k_cp_fix       P against max_pairs: the places to expand, or overflow
//   k_cp_expand    one pair place per thread: its chunk by halving in off, the
//                  holder from the index (past self in ALL mode)
//   k_cp_merge     the places ordered by (file, holder, place): a merge sort by
//                  halving, one launch per doubling of the bound
//   k_cp_heads     a head where (file, holder) differs from the place before;
//                  the heads per workgroup; the lengths in that order
//   k_cp_scan64    the lengths scanned (u64, tiles of 256 and three levels)
//   k_cp_edges     a head stores its edge (file, holder) at its rank among the
//                  heads, with the scan before it; its run's last place stores
//                  the scan behind it: the edge's bytes are the difference
//   k_cp_edge_init the difference taken, the edges numbered
//   k_cp_merge     the edges ordered by (file, bytes descending, holder)
//   k_cp_write     one edge per thread: its rank in its file is its place less
//                  the file's first place (a lower bound by file); ranks below k
//                  are stored, the file's last edge stores the count
//   k_cp_totals    the counts
// Every directory value is clamped to n, every computed place is checked
// against its array's bound before a store.
#include <hip/hip_runtime.h>

#include "chunk_peers.h"
#include "holders_device.h"
#include "index_device.h"

namespace sdcas {

namespace {

constexpr uint32_t kCpNoSelf = 0xFFFFFFFFu;

// the pair places' order: (file, holder, place)
struct CpPairLess {
  const uint32_t* file;
  const uint64_t* holder;
  __device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const {
    const uint32_t fa = file[a], fb = file[b];
    if (fa != fb) return fa < fb;
    const uint64_t ha = holder[a], hb = holder[b];
    if (ha != hb) return ha < hb;
    return a < b;
  }
};
// the edges' order: (file, bytes descending, holder); no two edges share (file, holder)
struct CpEdgeLess {
  const uint32_t* file;
  const uint64_t* bytes;
  const uint64_t* holder;
  __device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const {
    const uint32_t fa = file[a], fb = file[b];
    if (fa != fb) return fa < fb;
    const uint64_t ba = bytes[a], bb = bytes[b];
    if (ba != bb) return ba > bb;
    const uint64_t ha = holder[a], hb = holder[b];
    if (ha != hb) return ha < hb;
    return a < b;
  }
};

__global__ void __launch_bounds__(kChTB) k_cp_runs(IndexView ix, PeersIn in, uint32_t* __restrict__ first,
                                                   uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                   uint32_t* __restrict__ self, PeersOut out,
                                                   unsigned long long* __restrict__ sc) {
  __shared__ unsigned long long s_sum[3];  // pairs, chunks, common chunks
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * kChTB + threadIdx.x;
  if (c < in.m) {
    const uint32_t f = in.chunk_file[c];
    const bool take = (!in.valid || in.valid[c]) && f < in.n_files;
    uint32_t fst = 0, counted = 0, sp = kCpNoSelf;
    if (take) {
      const uint64_t len = in.chunk_len[c], fid = in.file_ids[f];
      uint32_t holders = 0;
      if (ix.n) {
        const uint64_t key = in.keys[c];
        const IxDigest dig = ix_digest(in.digests, c);
        uint32_t lo, hi;
        ix_bucket(ix, key, lo, hi);
        fst = ch_pair_bound(ix, lo, hi, key, dig, false);
        // the run's end lies in the same bucket: its entries share the key
        const uint32_t end = ch_pair_bound(ix, fst, hi, key, dig, true);
        if (end > fst) {
          bool found;
          uint32_t split = ch_lower_bound3(ix, ChTriple{key, dig, fid}, found);
          split = split < fst ? fst : ix_min(split, end);  // always inside the run
          if (in.mode == kPeersAll) {
            holders = end - fst - (found ? 1u : 0u);
            if (found) sp = split - fst;
          } else {
            holders = split - fst;
          }
        }
      }
      const bool common = holders > in.max_holders;
      counted = common ? 0u : holders;
      uint64_t* dst = common ? out.common : holders ? out.shared : out.unique;
      if (dst && len) atomicAdd(reinterpret_cast<unsigned long long*>(dst) + f, (unsigned long long)len);
      atomicAdd(&s_sum[1], 1ull);
      if (common) atomicAdd(&s_sum[2], 1ull);
      if (counted) atomicAdd(&s_sum[0], (unsigned long long)counted);
    }
    first[c] = fst, cnt[c] = counted, off[c] = counted, self[c] = sp;
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&sc[threadIdx.x], s_sum[threadIdx.x]);
}

// off[c]: the scan within c's tile plus the tiles before it
__global__ void __launch_bounds__(kChTB) k_cp_offsets(uint32_t* __restrict__ off, const uint32_t* __restrict__ l1,
                                                      const uint32_t* __restrict__ l2, const uint32_t* __restrict__ l3,
                                                      uint32_t m) {
  const uint32_t c = blockIdx.x * kChTB + threadIdx.x;
  if (c < m) off[c] += ch_base(l1, l2, l3, blockIdx.x);
}

// np[0] <- the places to expand, np[1] <- overflow. With P > cap nothing is
// expanded (and off, a 32-bit scan, may have wrapped: nothing reads it then).
__global__ void k_cp_fix(const unsigned long long* __restrict__ sc, uint32_t cap, uint32_t* __restrict__ np) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const bool over = sc[0] > cap;
    np[0] = over ? 0u : (uint32_t)sc[0];
    np[1] = over ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(kChTB) k_cp_expand(IndexView ix, PeersIn in, const uint32_t* __restrict__ first,
                                                     const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ off,
                                                     const uint32_t* __restrict__ self,
                                                     const uint32_t* __restrict__ np, uint32_t cap,
                                                     uint32_t* __restrict__ p_file, uint64_t* __restrict__ p_holder,
                                                     uint64_t* __restrict__ p_len, uint32_t* __restrict__ ord) {
  const uint32_t n = ix_min(np[0], cap);
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  if (p >= n) return;
  // the last chunk whose offset is <= p: chunks without pairs share the offset of the next one with some
  const uint32_t u = ix_upper(off, 0, in.m, p);
  uint32_t file = in.n_files;  // never stored: no file, the place scores for nobody
  uint64_t holder = 0, len = 0;
  if (u) {  // always: off[0] == 0
    const uint32_t c = u - 1;
    uint32_t j = p - off[c];
    if (j < cnt[c]) {  // always
      const uint32_t sp = self[c];
      if (sp != kCpNoSelf && j >= sp) ++j;
      const uint32_t e = first[c] + j;
      if (e < ix.n) {  // always: a place inside the run
        file = in.chunk_file[c];
        holder = ix.values ? ix.values[e] : 0ull;
        len = in.chunk_len[c];
      }
    }
  }
  p_file[p] = file, p_holder[p] = holder, p_len[p] = len, ord[p] = p;
}

// One pass of the merge sort over the first n = min(*n_p, cap) items by `less`,
// a total order. `in` holds the items in runs of w places, each run in order;
// every pair of neighbouring runs is merged into `out`. An item goes to its
// rank in its own run plus the number of the sibling run's items before it,
// found by halving: at most 30 steps per thread and pass, whatever the data.
// A pass whose w is n or more copies.
template <class Less>
__global__ void __launch_bounds__(kChTB) k_cp_merge(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                    Less less, uint32_t w, uint32_t cap,
                                                    const uint32_t* __restrict__ n_p) {
  const uint32_t n = ix_min(*n_p, cap);
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  if (p >= n) return;
  const uint32_t c = in[p];
  if (c >= n) return;  // never: `in` holds item numbers
  const uint32_t first = p / (2 * w) * (2 * w);  // w <= 2^29: 2 w fits
  const uint32_t mid = ix_min(first + w, n), end = ix_min(first + 2 * w, n);
  const bool left = p < mid;
  uint32_t lo = left ? mid : first, hi = left ? end : mid;
  const uint32_t sib = lo;
  while (lo < hi) {  // the sibling run's items before c
    const uint32_t q = lo + ((hi - lo) >> 1);
    const uint32_t e = in[q];
    if (e < n && less(e, c)) lo = q + 1;
    else hi = q;
  }
  const uint32_t at = first + (p - (left ? first : mid)) + (lo - sib);
  if (at < n) out[at] = c;  // always: a rank among the pair's end - first places
}

// head[p], the heads per workgroup into l1, run[p] <- the length at place p of the order
__global__ void __launch_bounds__(kChTB) k_cp_heads(const uint32_t* __restrict__ ord,
                                                    const uint32_t* __restrict__ p_file,
                                                    const uint64_t* __restrict__ p_holder,
                                                    const uint64_t* __restrict__ p_len,
                                                    const uint32_t* __restrict__ np, uint32_t cap,
                                                    uint64_t* __restrict__ run, uint8_t* __restrict__ head,
                                                    uint32_t* __restrict__ l1) {
  __shared__ uint32_t s_w[kChTB / 64];
  const uint32_t n = ix_min(np[0], cap);
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  bool h = false;
  if (p < n) {
    const uint32_t c = ord[p];
    uint64_t len = 0;
    if (c < n) {  // always
      h = p == 0;
      if (!h) {
        const uint32_t b = ord[p - 1];
        h = b >= n || p_file[b] != p_file[c] || p_holder[b] != p_holder[c];
      }
      len = p_len[c];
    }
    run[p] = len;
    head[p] = h ? 1 : 0;
  }
  uint32_t total;
  (void)ch_rank(h, s_w, &total);
  if (threadIdx.x == 0) l1[blockIdx.x] = total;
}

// One level of the u64 scan, k_ch_scan's shape: every workgroup turns its 256
// sums of a[0 .. n) into their exclusive scan and leaves their sum in
// up[blockIdx.x]; n is min(*n_p, n_max) when n_p is given.
__global__ void __launch_bounds__(kChTB) k_cp_scan64(unsigned long long* __restrict__ a, uint32_t n_max,
                                                     const uint32_t* __restrict__ n_p,
                                                     unsigned long long* __restrict__ up) {
  __shared__ unsigned long long s_w[kChTB / 64];
  const uint32_t n = n_p ? ix_min(*n_p, n_max) : n_max;
  const uint32_t i = blockIdx.x * kChTB + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long v = i < n ? a[i] : 0ull;
  unsigned long long inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kChTB / 64; ++w) {
    const unsigned long long t = s_w[w];
    before += w < wave ? t : 0ull;
    all += t;
  }
  if (i < n) a[i] = before + inc - v;
  if (threadIdx.x == 0) up[blockIdx.x] = all;
}

// the sum of the lengths at the places before p, from the four scanned levels
__device__ __forceinline__ uint64_t cp_before(const uint64_t* __restrict__ run, const uint64_t* __restrict__ s1,
                                              const uint64_t* __restrict__ s2, const uint64_t* __restrict__ s3,
                                              uint32_t p) {
  return run[p] + s1[p >> 8] + s2[p >> 16] + s3[p >> 24];
}

__global__ void __launch_bounds__(kChTB) k_cp_edges(const uint32_t* __restrict__ ord,
                                                    const uint32_t* __restrict__ p_file,
                                                    const uint64_t* __restrict__ p_holder,
                                                    const uint64_t* __restrict__ run, const uint64_t* __restrict__ s1,
                                                    const uint64_t* __restrict__ s2, const uint64_t* __restrict__ s3,
                                                    const uint64_t* __restrict__ stot,
                                                    const uint8_t* __restrict__ head, const uint32_t* __restrict__ l1,
                                                    const uint32_t* __restrict__ l2, const uint32_t* __restrict__ l3,
                                                    const uint32_t* __restrict__ np, uint32_t cap,
                                                    uint32_t* __restrict__ e_file, uint64_t* __restrict__ e_holder,
                                                    uint64_t* __restrict__ e_beg, uint64_t* __restrict__ e_end) {
  __shared__ uint32_t s_w[kChTB / 64];
  const uint32_t n = ix_min(np[0], cap);
  const uint32_t p = blockIdx.x * kChTB + threadIdx.x;
  const bool h = p < n && head[p];
  uint32_t total;
  const uint32_t rank = ch_base(l1, l2, l3, blockIdx.x) + ch_rank(h, s_w, &total);  // the heads before p
  if (p >= n) return;
  if (h && rank < cap) {  // always: a rank among at most n heads
    const uint32_t c = ord[p];
    if (c < n) e_file[rank] = p_file[c], e_holder[rank] = p_holder[c];
    e_beg[rank] = cp_before(run, s1, s2, s3, p);
  }
  const uint32_t upto = rank + (h ? 1u : 0u);  // the heads at places <= p
  const bool tail = p + 1 == n || head[p + 1];
  if (tail && upto && upto - 1 < cap) e_end[upto - 1] = p + 1 == n ? stot[0] : cp_before(run, s1, s2, s3, p + 1);
}

// e_beg[r] <- the edge's bytes, ord[r] <- r
__global__ void __launch_bounds__(kChTB) k_cp_edge_init(uint64_t* __restrict__ e_beg, const uint64_t* __restrict__ e_end,
                                                        const uint32_t* __restrict__ ne_p, uint32_t cap,
                                                        uint32_t* __restrict__ ord) {
  const uint32_t n = ix_min(*ne_p, cap);
  const uint32_t r = blockIdx.x * kChTB + threadIdx.x;
  if (r >= n) return;
  e_beg[r] = e_end[r] - e_beg[r];
  ord[r] = r;
}

__global__ void __launch_bounds__(kChTB) k_cp_write(const uint32_t* __restrict__ ord,
                                                    const uint32_t* __restrict__ e_file,
                                                    const uint64_t* __restrict__ e_holder,
                                                    const uint64_t* __restrict__ e_bytes,
                                                    const uint32_t* __restrict__ ne_p, uint32_t cap, uint32_t n_files,
                                                    uint32_t k, PeersOut out, unsigned long long* __restrict__ sc) {
  const uint32_t n = ix_min(*ne_p, cap);
  const uint32_t r = blockIdx.x * kChTB + threadIdx.x;
  bool top = false;
  if (r < n) {
    const uint32_t e = ord[r];
    const uint32_t f = e < n ? e_file[e] : n_files;
    if (f < n_files) {  // always
      uint32_t lo = 0, hi = r;
      while (lo < hi) {  // the first place of f's edges
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t g = ord[mid];
        if (g < n && e_file[g] < f) lo = mid + 1;
        else hi = mid;
      }
      const uint32_t rank = r - lo;
      top = rank == 0;
      if (rank < k) {
        const size_t at = (size_t)f * k + rank;
        if (out.peers) out.peers[at] = e_holder[e];
        if (out.peer_bytes) out.peer_bytes[at] = e_bytes[e];
      }
      bool last = r + 1 == n;
      if (!last) {
        const uint32_t g = ord[r + 1];
        last = g >= n || e_file[g] != f;
      }
      if (last && out.peer_count) out.peer_count[f] = ix_min(k, rank + 1);
    }
  }
  const uint32_t tops = (uint32_t)__popcll(__ballot(top));
  if (tops && (threadIdx.x & 63) == 0) atomicAdd(&sc[3], (unsigned long long)tops);
}

// files, chunks, common_chunks, pairs, edges, files_with_peer, overflow
__global__ void k_cp_totals(const unsigned long long* __restrict__ sc, const uint32_t* __restrict__ np,
                            const uint32_t* __restrict__ ne_p, uint32_t cap, uint32_t n_files,
                            unsigned long long* __restrict__ counts) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    counts[0] = n_files;
    counts[1] = sc[1];
    counts[2] = sc[2];
    counts[3] = sc[0];
    counts[4] = ix_min(*ne_p, cap);
    counts[5] = sc[3];
    counts[6] = np[1];
  }
}

template <class Less>
uint32_t* cp_sort(uint32_t* src, uint32_t* dst, Less less, uint32_t cap, const uint32_t* n_p, hipStream_t st) {
  const dim3 block(kChTB), grid(index_blocks(cap));
  for (uint64_t w = 1; w < cap; w <<= 1) {
    hipLaunchKernelGGL(k_cp_merge<Less>, grid, block, 0, st, (const uint32_t*)src, dst, less, (uint32_t)w, cap, n_p);
    uint32_t* t = src;
    src = dst, dst = t;
  }
  return src;
}

}  // namespace

hipError_t chunk_peers(uint8_t* ws, const IndexView& idx, const PeersIn& in, uint32_t max_pairs, const PeersOut& out,
                       unsigned long long* counts, hipStream_t st) {
  const PeersLayout l = peers_layout(in.m, max_pairs);
  uint32_t* first = index_at<uint32_t>(ws, l.first);
  uint32_t* cnt = index_at<uint32_t>(ws, l.cnt);
  uint32_t* off = index_at<uint32_t>(ws, l.off);
  uint32_t* self = index_at<uint32_t>(ws, l.self);
  uint32_t* p_file = index_at<uint32_t>(ws, l.p_file);
  uint64_t* p_holder = index_at<uint64_t>(ws, l.p_holder);
  uint64_t* p_len = index_at<uint64_t>(ws, l.p_len);
  uint32_t* ord_a = index_at<uint32_t>(ws, l.ord_a);
  uint32_t* ord_b = index_at<uint32_t>(ws, l.ord_b);
  uint64_t* run = index_at<uint64_t>(ws, l.run);
  uint64_t* s1 = index_at<uint64_t>(ws, l.s1);
  uint64_t* s2 = index_at<uint64_t>(ws, l.s2);
  uint64_t* s3 = index_at<uint64_t>(ws, l.s3);
  uint64_t* stot = index_at<uint64_t>(ws, l.stot);
  uint8_t* head = index_at<uint8_t>(ws, l.head);
  uint32_t* e_file = index_at<uint32_t>(ws, l.e_file);
  uint64_t* e_holder = index_at<uint64_t>(ws, l.e_holder);
  uint64_t* e_beg = index_at<uint64_t>(ws, l.e_beg);
  uint64_t* e_end = p_len;  // the lengths live on in `run` by then
  unsigned long long* sc = index_at<unsigned long long>(ws, l.sc);
  uint32_t* np = index_at<uint32_t>(ws, l.np);
  unsigned long long* cts = index_at<unsigned long long>(ws, l.counts);
  uint32_t* ne = index_at<uint32_t>(ws, l.hscan.tot);
  const uint32_t m = in.m, cap = max_pairs;
  const size_t nf = in.n_files;
  const dim3 block(kChTB);
  hipError_t e;
  if ((e = hipMemsetAsync(sc, 0, l.bytes - l.sc, st))) return e;  // sc, np and counts
  if ((e = hipMemsetAsync(ne, 0, 16, st))) return e;
  // every slot of every output is written: zero, then the sums and the stored ranks
  if (nf) {
    if (out.peer_count && (e = hipMemsetAsync(out.peer_count, 0, 4 * nf, st))) return e;
    if (out.peers && (e = hipMemsetAsync(out.peers, 0, 8 * nf * in.k, st))) return e;
    if (out.peer_bytes && (e = hipMemsetAsync(out.peer_bytes, 0, 8 * nf * in.k, st))) return e;
    if (out.shared && (e = hipMemsetAsync(out.shared, 0, 8 * nf, st))) return e;
    if (out.unique && (e = hipMemsetAsync(out.unique, 0, 8 * nf, st))) return e;
    if (out.common && (e = hipMemsetAsync(out.common, 0, 8 * nf, st))) return e;
  }
  if (m) {
    const dim3 grid(index_blocks(m));
    uint32_t* l1 = index_at<uint32_t>(ws, l.cscan.l1);
    hipLaunchKernelGGL(k_cp_runs, grid, block, 0, st, idx, in, first, cnt, off, self, out, sc);
    hipLaunchKernelGGL(k_ch_scan, dim3(l.cscan.n1), block, 0, st, off, m, l1);
    ch_scan(ws, l.cscan, st);
    hipLaunchKernelGGL(k_cp_offsets, grid, block, 0, st, off, (const uint32_t*)l1,
                       (const uint32_t*)index_at<uint32_t>(ws, l.cscan.l2),
                       (const uint32_t*)index_at<uint32_t>(ws, l.cscan.l3), m);
    if ((e = hipGetLastError())) return e;
  }
  hipLaunchKernelGGL(k_cp_fix, dim3(1), dim3(64), 0, st, (const unsigned long long*)sc, cap, np);
  if (m && cap) {
    const dim3 grid(index_blocks(cap));
    hipLaunchKernelGGL(k_cp_expand, grid, block, 0, st, idx, in, (const uint32_t*)first, (const uint32_t*)cnt,
                       (const uint32_t*)off, (const uint32_t*)self, (const uint32_t*)np, cap, p_file, p_holder, p_len,
                       ord_a);
    const uint32_t* ord = cp_sort(ord_a, ord_b, CpPairLess{p_file, p_holder}, cap, np, st);
    if ((e = hipGetLastError())) return e;
    uint32_t* h1 = index_at<uint32_t>(ws, l.hscan.l1);
    const uint32_t* h2 = index_at<uint32_t>(ws, l.hscan.l2);
    const uint32_t* h3 = index_at<uint32_t>(ws, l.hscan.l3);
    hipLaunchKernelGGL(k_cp_heads, grid, block, 0, st, ord, (const uint32_t*)p_file, (const uint64_t*)p_holder,
                       (const uint64_t*)p_len, (const uint32_t*)np, cap, run, head, h1);
    ch_scan(ws, l.hscan, st);
    hipLaunchKernelGGL(k_cp_scan64, dim3(l.n1), block, 0, st, (unsigned long long*)run, cap, (const uint32_t*)np,
                       (unsigned long long*)s1);
    hipLaunchKernelGGL(k_cp_scan64, dim3(l.n2), block, 0, st, (unsigned long long*)s1, l.n1, (const uint32_t*)nullptr,
                       (unsigned long long*)s2);
    hipLaunchKernelGGL(k_cp_scan64, dim3(l.n3), block, 0, st, (unsigned long long*)s2, l.n2, (const uint32_t*)nullptr,
                       (unsigned long long*)s3);
    hipLaunchKernelGGL(k_cp_scan64, dim3(1), block, 0, st, (unsigned long long*)s3, l.n3, (const uint32_t*)nullptr,
                       (unsigned long long*)stot);  // n3 <= 64
    hipLaunchKernelGGL(k_cp_edges, grid, block, 0, st, ord, (const uint32_t*)p_file, (const uint64_t*)p_holder,
                       (const uint64_t*)run, (const uint64_t*)s1, (const uint64_t*)s2, (const uint64_t*)s3,
                       (const uint64_t*)stot, (const uint8_t*)head, (const uint32_t*)h1, h2, h3, (const uint32_t*)np,
                       cap, e_file, e_holder, e_beg, e_end);
    if ((e = hipGetLastError())) return e;
    hipLaunchKernelGGL(k_cp_edge_init, grid, block, 0, st, e_beg, (const uint64_t*)e_end, (const uint32_t*)ne, cap,
                       ord_a);
    const uint32_t* eord = cp_sort(ord_a, ord_b, CpEdgeLess{e_file, e_beg, e_holder}, cap, ne, st);
    hipLaunchKernelGGL(k_cp_write, grid, block, 0, st, eord, (const uint32_t*)e_file, (const uint64_t*)e_holder,
                       (const uint64_t*)e_beg, (const uint32_t*)ne, cap, in.n_files, in.k, out, sc);
    if ((e = hipGetLastError())) return e;
  }
  if (counts) {
    hipLaunchKernelGGL(k_cp_totals, dim3(1), dim3(64), 0, st, (const unsigned long long*)sc, (const uint32_t*)np,
                       (const uint32_t*)ne, cap, in.n_files, cts);
    if ((e = hipGetLastError())) return e;
    return hipMemcpyAsync(counts, cts, kPeersCounts * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  }
  return hipSuccess;
}

}  // namespace sdcas
