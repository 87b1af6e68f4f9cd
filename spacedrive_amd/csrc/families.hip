// families.hip — the file families: the connected components of the graph
// whose edges are the peer rows that pass a shared-bytes threshold
// (include/sdcas.h has the definition; families.h the workspace). A graph
// problem and not a sort: a lock-free union-find over u32 row indices.
//   k_ff_init   parent[i] = i, size[i] = 0; ids[i] < ids[i + 1] or `unsorted`
//   k_ff_union  one row per thread, its at most k slots: the peer's row by one
//               halving in ids, the slot's class counted, a link united (a
//               wave's rows that link one row: with each other, one with it)
//   k_ff_jump   parent[i] = parent[parent[i]], ceil_log2(n) launches; a pass
//               that moved nothing tells the next ones to leave
//   k_ff_sizes  size[parent[i]] += 1, family[i] = parent[i]
//   k_ff_write  family_size[i] = size[parent[i]]; the roots with two rows or
//               more counted, one atomic per workgroup and count
//   k_ff_totals the counts
// With `unsorted` set the later kernels write the trivial rows and nothing else.
//
// The per-XCD L2s are not coherent with each other and a CU's L1 is never
// refreshed by another CU's stores, so inside k_ff_union EVERY access to
// parent[] is a relaxed agent-scope atomic (load, store, compare-and-swap):
// they are served past the L1, and a value they return was stored by some
// thread. They may still return an OLD value. Three invariants make that
// correct and keep the kernel from hanging:
//   (a) Termination. parent[x] <= x always, and parent[x] < x unless x is a
//       root: k_ff_init stores x, a hook stores a smaller row under the larger
//       root, a halving stores an ancestor, and an ancestor is smaller. A
//       descent (ff_unite's find) therefore strictly falls and ends within x
//       steps whatever stale value it reads: a stale parent is still an
//       ancestor.
//   (b) Progress. The only writes that change a root are successful
//       compare-and-swaps, at most n - 1 of them, and a failed one means that
//       another thread's succeeded (the word no longer held the root).
//   (c) No waiting. No thread ever waits for a value another thread has yet to
//       write: no spin, no lock, no flag.
// From (a) the one root of a component is its lowest index, so the result does
// not depend on scheduling. Kernel boundaries make every kernel's writes
// visible to the next: k_ff_jump's passes, k_ff_sizes and k_ff_write read what
// the launch before them wrote.
//
// The one loop whose length follows the data is that descent: it follows the
// depth of the forest at that moment, which halving and the hook direction
// keep short; no bound better than x is known.
#include <hip/hip_runtime.h>

#include "families.h"
#include "wg_scan.h"

namespace sdcas {

namespace {

constexpr uint32_t kTB = kFamiliesTB;
enum { kScSlots, kScMissing, kScSelf, kScWeak, kScLinks, kScFamilies, kScMembers, kScLargest, kScWords };
static_assert(kScWords == 8, "families_layout's sc");

__device__ __forceinline__ uint32_t ff_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ff_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The two rows' trees made one. The LARGER of the two rows descends towards its
// root, halving its path on the way (any ancestor is a valid parent); when it
// is a root it is hooked, by one compare-and-swap, under the smaller row. That
// row need not be a root: a root is the lowest row of its tree, so a row below
// it lies in another tree, the hook closes no cycle, and the joined tree's root
// is the other tree's, again its lowest row. A failed swap returns parent[a],
// an ancestor below a, and the descent goes on from there. max(a, b) falls
// with every step, so the loop ends within max(i, j) steps whatever it reads.
__device__ __forceinline__ void ff_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  while (a != b) {
    if (a < b) {
      const uint32_t t = a;
      a = b, b = t;
    }
    const uint32_t p = ff_load(parent + a);
    if (p == a) {
      uint32_t seen = a;
      if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        return;
      a = seen;
    } else {
      const uint32_t g = ff_load(parent + p);
      if (g != p) ff_store(parent + a, g);  // g < p < a
      a = g;
    }
  }
}

// b * den >= num * m, exactly: the products reach 2^96
__device__ __forceinline__ bool ff_passes(uint64_t b, uint32_t den, uint32_t num, uint64_t m) {
  const uint64_t lh = __umul64hi(b, (uint64_t)den), ll = b * den;
  const uint64_t rh = __umul64hi(m, (uint64_t)num), rl = m * num;
  return lh != rh ? lh > rh : ll >= rl;
}

__global__ void __launch_bounds__(kTB) k_ff_init(const uint64_t* __restrict__ ids, uint32_t n,
                                                 uint32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                 uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  if (i >= n) return;
  parent[i] = i, size[i] = 0;
  if (i + 1 < n && !(ids[i] < ids[i + 1])) atomicOr(&flags[0], 1u);
}

__global__ void __launch_bounds__(kTB) k_ff_union(FamiliesIn in, uint32_t* parent, const uint32_t* __restrict__ flags,
                                                  unsigned long long* __restrict__ sc) {
  __shared__ unsigned long long s_sum[5];  // slots, missing, self, weak, links
  if (flags[0]) return;  // the whole grid alike
  if (threadIdx.x < 5) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kTB + threadIdx.x, lane = threadIdx.x & 63;
  const bool on = i < in.n;
  const uint32_t cnt = !on ? 0u : in.peer_count[i] < in.k ? in.peer_count[i] : in.k;
  const uint64_t own = on ? in.ids[i] : 0ull, si = on ? in.sizes[i] : 0ull;
  uint32_t c_missing = 0, c_self = 0, c_weak = 0, c_links = 0;
  for (uint32_t s = 0; s < in.k; ++s) {
    const bool read = s < cnt;
    if (!__ballot(read)) break;  // the whole wave alike: no row of it has a slot s or beyond
    bool link = false;
    uint32_t j = 0;
    if (read) {
      const size_t at = (size_t)i * in.k + s;
      const uint64_t f = in.peers[at], b = in.peer_bytes[at];
      uint32_t lo = 0, hi = in.n;
      while (lo < hi) {  // the first row whose id is not below f
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (in.ids[mid] < f) lo = mid + 1;
        else hi = mid;
      }
      j = lo;
      if (j >= in.n || in.ids[j] != f) {
        ++c_missing;
      } else if (f == own) {
        ++c_self;
      } else {
        const uint64_t sj = in.sizes[j];
        link = b && ff_passes(b, in.den, in.num, si > sj ? si : sj);
        if (link) ++c_links;
        else ++c_weak;
      }
    }
    // The wave's rows that link the same row as its first linking row are
    // united with THAT row instead, which is united with the target: the same
    // component, and a row that everybody lists (a star) is approached by one
    // lane of a wave, not by 64.
    const unsigned long long links = __ballot(link);
    if (links) {
      const uint32_t lead = (uint32_t)__ffsll((long long)links) - 1;
      const uint32_t lj = __shfl(j, lead), li = __shfl(i, lead);
      if (link) ff_unite(parent, i, lane != lead && j == lj ? li : j);
    }
  }
  if (cnt) atomicAdd(&s_sum[0], (unsigned long long)cnt);
  if (c_missing) atomicAdd(&s_sum[1], (unsigned long long)c_missing);
  if (c_self) atomicAdd(&s_sum[2], (unsigned long long)c_self);
  if (c_weak) atomicAdd(&s_sum[3], (unsigned long long)c_weak);
  if (c_links) atomicAdd(&s_sum[4], (unsigned long long)c_links);
  __syncthreads();
  if (threadIdx.x < 5 && s_sum[threadIdx.x]) atomicAdd(&sc[kScSlots + threadIdx.x], s_sum[threadIdx.x]);
}

// Pass p. A row reads its parent's parent while that parent's own thread may
// be storing it: either value is an ancestor at least as high as the one
// before the pass, so the depth at least halves.
__global__ void __launch_bounds__(kTB) k_ff_jump(uint32_t* parent, uint32_t n, uint32_t* __restrict__ flags,
                                                 uint32_t pass) {
  if (flags[0] || (pass && !flags[pass])) return;  // flags[1 + (pass - 1)]: the pass before moved nothing
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  bool moved = false;
  if (i < n) {
    const uint32_t p = ff_load(parent + i);
    const uint32_t g = ff_load(parent + p);
    if (g != p) {
      ff_store(parent + i, g);
      moved = true;
    }
  }
  if (__syncthreads_or(moved) && threadIdx.x == 0) flags[1 + pass] = 1u;
}

__global__ void __launch_bounds__(kTB) k_ff_sizes(const uint32_t* __restrict__ parent, uint32_t n,
                                                  const uint32_t* __restrict__ flags, uint32_t* __restrict__ size,
                                                  int64_t* __restrict__ family) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  const bool on = i < n;
  if (flags[0]) {
    if (on && family) family[i] = (int64_t)i;
    return;
  }
  const uint32_t r = on ? parent[i] : 0u;
  // the rows of one wave that share its first row's root add once: a family of
  // everything is one add per wave, not 64 to one word
  const unsigned long long live = __ballot(on);
  if (live) {
    const uint32_t lead = (uint32_t)__ffsll((long long)live) - 1;
    const uint32_t lr = __shfl(r, lead);
    const unsigned long long same = __ballot(on && r == lr);
    if ((threadIdx.x & 63) == lead) atomicAdd(&size[lr], (uint32_t)__popcll(same));
    else if (on && r != lr) atomicAdd(&size[r], 1u);
  }
  if (on && family) family[i] = (int64_t)r;
}

__global__ void __launch_bounds__(kTB) k_ff_write(const uint32_t* __restrict__ parent, uint32_t n,
                                                  const uint32_t* __restrict__ flags,
                                                  const uint32_t* __restrict__ size,
                                                  uint32_t* __restrict__ family_size,
                                                  unsigned long long* __restrict__ sc) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  if (flags[0]) {
    if (i < n && family_size) family_size[i] = 1u;
    return;
  }
  unsigned long long fam = 0, mem = 0, big = 0;
  if (i < n) {
    const uint32_t r = parent[i];
    const uint32_t sz = size[r];
    if (family_size) family_size[i] = sz;
    if (r == i && sz >= 2) fam = 1, mem = sz, big = sz;
  }
  wg_reduce_sum2_max(fam, mem, big);
  if (threadIdx.x == 0 && fam) {
    atomicAdd(&sc[kScFamilies], fam);
    atomicAdd(&sc[kScMembers], mem);
    atomicMax(&sc[kScLargest], big);
  }
}

// files, slots, missing, self_slots, weak, links, families, members, largest, unsorted
__global__ void k_ff_totals(const unsigned long long* __restrict__ sc, const uint32_t* __restrict__ flags, uint32_t n,
                            unsigned long long* __restrict__ counts) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    counts[0] = n;
    for (uint32_t w = 0; w < kScWords; ++w) counts[1 + w] = sc[w];
    counts[9] = flags[0] ? 1ull : 0ull;
  }
}

}  // namespace

hipError_t file_families(uint8_t* ws, const FamiliesIn& in, int64_t* family, uint32_t* family_size,
                         unsigned long long* counts, hipStream_t st) {
  static_assert(kFamiliesCounts == 2 + kScWords, "files, sc, unsorted");
  const FamiliesLayout l = families_layout(in.n);
  uint32_t* parent = index_at<uint32_t>(ws, l.parent);
  uint32_t* size = index_at<uint32_t>(ws, l.size);
  uint32_t* flags = index_at<uint32_t>(ws, l.flags);
  unsigned long long* sc = index_at<unsigned long long>(ws, l.sc);
  const uint32_t n = in.n;
  hipError_t e;
  if ((e = hipMemsetAsync(flags, 0, l.bytes - l.flags, st))) return e;  // flags and sc
  if (n) {
    const dim3 block(kTB), grid((n + kTB - 1) / kTB);
    hipLaunchKernelGGL(k_ff_init, grid, block, 0, st, in.ids, n, parent, size, flags);
    hipLaunchKernelGGL(k_ff_union, grid, block, 0, st, in, parent, (const uint32_t*)flags, sc);
    if ((e = hipGetLastError())) return e;
    const uint32_t passes = families_passes(n);  // <= kFamiliesMaxPasses: flags[1 + pass] stays inside
    for (uint32_t p = 0; p < passes; ++p) hipLaunchKernelGGL(k_ff_jump, grid, block, 0, st, parent, n, flags, p);
    hipLaunchKernelGGL(k_ff_sizes, grid, block, 0, st, (const uint32_t*)parent, n, (const uint32_t*)flags, size,
                       family);
    hipLaunchKernelGGL(k_ff_write, grid, block, 0, st, (const uint32_t*)parent, n, (const uint32_t*)flags,
                       (const uint32_t*)size, family_size, sc);
    if ((e = hipGetLastError())) return e;
  }
  if (counts) {
    hipLaunchKernelGGL(k_ff_totals, dim3(1), dim3(64), 0, st, (const unsigned long long*)sc, (const uint32_t*)flags, n,
                       counts);
    if ((e = hipGetLastError())) return e;
  }
  return hipSuccess;
}

}  // namespace sdcas
