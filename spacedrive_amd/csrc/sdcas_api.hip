// sdcas_api.hip — the C ABI of include/sdcas.h: context, staging, file I/O
// and the batch calls that sd-core's Rust host binds.
//
// Host work here is exactly what the reference does around the hash
// (core/src/object/cas.rs:23-62, core/src/object/validation/hash.rs:11-25):
// the same reads at the same offsets, with the same error kinds — but into a
// pinned staging buffer laid out as device messages, after which one H2D
// copy and one kernel sequence hash the whole batch. There is no CPU hashing
// path: every digest this library returns comes from the HIP kernels.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <chrono>
#include <memory>
#include <vector>

#include "../../include/sdcas.h"
#include "../../include/sdcas_bench.h"
#include "../host/cas_io.hpp"
#include "b3_batch.h"
#include "confirm.h"
#include "dupsets.h"
#include "dirtree.h"
#include "cdc.h"
#include "chunk_holders.h"
#include "chunk_peers.h"
#include "families.h"
#include "family_bytes.h"
#include "family_recipes.h"
#include "family_forget.h"
#include "family_store.h"
#include "chunk_index.h"
#include "dist_dedup.h"
#include "synth.h"

using namespace sdcas;

namespace {

// file I/O with the reference's read pattern (GPU-free, in
// spacedrive_amd/host/cas_io.cpp: tested under ASan / UBSan / TSan by
// tests/cpp/test_cas_io.cpp)
using sdcas_io::open_for_read;
using sdcas_io::plan_batch;
using sdcas_io::pread_direct;
using sdcas_io::pread_exact;
using sdcas_io::read_cas_message;
using sdcas_io::read_whole;
using sdcas_io::read_whole_any;

constexpr uint64_t kMin = SDCAS_MINIMUM_FILE_SIZE;  // cas.rs:15 (the reads themselves: host/cas_io.cpp)
constexpr uint64_t kSlack = 64;  // readable bytes kept after every message

// staged messages start on 128-byte (L2/HBM line) boundaries
inline uint64_t align16(uint64_t x) { return sdcas_io::align_line(x); }
inline uint64_t chunks_of(uint64_t len) { return len == 0 ? 1 : (len + 1023) / 1024; }

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max<size_t>(n, 16);
    hipError_t e = hipMalloc(&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// One pinned staging slot: message bytes, per-message metadata and results,
// their device twins, and the event that fences the slot's GPU work.
struct Slot {
  uint8_t* h = nullptr;   // pinned message bytes
  size_t h_cap = 0;
  bool h_mapped = false;  // h is an mmap'd, hipHostRegister'ed range (SDCAS_STAGING_THP)
  uint64_t* hm = nullptr;  // pinned: offs[cap_n] | lens[cap_n] | results (32 B per message)
  size_t cap_n = 0;
  DevBuf<uint8_t> d_blob;
  DevBuf<uint64_t> d_meta;  // offs | lens (or piece descriptors)
  DevBuf<uint8_t> d_res;
  hipEvent_t ev = nullptr;
  hipEvent_t h2d = nullptr;  // the slot's uploads done (on the copy stream)
  bool busy = false, res32 = false;
  size_t n = 0;
  uint64_t used = 0, chunks = 0;
  uint64_t content = 0;  // input bytes whose results this slot's batch makes final (progress)
  std::vector<size_t> idx;  // caller index of message k
  const uint8_t* src = nullptr;  // message bytes DMA'd from here instead of h (a pinned caller buffer)
  bool blob_uploaded = false;    // the bytes went up in parts while the slot was being read (slot_submit skips them)
  uint64_t* offs() { return hm; }
  uint64_t* lens() { return hm + cap_n; }
  uint8_t* res() { return reinterpret_cast<uint8_t*>(hm + 2 * cap_n); }
};

// Small host arrays (the device stream's message and segment descriptors)
// sent to the device in stream order without a host wait: each put copies
// into the next of kN page-locked buffers and enqueues the upload from it; a
// buffer is reused only after the event recorded behind its last upload.
struct HostStage {
  static constexpr int kN = 4;
  uint8_t* h[kN] = {};
  size_t cap[kN] = {};
  hipEvent_t ev[kN] = {};
  bool recorded[kN] = {};
  int next = 0;
  HostStage() = default;
  HostStage(const HostStage&) = delete;
  HostStage& operator=(const HostStage&) = delete;
  ~HostStage() { release(); }
  // the next buffer, free and of at least `bytes` bytes, for a caller that
  // builds its array in place; send() uploads it
  hipError_t reserve(size_t bytes, uint8_t** out) {
    const int i = next;
    hipError_t e;
    if (recorded[i] && (e = hipEventSynchronize(ev[i]))) return e;
    recorded[i] = false;
    if (bytes > cap[i]) {
      if (h[i]) (void)hipHostFree(h[i]);
      h[i] = nullptr;
      cap[i] = 0;
      const size_t want = std::max<size_t>(bytes + bytes / 4, 64 << 10);
      if ((e = hipHostMalloc(&h[i], want, hipHostMallocDefault))) return e;
      cap[i] = want;
    }
    if (!ev[i] && (e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming))) return e;
    *out = h[i];
    return hipSuccess;
  }
  // the reserved buffer's first `bytes` bytes to d_dst in stream order
  hipError_t send(size_t bytes, void* d_dst, hipStream_t st) {
    const int i = next;
    next = (next + 1) % kN;
    hipError_t e;
    if ((e = hipMemcpyAsync(d_dst, h[i], bytes, hipMemcpyHostToDevice, st))) return e;
    if ((e = hipEventRecord(ev[i], st))) return e;
    recorded[i] = true;
    return hipSuccess;
  }
  hipError_t put(const void* src, size_t bytes, void* d_dst, hipStream_t st) {
    if (!bytes) return hipSuccess;
    uint8_t* buf = nullptr;
    if (hipError_t e = reserve(bytes, &buf)) return e;
    memcpy(buf, src, bytes);
    return send(bytes, d_dst, st);
  }
  void release() {
    for (int i = 0; i < kN; ++i) {
      if (recorded[i]) (void)hipEventSynchronize(ev[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      if (h[i]) (void)hipHostFree(h[i]);
      h[i] = nullptr, ev[i] = nullptr, cap[i] = 0, recorded[i] = false;
    }
  }
};

}  // namespace

struct sdcas_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // staging slots' host-to-device copies
  std::string err;
  std::mutex mu;
  // reader threads: 16 unless the machine has fewer CPUs (C-ABI probe, C2
  // files from the page cache, profiles/r02_latency_threads.json: 16 against
  // 8 cut 100 / 1000 / 10000-file calls by 8 / 17 / 18 %; 32 no better)
  uint32_t io_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  static constexpr uint32_t kMaxIoThreads = 256;
  std::unique_ptr<sdcas_io::WorkerPool> pool;  // io_threads readers (the calling thread is one)
  uint64_t staging_bytes = 256ull << 20;
  bool direct_io = false;  // SDCAS_OPT_DIRECT_IO: big-file checksum reads bypass the page cache

  BatchWorkspace ws;
  DevBuf<uint64_t> ws_S, ws_total, ws_soffs, ws_slens;
  DevBuf<uint32_t> ws_tile_first, ws_nodes, ws_perm, ws_sort_keys;
  DevBuf<uint8_t> ws_scan;

  // host-API device buffers
  DevBuf<uint8_t> d_out32;
  DevBuf<FileDesc> d_files;
  DevBuf<uint32_t> d_file_nodes;
  Slot slots[2];  // double-buffered pinned staging (host fills one, GPU hashes the other)
  DevBuf<uint8_t> id_scratch;  // sdcas_dev_identify / sdcas_identify_checksums: the dual plans and the gathered cas messages

  // The device copies of the host arrays of every host-array entry point
  // (sdcas_dedup_window ... sdcas_chunk_holders_remove; laid out by Parts).
  // One buffer serves them all: each such call holds the context's mutex,
  // runs on the context's own stream and returns only after waiting for that
  // stream (after an error return the next call is still ordered behind it
  // there), so no two of them ever use the buffer at once.
  DevBuf<uint8_t> host_io;

  // the dedup's ordinals (sdcas_dedup_window, sdcas_dev_dedup)
  DevBuf<uint64_t> dd_ids;

  // the workspaces of the (cas key, checksum) group-by (confirm.hip) and of
  // the duplicate sets (dupsets.hip)
  DevBuf<uint32_t> cf_ws, ds_ws;

  // directory digests and top-most duplicates (dirtree.hip): the workspaces
  // and the shape's upload
  DevBuf<uint8_t> tr_ws;
  HostStage tr_stage;
  DevBuf<uint32_t> tt_ws;

  // content-defined chunks and their sharing (cdc.hip): the workspaces, the
  // packed chunks of one hash batch and the packed offsets' upload
  DevBuf<uint8_t> cd_ws, cd_pack, cs_ws;
  HostStage cd_stage;

  // the chunk index (chunk_index.hip): the add's workspace
  DevBuf<uint8_t> ci_ws;
  // the holders index (chunk_holders.hip): the add's and the remove's workspace
  DevBuf<uint8_t> ch_ws;
  // the chunk peers (chunk_peers.hip): the runs, the expansion and the edges
  DevBuf<uint8_t> cp_ws;
  // the file families (families.hip): the forest, the sizes, the flags and the sums
  DevBuf<uint8_t> ff_ws;
  // the family bytes (family_bytes.hip): the class table, the row and label sums, the order
  DevBuf<uint8_t> fb_ws;
  // the family recipes (family_recipes.hip): the class table, the chunks' sources and ops
  DevBuf<uint8_t> fr_ws;
  // the family store (family_store.hip): the op sums, tile starts and clipped ranges
  DevBuf<uint8_t> fs_ws;
  // a family store that forgets rows (family_forget.hip): the tables, new numbers and move heads
  DevBuf<uint8_t> fg_ws;

  // multi-GPU dedup stages
  DistWs dist;

  // device-resident big-message stream (sdcas_dev_stream_*)
  std::vector<FileDesc> sm_files;
  DevBuf<FileDesc> sm_d_files;
  DevBuf<uint32_t> sm_nodes;
  DevBuf<PieceDesc> sm_pieces;
  DevBuf<SegDesc> sm_segs;
  HostStage sm_stage;             // descriptor uploads without a host wait
  bool sm_active = false;
  bool sm_begin_pending = false;  // stream_begin's descriptor upload and node-list clear, enqueued by the next call
  uint64_t sm_node_bytes = 0;
  DevBuf<uint32_t> piece_ctr;  // the persistent piece kernels' work counter
  DevBuf<uint32_t> piece_l4;   // piece variant 19's level-4 nodes (kPieceL4Words per piece)
  int piece_variant = -1;

  // Every call that enqueues work on the context's device scratch (the
  // workspaces above) may name its own stream. The scratch is shared, so a
  // call first makes its stream wait for the previous call's work (the event
  // recorded at the end of that call), then records the event anew: calls on
  // one context are ordered on the device as they are on the host, whatever
  // streams they name.
  hipEvent_t scratch_ev = nullptr;
  hipStream_t scratch_st = nullptr;
  bool scratch_pending = false;
  // sdcas_dev_bind_stream: streams whose identity the caller named
  std::vector<std::pair<hipStream_t, uint64_t>> bound;
  uint64_t scratch_token = 0;  // the token of the stream the last call used (0: none)
  bool scratch_recorded = true;  // scratch_ev marks the last call's end (else: record it first)
  uint64_t token_of(hipStream_t st) const {
    for (const auto& b : bound)
      if (b.first == st) return b.second;
    return 0;
  }
  uint32_t upload_parts = 4;  // sdcas_cas_ids: a lone slot's reads and upload overlapped in this many parts (0/1: off)
  bool plan_small = true;      // small batches planned on the host (SDCAS_PLAN_SMALL=0: on the device)
  bool small_direct = true;    // such a batch: metadata behind its bytes, results written to pinned memory (slot_submit)

  // progress / cancellation of the path APIs (sdcas_options, sdcas_set_progress)
  sdcas_progress_fn progress = nullptr;
  void* progress_user = nullptr;
  const volatile int32_t* cancel = nullptr;

  // profiling
  bool profile = false;
  std::vector<hipEvent_t> ev_free;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_leaf, ev_all;

  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
  int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? SDCAS_E_OOM : SDCAS_E_HIP, "%s: %s", what, hipGetErrorString(e));
  }
  // before enqueuing on st: wait for the previous call's use of the scratch
  // — unless it ran on this same stream, which only a bound token can tell
  // (a handle value may have been reused by a new stream after the caller
  // destroyed the old one)
  hipError_t fence_in(hipStream_t st) {
    if (!scratch_pending) return hipSuccess;
    if (st == scratch_st && scratch_token && token_of(st) == scratch_token) return hipSuccess;
    hipError_t e = scratch_event();
    return e ? e : hipStreamWaitEvent(st, scratch_ev, 0);
  }
  // after enqueuing on st. On a bound stream the event is recorded only when
  // something needs it — a call on another stream, a host wait for the
  // scratch — and then on that stream, behind everything enqueued on it so
  // far: a recorded event is a barrier packet that idled the GPU ~6-8 us
  // between two calls on the step's stream (the C5 step's kernel trace)
  hipError_t fence_out(hipStream_t st) {
    scratch_st = st;
    scratch_token = token_of(st);
    scratch_pending = true;
    scratch_recorded = false;
    return scratch_token ? hipSuccess : scratch_event();
  }
  // the scratch event, recorded on the last call's stream if it was not yet
  hipError_t scratch_event() {
    if (scratch_recorded) return hipSuccess;
    hipError_t e = hipSuccess;
    if (!scratch_ev && (e = hipEventCreateWithFlags(&scratch_ev, hipEventDisableTiming))) return e;
    if ((e = hipEventRecord(scratch_ev, scratch_st))) return e;
    scratch_recorded = true;
    return hipSuccess;
  }
  // the host waits until no enqueued call still uses the scratch
  hipError_t scratch_sync() {
    if (!scratch_pending) return hipSuccess;
    hipError_t e = scratch_event();
    return e ? e : hipEventSynchronize(scratch_ev);
  }
  bool cancelled() const { return cancel && __atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0; }
  void report(uint64_t done, uint64_t total) {
    if (progress) progress(progress_user, done, total);
  }
  hipEvent_t event() {
    if (!ev_free.empty()) {
      hipEvent_t e = ev_free.back();
      ev_free.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
};

namespace {

// A workspace grown to `need` elements for a call on st. The host waits first
// for the scratch and for st, as an earlier call's kernels may still use the
// buffer about to be freed; a buffer that is large enough costs nothing.
template <class T>
int grow_synced(sdcas_ctx* c, DevBuf<T>& buf, size_t need, hipStream_t st, const char* what) {
  if (need <= buf.cap) return SDCAS_OK;
  hipError_t e = c->scratch_sync();
  if (!e) e = hipStreamSynchronize(st);
  if (!e) e = buf.ensure(need);
  return e ? c->hip_fail(e, what) : SDCAS_OK;
}

// a HIP error of entry point `who` at `step` ("", " H2D", ...)
int hip_fail_at(sdcas_ctx* c, hipError_t e, const char* who, const char* step) {
  return c->hip_fail(e, (std::string(who) + step).c_str());
}

// The arrays of one host-array call `who` on stream st. Each is declared once,
// with its host pointer and its element count, and becomes a 16-byte aligned
// part of the context's host_io; the part converts to its typed device
// pointer there (from reserve() on). A part whose host pointer is null is
// off: it takes no room, its device pointer is null and nothing is copied for
// it. A part of no elements is copied neither.
struct Parts {
  struct Item {
    const void* up;  // uploaded from here (null: not)
    void* down;      // downloaded to here (null: not)
    size_t off, bytes, down_bytes;
    bool on;
  };
  template <class T>
  struct Part {
    Parts* p;
    size_t i;
    operator T*() const {
      const Item& x = p->items[i];
      return x.on ? reinterpret_cast<T*>(p->c->host_io.p + x.off) : nullptr;
    }
    template <class U>
    U* as() const {
      return reinterpret_cast<U*>(static_cast<T*>(*this));
    }
    // only the first k elements come down (k within the declared count: the caller checks)
    void first(size_t k) const { p->items[i].down_bytes = k * sizeof(T); }
  };
  sdcas_ctx* c;
  hipStream_t st;
  const char* who;
  std::vector<Item> items;
  size_t o = 0;
  Parts(sdcas_ctx* cc, hipStream_t s, const char* w) : c(cc), st(s), who(w) { items.reserve(16); }

  template <class T>
  Part<T> take(const void* up, void* down, size_t n, bool on) {
    const size_t bytes = n * sizeof(T);
    items.push_back(Item{on ? up : nullptr, on ? down : nullptr, o, bytes, bytes, on});
    if (on) o += (bytes + 15) & ~(size_t)15;
    return Part<T>{this, items.size() - 1};
  }
  template <class T>
  Part<const T> in(const T* h, size_t n) {
    return take<const T>(h, nullptr, n, h != nullptr);
  }
  // keep: the device array is there (the kernels write it) whether or not the caller asks for it
  template <class T>
  Part<T> out(T* h, size_t n, bool keep = false) {
    return take<T>(nullptr, h, n, keep || h != nullptr);
  }
  template <class T>
  Part<T> inout(T* h, size_t n) {
    return take<T>(h, h, n, h != nullptr);
  }
  // a device array of the call that no host array stands behind
  template <class T>
  Part<T> room(size_t n) {
    return take<T>(nullptr, nullptr, n, true);
  }

  // host_io grown to the sum of the parts (the host waits only when it must be reallocated)
  int reserve() { return grow_synced(c, c->host_io, o, st, (std::string(who) + " buffers").c_str()); }
  int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* step) {
    if (!bytes) return SDCAS_OK;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
    return e ? hip_fail_at(c, e, who, step) : SDCAS_OK;
  }
  int sync(const char* step = " sync") {
    const hipError_t e = hipStreamSynchronize(st);
    return e ? hip_fail_at(c, e, who, step) : SDCAS_OK;
  }
  // every input up
  int upload() {
    for (const Item& x : items)
      if (x.up)
        if (int rc = copy(c->host_io.p + x.off, x.up, x.bytes, hipMemcpyHostToDevice, " H2D")) return rc;
    return SDCAS_OK;
  }
  // The counts down on their own, and the wait for them: they say how many
  // entries of the other outputs follow. The caller checks their range and
  // names the prefixes (Part::first); download() fetches the rest.
  template <class T>
  int counts(const Part<T>& part) {
    Item& x = items[part.i];
    if (int rc = copy(x.down, c->host_io.p + x.off, x.down_bytes, hipMemcpyDeviceToHost, " counts")) return rc;
    x.down = nullptr;
    return sync(" counts");
  }
  // a device array that is no part of the call, down with the outputs
  template <class T>
  int fetch(T* dst, const void* d_src, size_t n) {
    return copy(dst, d_src, n * sizeof(T), hipMemcpyDeviceToHost, " D2H");
  }
  // every output down, and the call's final wait
  int download() {
    for (const Item& x : items)
      if (x.down)
        if (int rc = copy(x.down, c->host_io.p + x.off, x.down_bytes, hipMemcpyDeviceToHost, " D2H")) return rc;
    return sync();
  }
};

int reserve_ws(sdcas_ctx* c, size_t max_msgs, uint64_t max_chunks) {
  hipError_t e;
  // a batch's message count is an int all the way down
  if (max_msgs > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "batch of %zu messages exceeds 2^31 - 1", max_msgs);
  if ((e = c->ws_S.ensure(max_msgs + 1))) return c->hip_fail(e, "workspace S");
  // 3 slots per message (of as many as the workspace takes) and 8 more are
  // padding no kernel fills since the quad slot layout went; they stay,
  // because the capacities callers see derive from them
  // (rounded up, +3: cap_chunks below comes out >= max_chunks, so that
  // slots_prepare's check holds on the next call instead of re-reserving)
  const uint64_t tiles = (max_chunks + 3 * (uint64_t)(c->ws_S.cap - 1) + 8 + kTile - 1) / kTile + 3;
  // tile_first also serves the small-batch kernel's tiles (kSmallTile slots)
  const uint64_t small_tiles = (std::min<uint64_t>(max_chunks, kSmallSlots) + kSmallTile - 1) / kSmallTile + 3;
  if ((e = c->ws_total.ensure(4))) return c->hip_fail(e, "workspace total");
  if ((e = c->ws_tile_first.ensure(std::max<uint64_t>(tiles, small_tiles))))
    return c->hip_fail(e, "workspace tile_first");
  if ((e = c->ws_nodes.ensure(8 * (tiles * kTile)))) return c->hip_fail(e, "workspace nodes");
  size_t tb = batch_scan_temp_bytes((uint32_t)std::max<size_t>(max_msgs, 1));
  if ((e = c->ws_scan.ensure(tb))) return c->hip_fail(e, "workspace scan");
  if ((e = c->ws_perm.ensure(max_msgs + 1)) || (e = c->ws_soffs.ensure(max_msgs + 1)) ||
      (e = c->ws_slens.ensure(max_msgs + 1)) || (e = c->ws_sort_keys.ensure(sort_key_words(max_msgs + 1))))
    return c->hip_fail(e, "workspace sort");
  c->ws.S = c->ws_S.p;
  c->ws.total = c->ws_total.p;
  c->ws.tile_first = c->ws_tile_first.p;
  c->ws.nodes = c->ws_nodes.p;
  c->ws.scan_tmp = c->ws_scan.p;
  c->ws.scan_tmp_bytes = c->ws_scan.cap;
  c->ws.perm = c->ws_perm.p;
  c->ws.soffs = c->ws_soffs.p;
  c->ws.slens = c->ws_slens.p;
  c->ws.cap_msgs =
      (uint32_t)std::min<size_t>({c->ws_S.cap - 1, c->ws_perm.cap - 1, c->ws_soffs.cap - 1, c->ws_slens.cap - 1});
  c->ws.sort_keys = c->ws_sort_keys.p;
  // every tile the leaf kernel may touch needs a tile_first entry and its node slots
  c->ws.cap_slots = std::min<uint64_t>((c->ws_tile_first.cap - 1) * kTile, c->ws_nodes.cap / 8 - 2 * kTile);
  c->ws.cap_small_tiles = c->ws_tile_first.cap;
  const uint64_t pad = 3 * (uint64_t)(c->ws_S.cap - 1) + 8;
  c->ws.cap_chunks = c->ws.cap_slots > pad ? c->ws.cap_slots - pad : 0;
  return SDCAS_OK;
}

// Enqueue the hash of n device messages (the one launch sequence every API
// ends in), with optional HIP-event profiling of the leaf kernel.
int launch_batch(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offs, const uint64_t* lens, uint32_t n,
                 uint8_t* out32, uint64_t* keys, hipStream_t st, uint64_t max_chunks = 0,
                 const BatchPlan* plan = nullptr) {
  hipError_t e;
  if (c->profile) {
    hipEvent_t a = c->event(), b = c->event(), la = c->event(), lb = c->event();
    (void)hipEventRecord(a, st);
    e = batch_hash(c->ws, blob, offs, lens, n, out32, keys, st, max_chunks, la, lb, plan);
    (void)hipEventRecord(b, st);
    c->ev_all.push_back({a, b});
    c->ev_leaf.push_back({la, lb});
  } else {
    e = batch_hash(c->ws, blob, offs, lens, n, out32, keys, st, max_chunks, nullptr, nullptr, plan);
  }
  if (e) return c->hip_fail(e, "batch_hash");
  return SDCAS_OK;
}

// ---- double-buffered pinned staging ------------------------------------------
//
// Host work (file reads, or copies out of the caller's buffer) fills one
// pinned slot while the GPU copies and hashes the other: each slot's H2D,
// kernels and D2H are enqueued on the context stream and fenced by the slot's
// event, which is waited for only when the slot is about to be refilled.

// The message slots are anonymous mappings advised to transparent huge
// pages and then pinned (hipHostRegister): the readers' page-cache copies
// into a slot walk 2 MiB pages instead of hipHostMalloc's 4 KiB ones
// (profiles/r05_staging_thp_ab.json). A mapping or registration that fails
// falls back to hipHostMalloc; SDCAS_STAGING_THP=0 always takes it (A/B).
static bool staging_thp() {
  static const bool on = [] {
    const char* v = getenv("SDCAS_STAGING_THP");
    return !(v && strcmp(v, "0") == 0);
  }();
  return on;
}

static void free_staging(Slot& s) {
  if (!s.h) return;
  if (s.h_mapped) {
    (void)hipHostUnregister(s.h);
    munmap(s.h, s.h_cap);
  } else {
    (void)hipHostFree(s.h);
  }
  s.h = nullptr;
  s.h_cap = 0;
  s.h_mapped = false;
}

int slot_prepare(sdcas_ctx* c, Slot& s, uint64_t bytes, size_t n) {
  hipError_t e;
  if (bytes + kSlack > s.h_cap) {
    free_staging(s);
    const size_t want = bytes + kSlack;
    if (staging_thp()) {
      const size_t huge = 2u << 20, len = (want + huge - 1) / huge * huge;
      void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
      if (p != MAP_FAILED) {
        (void)madvise(p, len, MADV_HUGEPAGE);
        if (hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess) {
          s.h = static_cast<uint8_t*>(p);
          s.h_cap = len;
          s.h_mapped = true;
        } else {
          (void)hipGetLastError();  // the fallback below; not this call's error
          munmap(p, len);
        }
      }
    }
    if (!s.h) {
      if ((e = hipHostMalloc(&s.h, want, hipHostMallocDefault))) return c->hip_fail(e, "pinned staging");
      s.h_cap = want;
    }
  }
  if (n > s.cap_n) {
    if (s.hm) (void)hipHostFree(s.hm);
    s.hm = nullptr;
    s.cap_n = 0;
    const size_t want = std::max<size_t>(n, 1024);
    // offs[cap_n] | lens[cap_n] | results (32 B per message)
    if ((e = hipHostMalloc(&s.hm, 48 * want, hipHostMallocDefault))) return c->hip_fail(e, "pinned metadata");
    s.cap_n = want;
  }
  if ((e = s.d_blob.ensure(s.h_cap)) || (e = s.d_meta.ensure(2 * s.cap_n)) || (e = s.d_res.ensure(32 * s.cap_n)))
    return c->hip_fail(e, "device staging");
  if (!s.ev && (e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming))) return c->hip_fail(e, "event");
  if (!s.h2d && (e = hipEventCreateWithFlags(&s.h2d, hipEventDisableTiming))) return c->hip_fail(e, "event");
  return SDCAS_OK;
}

void slot_release(Slot& s) {
  free_staging(s);
  if (s.hm) (void)hipHostFree(s.hm);
  s.hm = nullptr;
  s.cap_n = 0;
  if (s.ev) (void)hipEventDestroy(s.ev);
  if (s.h2d) (void)hipEventDestroy(s.h2d);
  s.ev = s.h2d = nullptr;
}

// Both slots sized for `cap` staging bytes, and the kernel workspace for the
// largest batch such a slot can hold, so that no buffer is reallocated while
// the other slot's work is in flight.
int slots_prepare(sdcas_ctx* c, uint64_t cap, size_t cap_n) {
  int rc;
  for (Slot& s : c->slots)
    if ((rc = slot_prepare(c, s, cap, cap_n))) return rc;
  if (cap_n > c->ws.cap_msgs || cap / 1024 + cap_n > c->ws.cap_chunks) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e) return c->hip_fail(e, "sync");
    return reserve_ws(c, std::max<size_t>(cap_n, c->ws.cap_msgs),
                      std::max<uint64_t>(cap / 1024 + cap_n, c->ws.cap_chunks));
  }
  return SDCAS_OK;
}

// While the other slot's batch is in flight, a slot's host-to-device copies
// run on the context's copy stream, so that they overlap that batch's kernels
// on the compute stream (PCIe and the CUs work at once: the path calls are
// bound by the copy); the compute stream waits for them before this slot's
// kernels. With nothing to overlap (a call's first or only slot) they go on
// the compute stream itself: the event and the cross-stream wait would only
// add latency. Refilling a slot waits for its previous batch on the host
// first (slot_complete), so a copy never lands under kernels still reading
// the slot.
template <class Copies>
hipError_t slot_upload(sdcas_ctx* c, Slot& s, Copies copies) {
  const Slot& other = &s == &c->slots[0] ? c->slots[1] : c->slots[0];
  if (!other.busy) return copies(c->stream);
  hipError_t e;
  if ((e = copies(c->copy_stream)) || (e = hipEventRecord(s.h2d, c->copy_stream))) return e;
  return hipStreamWaitEvent(c->stream, s.h2d, 0);
}

// Enqueue the slot's batch: s.n messages at s.offs()/s.lens() in s.h (s.used
// bytes, s.chunks chunks); results land in s.res() (digests if res32, else
// cas keys) once s.ev has fired.
int slot_submit(sdcas_ctx* c, Slot& s, bool res32) {
  s.res32 = res32;
  const bool uploaded = s.blob_uploaded;  // this batch's bytes only: the flag never outlives its submit
  s.blob_uploaded = false;
  if (!s.n) return SDCAS_OK;
  int rc;
  hipStream_t st = c->stream;
  hipError_t e;
  if (s.n > c->ws.cap_msgs || s.chunks > c->ws.cap_chunks) {
    // growing the kernel workspace frees buffers the other slot's kernels may
    // still be using: drain the stream first (rare: slots are pre-reserved)
    if ((e = hipStreamSynchronize(st))) return c->hip_fail(e, "sync");
    if ((rc = reserve_ws(c, std::max<size_t>(s.n, c->ws.cap_msgs), std::max<uint64_t>(s.chunks, c->ws.cap_chunks))))
      return rc;
  }
  // offsets and lengths in one copy: the lengths are moved up behind the
  // offsets when they fit there (each small copy is a blit kernel of its own)
  const bool packed = 2 * s.n <= s.cap_n;
  if (packed) memcpy(s.hm + s.n, s.lens(), 8 * s.n);
  // A batch for the small kernel in caller order is planned here and its
  // plan goes up behind the lengths in the same copy: the plan kernels
  // and (when no message crosses a tile) k_finish_t are not launched.
  uint64_t meta_words = packed ? 2 * s.n : s.n;
  const uint64_t plan_tiles = s.chunks / kSmallTile + 2;
  const uint64_t plan_words = s.n + (plan_tiles + 1) / 2 + 4;
  const bool use_plan = c->plan_small && packed && s.n < kSortMinMsgs && s.chunks <= c->ws.small_slots &&
                        2 * s.n + plan_words <= s.cap_n;
  if (use_plan) meta_words = 2 * s.n + plan_words;
  // Round 6, a small planned batch read into the slot (the latency-bound
  // calls: a lone file of the watcher or of browse): its metadata words go up
  // behind its bytes in the SAME copy (at a 256-byte offset past them, inside
  // the slot's capacity), and the kernels write the results straight into the
  // slot's pinned result words (device-visible host memory) instead of a
  // device buffer and a download. Two copies (and their API calls) fewer;
  // the event the host waits on follows the kernels, so their writes to
  // host memory are visible when it fires. SDCAS_SMALL_DIRECT=0: off (A/B).
  const uint64_t moff = (s.used + 255) & ~uint64_t(255);
  const bool direct = c->small_direct && use_plan && !uploaded && !s.src &&
                      moff + 8 * meta_words + kSlack <= std::min<uint64_t>(s.h_cap, s.d_blob.cap);
  uint64_t* dm = direct ? reinterpret_cast<uint64_t*>(s.d_blob.p + moff) : s.d_meta.p;
  const uint64_t* d_lens = dm + (packed ? s.n : s.cap_n);
  BatchPlan plan;
  if (use_plan) {
    uint64_t* hS = s.hm + 2 * s.n;
    uint32_t* htf = reinterpret_cast<uint32_t*>(hS + s.n);
    uint64_t* htot = hS + s.n + (plan_tiles + 1) / 2;
    batch_plan_host(s.lens(), (uint32_t)s.n, kSmallTile, c->ws.cap_slots, hS, htf, htot, &plan.crossing);
    plan.S = dm + 2 * s.n;
    plan.tile_first = reinterpret_cast<const uint32_t*>(plan.S + s.n);
    plan.total = dm + 2 * s.n + s.n + (plan_tiles + 1) / 2;
    plan.tile = kSmallTile;
  }
  if (direct) memcpy(s.h + moff, s.hm, 8 * meta_words);
  if ((e = slot_upload(c, s, [&](hipStream_t cs) {
         hipError_t r;
         if (direct) return hipMemcpyAsync(s.d_blob.p, s.h, moff + 8 * meta_words, hipMemcpyHostToDevice, cs);
         if ((!uploaded && (r = hipMemcpyAsync(s.d_blob.p, s.src ? s.src : s.h, s.used, hipMemcpyHostToDevice, cs))) ||
             (r = hipMemcpyAsync(s.d_meta.p, s.hm, 8 * meta_words, hipMemcpyHostToDevice, cs)))
           return r;
         return packed ? hipSuccess
                       : hipMemcpyAsync(s.d_meta.p + s.cap_n, s.hm + s.cap_n, 8 * s.n, hipMemcpyHostToDevice, cs);
       })))
    return c->hip_fail(e, "H2D");
  uint8_t* res = direct ? s.res() : s.d_res.p;
  if ((rc = launch_batch(c, s.d_blob.p, dm, d_lens, (uint32_t)s.n, res32 ? res : nullptr,
                         res32 ? nullptr : reinterpret_cast<uint64_t*>(res), st, s.chunks,
                         use_plan ? &plan : nullptr)))
    return rc;
  if ((!direct && (e = hipMemcpyAsync(s.res(), s.d_res.p, (res32 ? 32 : 8) * s.n, hipMemcpyDeviceToHost, st))) ||
      (e = hipEventRecord(s.ev, st)))
    return c->hip_fail(e, "D2H");
  s.busy = true;
  return SDCAS_OK;
}

// Progress of one path call: bytes of input whose results are final.
struct Progress {
  sdcas_ctx* c;
  uint64_t total = 0, done = 0;
  void add(uint64_t bytes) {
    done += bytes;
    c->report(done, total);
  }
};

// Wait for the slot's batch, hand message k's result to sink(k, ptr) and
// report the slot's input bytes as done.
template <class Sink>
int slot_complete(sdcas_ctx* c, Slot& s, Sink sink, Progress* pr = nullptr) {
  if (!s.busy) return SDCAS_OK;
  s.busy = false;
  hipError_t e = hipEventSynchronize(s.ev);
  if (e) return c->hip_fail(e, "batch");
  for (size_t k = 0; k < s.n; ++k) sink(k, s.res() + (s.res32 ? 32 : 8) * k);
  if (pr) pr->add(s.content);
  return SDCAS_OK;
}

// Big messages (> 1 MiB) from host memory: 1 MiB pieces streamed through the
// two staging slots (one window filled while the GPU hashes the other). A
// window's pieces are filled by the I/O threads in parallel (several reads in
// flight: what cold storage needs, and page-cache copies scale with threads
// too); `fill(k, dst, off, len)` provides bytes [off, off+len) of item k and
// returns a status (0 ok). Pieces sit at 4 KiB-aligned window offsets (the
// O_DIRECT rule; the device needs 16 B). Digests go to
// out32_host[32 * out_index]. Cancellation is checked once per window: items
// whose every piece was submitted by then are finished, the rest get
// SDCAS_STATUS_CANCELLED and *cancelled is set.
struct BigItem {
  uint64_t len;
  uint64_t out_index;
};

inline uint64_t align_page(uint64_t x) { return (x + sdcas_io::kDirectAlign - 1) & ~(sdcas_io::kDirectAlign - 1); }

template <class Fill>
int run_big(sdcas_ctx* c, const std::vector<BigItem>& items, uint8_t* out32_host, Fill fill, int32_t* status,
            Progress& pr, bool* cancelled) {
  *cancelled = false;
  if (items.empty()) return SDCAS_OK;
  hipError_t e;
  int rc;
  const uint64_t piece_bytes = 1024ull * kTile;
  const uint64_t window = std::max<uint64_t>(piece_bytes, (c->staging_bytes / piece_bytes) * piece_bytes);
  const size_t max_pieces = (size_t)(window / piece_bytes);
  for (Slot& s : c->slots)
    if ((rc = slot_prepare(c, s, window, 2 * max_pieces))) return rc;
  std::vector<FileDesc> files(items.size());
  uint64_t nodes = 0;
  for (size_t i = 0; i < items.size(); ++i) {
    files[i].C = chunks_of(items[i].len);
    files[i].node_base = nodes;
    files[i].out_index = i;
    nodes += bigfile_node_count(files[i].C);
  }
  if ((e = c->d_file_nodes.ensure(8 * nodes + 8))) return c->hip_fail(e, "file nodes");
  if ((e = c->d_files.ensure(items.size()))) return c->hip_fail(e, "file descs");
  if ((e = c->d_out32.ensure(32 * items.size()))) return c->hip_fail(e, "device digests");
  if ((e = c->piece_ctr.ensure(1))) return c->hip_fail(e, "piece counter");
  if ((e = c->piece_l4.ensure(kPieceL4Words * 2 * max_pieces))) return c->hip_fail(e, "piece level-4 nodes");
  hipStream_t st = c->stream;
  int cur = 0;
  struct Job {
    size_t item;
    uint64_t off, dst;
    uint32_t len;
  };
  std::vector<Job> jobs;
  std::vector<int32_t> jst;
  uint64_t used = 0, content = 0;
  std::vector<int32_t> item_st(items.size(), 0);
  auto wait_slot = [&](Slot& s) -> int {
    if (!s.busy) return SDCAS_OK;
    s.busy = false;
    hipError_t ee = hipEventSynchronize(s.ev);
    if (ee) return c->hip_fail(ee, "piece window");
    pr.add(s.content);
    return SDCAS_OK;
  };
  // fill the window's pieces (in parallel), then copy and hash them
  auto flush = [&]() -> int {
    if (jobs.empty()) return SDCAS_OK;
    Slot& s = c->slots[cur];
    jst.assign(jobs.size(), 0);
    c->pool->run(jobs.size(), [&](size_t k) {
      const Job& jb = jobs[k];
      jst[k] = fill(jb.item, s.h + jb.dst, jb.off, jb.len);
    });
    PieceDesc* hp = reinterpret_cast<PieceDesc*>(s.hm);
    for (size_t k = 0; k < jobs.size(); ++k) {
      if (jst[k] && !item_st[jobs[k].item]) item_st[jobs[k].item] = jst[k];
      PieceDesc pd{};
      pd.off = jobs[k].dst;
      pd.j0 = jobs[k].off / 1024;
      pd.node_base = files[jobs[k].item].node_base;
      pd.len = jobs[k].len;
      hp[k] = pd;  // a failed item's pieces are hashed too: its digest is never returned
    }
    PieceDesc* dp = reinterpret_cast<PieceDesc*>(s.d_meta.p);
    if (kPieceL4Words * jobs.size() > c->piece_l4.cap)  // a window holds at most 2 pieces per MiB
      return c->fail(SDCAS_E_CAPACITY, "piece window: %zu pieces", jobs.size());
    hipError_t ee;
    if ((ee = slot_upload(c, s, [&](hipStream_t cs) {
           hipError_t r = hipMemcpyAsync(s.d_blob.p, s.h, used, hipMemcpyHostToDevice, cs);
           return r ? r : hipMemcpyAsync(dp, hp, sizeof(PieceDesc) * jobs.size(), hipMemcpyHostToDevice, cs);
         })))
      return c->hip_fail(ee, "H2D pieces");
    if ((ee = piece_hash(s.d_blob.p, dp, (uint32_t)jobs.size(), c->d_file_nodes.p, c->piece_ctr.p, c->piece_l4.p,
                         c->piece_variant,
                         st)))
      return c->hip_fail(ee, "piece_hash");
    if ((ee = hipEventRecord(s.ev, st))) return c->hip_fail(ee, "event");
    s.busy = true;
    s.content = content;
    cur ^= 1;
    jobs.clear();
    used = 0;
    content = 0;
    return wait_slot(c->slots[cur]);  // the next window's buffers are free again
  };
  if ((rc = wait_slot(c->slots[cur]))) return rc;
  size_t complete = items.size();  // items [0, complete) have every piece submitted
  for (size_t i = 0; i < items.size() && !*cancelled; ++i) {
    const uint64_t len = items[i].len;
    for (uint64_t off = 0; off < len && !item_st[i]; off += piece_bytes) {
      const uint32_t pl = (uint32_t)std::min<uint64_t>(piece_bytes, len - off);
      if (used + align_page(pl) > window) {
        if ((rc = flush())) return rc;
        if (c->cancelled()) {
          *cancelled = true;
          complete = i;  // item i has pieces left (or none submitted yet): not complete
          break;
        }
      }
      jobs.push_back({i, off, used, pl});
      used += align_page(pl);
      content += pl;
    }
  }
  if (*cancelled) {
    jobs.clear();  // pieces of an incomplete item are never hashed
    used = content = 0;
  }
  if ((rc = flush())) return rc;
  for (Slot& s : c->slots)
    if ((rc = wait_slot(s))) return rc;
  for (size_t i = 0; i < items.size(); ++i)
    if (status && item_st[i] && !status[items[i].out_index]) status[items[i].out_index] = item_st[i];
  const size_t nf = complete;
  if (nf) {
    if ((e = hipMemcpyAsync(c->d_files.p, files.data(), sizeof(FileDesc) * nf, hipMemcpyHostToDevice, st)))
      return c->hip_fail(e, "H2D files");
    if ((e = bigfile_finish(c->d_files.p, (uint32_t)nf, c->d_file_nodes.p, c->d_out32.p, st)))
      return c->hip_fail(e, "bigfile_finish");
    std::vector<uint8_t> tmp(32 * nf);
    if ((e = hipMemcpyAsync(tmp.data(), c->d_out32.p, tmp.size(), hipMemcpyDeviceToHost, st)) ||
        (e = hipStreamSynchronize(st)))
      return c->hip_fail(e, "D2H big digests");
    for (size_t i = 0; i < nf; ++i) memcpy(out32_host + 32 * items[i].out_index, &tmp[32 * i], 32);
  }
  for (size_t i = nf; i < items.size(); ++i)
    if (status && !status[items[i].out_index]) status[items[i].out_index] = SDCAS_STATUS_CANCELLED;
  return SDCAS_OK;
}



}  // namespace

// ===========================================================================

extern "C" {

const char* sdcas_version(void) { return "sdcas-mi355x 0.3.0 (gfx950)"; }

int sdcas_abi_version(void) { return SDCAS_ABI_VERSION; }

int sdcas_init(const sdcas_options* opts, sdcas_ctx** out) {
  if (!out) return SDCAS_E_INVALID;
  *out = nullptr;
  if (opts && opts->struct_size != sizeof(sdcas_options)) return SDCAS_E_INVALID;  // another revision of the struct
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SDCAS_E_NO_DEVICE;
  auto* c = new sdcas_ctx();
  int dev = -1;
  if (opts) {
    dev = opts->device;
    if (opts->io_threads) c->io_threads = std::min<uint32_t>(opts->io_threads, sdcas_ctx::kMaxIoThreads);
    if (opts->staging_bytes) c->staging_bytes = std::max<uint64_t>(opts->staging_bytes, 1ull << 20);
    c->direct_io = (opts->flags & SDCAS_OPT_DIRECT_IO) != 0;
    c->progress = opts->progress;
    c->progress_user = opts->progress_user;
    c->cancel = opts->cancel;
  }
  if (dev < 0) (void)hipGetDevice(&dev);
  if (dev >= count) {
    delete c;
    return SDCAS_E_NO_DEVICE;
  }
  // the largest batch (chunk slots) the default leaf kernel hands to the
  // small-batch kernel (b3_batch.h kSmallSlots; 0: never), for A/B runs
  if (const char* e = getenv("SDCAS_SMALL_SLOTS")) c->ws.small_slots = strtoull(e, nullptr, 0);
  if (const char* e = getenv("SDCAS_SMALL_VARIANT")) c->ws.small_variant = atoi(e);
  if (const char* e = getenv("SDCAS_UPLOAD_PARTS")) c->upload_parts = (uint32_t)std::min(atoi(e) > 0 ? atoi(e) : 0, 16);
  if (const char* e = getenv("SDCAS_PLAN_SMALL")) c->plan_small = atoi(e) != 0;
  if (const char* e = getenv("SDCAS_SMALL_DIRECT")) c->small_direct = atoi(e) != 0;
  // pinned staging per slot in MiB, over the caller's choice (A/B runs)
  if (const char* e = getenv("SDCAS_STAGING_MB"); e && atoi(e) > 0) c->staging_bytes = (uint64_t)atoi(e) << 20;
  c->device = dev;
  if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) {
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SDCAS_E_NO_DEVICE;
  }
  *out = c;
  return SDCAS_OK;
}

void sdcas_destroy(sdcas_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  // a bound stream's last call may not have recorded its event, and the
  // caller's stream may be gone by now: wait for the whole device instead
  if (!c->scratch_recorded) (void)hipDeviceSynchronize();
  else (void)c->scratch_sync();
  // (the context's DevBufs and HostStages release themselves in `delete c`,
  // after the waits above and before the streams go)
  c->dist.release();
  for (Slot& s : c->slots) slot_release(s);
  for (auto e : c->ev_free) (void)hipEventDestroy(e);
  for (auto& p : c->ev_leaf) (void)hipEventDestroy(p.first), (void)hipEventDestroy(p.second);
  for (auto& p : c->ev_all) (void)hipEventDestroy(p.first), (void)hipEventDestroy(p.second);
  if (c->scratch_ev) (void)hipEventDestroy(c->scratch_ev);
  const hipStream_t stream = c->stream, copy_stream = c->copy_stream;
  delete c;
  if (stream) (void)hipStreamDestroy(stream);
  if (copy_stream) (void)hipStreamDestroy(copy_stream);
}

const char* sdcas_last_error(const sdcas_ctx* c) { return c ? c->err.c_str() : "no context"; }

int sdcas_set_progress(sdcas_ctx* c, sdcas_progress_fn progress, void* user, const volatile int32_t* cancel) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  c->progress = progress;
  c->progress_user = user;
  c->cancel = cancel;
  return SDCAS_OK;
}

uint64_t sdcas_cas_message_len(uint64_t size) { return size <= kMin ? size + 8 : SDCAS_SAMPLED_MESSAGE_LEN; }

// The host's copy of k_plan_walk (dist_dedup.hip; the rule is described
// there): the job needs to know which rows its steps read before it writes
// their cas_ids (mod.rs:157-178 precede the lookup of :181-188), and that
// depends only on the rows' status and has_key.
int sdcas_job_plan(const uint8_t* has_key, const int32_t* status, size_t n, size_t chunk_size,
                   sdcas_job_window* win, uint64_t* out_step, uint32_t* out_reads) {
  if (!win || (n && !has_key)) return SDCAS_E_INVALID;
  const uint64_t cs = chunk_size ? chunk_size : SDCAS_IDENTIFIER_CHUNK_SIZE;
  auto stays = [&](size_t i) { return (status && status[i] != 0) || !has_key[i]; };
  std::vector<uint64_t> rr;  // re-read rows
  size_t first = SIZE_MAX;
  for (size_t p = 0; p < n; ++p) {
    if (!stays(p)) continue;
    if (first == SIZE_MAX) first = p;
    if (cs > 1 && p + 1 < n && (p + rr.size()) % cs == cs - 1) rr.push_back(p);
  }
  const uint64_t T = win->max_steps ? win->max_steps : (n + cs - 1) / cs;
  uint64_t loop = UINT64_MAX, reads = 0, steps, limit, rows = 0;
  if (cs == 1 && first != SIZE_MAX && first < T) {
    loop = first;
    reads = T - first;
    steps = T;
    limit = first;
    rows = first + 1;
  } else {
    const uint64_t E = n + rr.size();
    const uint64_t avail = win->more ? E / cs : (E + cs - 1) / cs;
    steps = std::min(avail, T);
    limit = steps * cs;
    if (steps) {
      const uint64_t P = std::min(limit, E) - 1;
      uint64_t k = 0;
      while (k < rr.size() && rr[k] + k + 1 <= P) ++k;
      rows = P - k + 1;
    }
    if (!win->more && T > avail && n && stays(n - 1)) {
      loop = n - 1;
      reads = 1 + (T - avail);
      steps = T;
    }
  }
  uint64_t run = 0;
  while (run < rr.size() && rr[run] + run + 1 < limit) ++run;
  win->steps = steps;
  win->rows = rows;
  win->rereads = run + (loop != UINT64_MAX ? reads - 1 : 0);
  if (out_step || out_reads) {
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
      while (k < rr.size() && rr[k] < i) ++k;
      const uint64_t pos = i + k;
      uint64_t s = UINT64_MAX;
      uint32_t r = 0;
      if (loop != UINT64_MAX && i >= loop) {
        if (i == loop) s = pos / cs, r = (uint32_t)std::min<uint64_t>(reads, UINT32_MAX);
      } else if (pos < limit) {
        s = pos / cs;
        r = 1 + (k < rr.size() && rr[k] == i && pos + 1 < limit ? 1 : 0);
      }
      if (out_step) out_step[i] = s;
      if (out_reads) out_reads[i] = r;
    }
  }
  return SDCAS_OK;
}

void sdcas_key_to_hex(uint64_t key, char out[17]) {
  static const char* H = "0123456789abcdef";
  for (int i = 0; i < 16; ++i) out[i] = H[(key >> (60 - 4 * i)) & 15];
  out[16] = 0;
}

void sdcas_digest_to_hex(const uint8_t d[32], char out[65]) {
  static const char* H = "0123456789abcdef";
  for (int i = 0; i < 32; ++i) {
    out[2 * i] = H[d[i] >> 4];
    out[2 * i + 1] = H[d[i] & 15];
  }
  out[64] = 0;
}

// A device-stream call: holds the context's mutex, orders its stream after
// the previous call's use of the device scratch (sdcas_ctx::fence_in) and
// marks its own use when it returns.
struct DevCall {
  sdcas_ctx* c;
  std::lock_guard<std::mutex> g;
  hipStream_t st;
  int rc = SDCAS_OK;
  DevCall(sdcas_ctx* cc, void* stream) : c(cc), g(cc->mu), st(stream ? (hipStream_t)stream : cc->stream) {
    (void)hipSetDevice(c->device);
    hipError_t e = c->fence_in(st);
    if (e) rc = c->hip_fail(e, "stream wait");
  }
  ~DevCall() { (void)c->fence_out(st); }
};

int sdcas_dev_reserve(sdcas_ctx* c, size_t max_msgs, uint64_t max_chunks) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipSetDevice(c->device);
  // the workspace is reallocated: no earlier call may still be using it
  if (hipError_t e = c->scratch_sync()) return c->hip_fail(e, "sync");
  return reserve_ws(c, max_msgs, max_chunks);
}

int sdcas_dev_hash_messages(sdcas_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, const uint64_t* d_lens,
                            size_t n, uint8_t* d_out32, uint64_t* d_out_keys, void* stream) {
  if (!c || (n && (!d_blob || !d_offsets || !d_lens))) return SDCAS_E_INVALID;
  if (n == 0) return SDCAS_OK;
  if (((uintptr_t)d_blob & 15) || ((uintptr_t)d_out32 & 15) || ((uintptr_t)d_out_keys & 7))
    return c->fail(SDCAS_E_INVALID, "dev_hash_messages: blob, digests (16 B) or keys (8 B) misaligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (n > c->ws.cap_msgs || !c->ws.S)
    return c->fail(SDCAS_E_CAPACITY, "dev_hash_messages: %zu messages > reserved %u", n, c->ws.cap_msgs);
  return launch_batch(c, d_blob, d_offsets, d_lens, (uint32_t)n, d_out32, d_out_keys, call.st);
}

// Enqueue identify_hash (b3_dual.hip) with the context's scratch grown to the
// call: n files, room for `sampled_cap` of them above 100 KiB.
static int identify_launch(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offs, const uint64_t* lens, uint32_t n,
                           uint32_t sampled_cap, uint64_t* keys, uint8_t* out32, uint8_t* has_key, hipStream_t st) {
  const size_t need = identify_scratch_bytes(n, sampled_cap);
  if (need > c->id_scratch.cap) {
    // an earlier call's kernels may still read the scratch about to be freed
    hipError_t e = c->scratch_sync();
    if (!e) e = hipStreamSynchronize(st);
    if (!e) e = c->id_scratch.ensure(need + need / 4);
    if (e) return c->hip_fail(e, "identify scratch");
  }
  const IdentifyScratch sc{c->id_scratch.p, c->id_scratch.cap};
  hipError_t e = identify_hash(c->ws, sc, blob, offs, lens, n, sampled_cap, keys, out32, has_key, st);
  return e ? c->hip_fail(e, "identify_hash") : SDCAS_OK;
}

int sdcas_dev_identify(sdcas_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, const uint64_t* d_lens, size_t n,
                       uint64_t* d_out_keys, uint8_t* d_out32, uint8_t* d_out_has_key, void* stream) {
  if (!c || (n && (!d_blob || !d_offsets || !d_lens))) return SDCAS_E_INVALID;
  if (n == 0) return SDCAS_OK;
  if (((uintptr_t)d_blob & 15) || ((uintptr_t)d_out32 & 15) || ((uintptr_t)d_out_keys & 7))
    return c->fail(SDCAS_E_INVALID, "dev_identify: blob, digests (16 B) or keys (8 B) misaligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (n > c->ws.cap_msgs || !c->ws.S || c->ws.cap_slots < 2 * kTile)
    return c->fail(SDCAS_E_CAPACITY, "dev_identify: %zu files > reserved %u", n, c->ws.cap_msgs);
  const uint32_t sampled_cap = (uint32_t)std::min<size_t>(n, SDCAS_IDENTIFY_MAX_SAMPLED);
  return identify_launch(c, d_blob, d_offsets, d_lens, (uint32_t)n, sampled_cap, d_out_keys, d_out32, d_out_has_key,
                         call.st);
}

int sdcas_dev_bind_stream(sdcas_ctx* c, void* stream, uint64_t token) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  const hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  // the last call's event, owed by this stream, is recorded while the
  // stream surely lives (a caller unbinds before destroying it)
  if (c->scratch_pending && st == c->scratch_st)
    if (hipError_t e = c->scratch_event()) return c->hip_fail(e, "dev_bind_stream");
  for (size_t i = 0; i < c->bound.size(); ++i) {
    if (c->bound[i].first != st) continue;
    if (token) c->bound[i].second = token;
    else c->bound.erase(c->bound.begin() + (long)i);
    return SDCAS_OK;
  }
  if (!token) return SDCAS_OK;
  if (c->bound.size() >= 64) return c->fail(SDCAS_E_CAPACITY, "dev_bind_stream: 64 streams bound");
  c->bound.push_back({st, token});
  return SDCAS_OK;
}

int sdcas_dev_sync(sdcas_ctx* c, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  hipError_t e = hipStreamSynchronize(st);
  if (e) return c->hip_fail(e, "sync");
  uint64_t total = 0;
  if (c->ws.total && (e = hipMemcpy(&total, c->ws.total, 8, hipMemcpyDeviceToHost))) return c->hip_fail(e, "total");
  if (total > c->ws.cap_slots)
    return c->fail(SDCAS_E_CAPACITY, "batch of %llu chunk slots exceeds reserved %llu", (unsigned long long)total,
                   (unsigned long long)c->ws.cap_slots);
  return SDCAS_OK;
}

int sdcas_dev_profile(sdcas_ctx* c, int enable) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  c->profile = enable != 0;
  for (auto* v : {&c->ev_all, &c->ev_leaf}) {
    for (auto& p : *v) c->ev_free.push_back(p.first), c->ev_free.push_back(p.second);
    v->clear();
  }
  return SDCAS_OK;
}

static float mean_ms(std::vector<std::pair<hipEvent_t, hipEvent_t>>& v) {
  float sum = 0;
  int cnt = 0;
  for (auto& p : v) {
    if (hipEventSynchronize(p.second) != hipSuccess) continue;
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
      sum += ms;
      ++cnt;
    }
  }
  return cnt ? sum / cnt : 0.f;
}

int sdcas_dev_last_kernel_ms(sdcas_ctx* c, float* leaf_ms, float* total_ms) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  if (leaf_ms) *leaf_ms = mean_ms(c->ev_leaf);
  if (total_ms) *total_ms = mean_ms(c->ev_all);
  return SDCAS_OK;
}

int sdcas_hash_messages(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* lens, size_t n,
                        uint8_t* out32);
// page-locked host memory (hipHostMalloc / hipHostRegister)? Pageable
// pointers make the query fail; its error is cleared.
static bool host_pinned(const void* p) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost && a.hostPointer != nullptr;
}

// The path calls hold the context's mutex and run on its stream; they order
// themselves after any device call that used the scratch on another stream,
// and mark their own use when they return.
struct PathCall {
  sdcas_ctx* c;
  std::lock_guard<std::mutex> g;
  int rc = SDCAS_OK;
  explicit PathCall(sdcas_ctx* cc) : c(cc), g(cc->mu) {
    (void)hipSetDevice(c->device);
    // the readers start with the context's first path call (a context used
    // only for device-resident batches never creates them)
    if (!c->pool) c->pool.reset(new sdcas_io::WorkerPool(c->io_threads));
    sdcas_io::new_path_epoch();
    hipError_t e = c->fence_in(c->stream);
    if (e) rc = c->hip_fail(e, "stream wait");
  }
  ~PathCall() {
    (void)c->fence_out(c->stream);
    sdcas_io::drop_dir_cache();  // the caller's thread (big-file opens) keeps no directory open
  }
};

// Staging bytes per slot for one path call. The two slots alternate: the I/O
// threads fill one while the GPU copies and hashes the other, so a call whose
// files fit one slot runs read -> copy -> hash -> copy back in series. A call
// of up to a few slots' worth is therefore cut into kSplit slots, but none
// below kMinSlot, where a slot's fixed cost (its copies and launches) would
// outweigh what the overlap hides. Same-process A/B with the call order
// rotated (profiles/r02_batch_split_ab.json, C2 files from the page cache):
// 3000 files per call 9.4 -> 7.8 ms, 10000 per call 22.6 -> 20.7 ms; calls
// of up to 16 MiB (the reference's 100-file step) unchanged.
constexpr uint64_t kSplit = 8, kMinSlot = 16ull << 20;
// a lone slot's reads and upload overlapped in parts (sdcas_cas_ids;
// sdcas_ctx::upload_parts, SDCAS_UPLOAD_PARTS) from this many slot bytes
constexpr uint64_t kUploadSplitMin = 1ull << 20;
static uint64_t split_cap(const uint64_t* need, const size_t* order, size_t n, uint64_t cap) {
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) total += sdcas_io::align_line(need[order ? order[i] : i]);
  return std::min<uint64_t>(cap, std::max<uint64_t>(total / kSplit + 1, kMinSlot));
}

static int hash_host_messages(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* lens,
                              size_t n, uint8_t* out32, uint64_t* keys) {
  if (!c || (n && (!blob || !offsets || !lens))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "batch of %zu messages exceeds 2^31 - 1", n);
  PathCall call(c);
  if (call.rc) return call.rc;
  const uint64_t big_cut = 1024ull * kTile;  // > 1 MiB: piece path
  const uint64_t cap = c->staging_bytes;
  const size_t cap_n = (size_t)(cap / 128) + 1;
  int rc;
  if ((rc = slots_prepare(c, cap, cap_n))) return rc;
  Progress pr{c};
  uint64_t small_bytes = 0;
  for (size_t i = 0; i < n; ++i) {
    pr.total += lens[i];
    if (lens[i] <= big_cut) small_bytes += sdcas_io::align_line(lens[i]);
  }
  const uint64_t scap = split_cap(&small_bytes, nullptr, 1, cap);
  std::vector<BigItem> big;
  int cur = 0;
  // Direct DMA: a caller buffer in pinned (page-locked) host memory whose
  // messages lie in ascending, non-overlapping, 16-byte aligned ranges is
  // copied range by range straight into the device slot (no host memcpy; the
  // path then runs at the PCIe H2D rate).
  bool direct = n > 0 && host_pinned(blob);
  for (size_t i = 0; direct && i < n; ++i)
    if ((offsets[i] & 15) || (i && offsets[i] < offsets[i - 1] + lens[i - 1])) direct = false;
  uint64_t base = 0;  // caller offset of the current direct slot's first byte
  auto begin = [&](Slot& s) -> int {
    const int r = slot_complete(
        c, s,
        [&](size_t k, const uint8_t* res) {
          const size_t i = s.idx[k];
          if (out32) memcpy(out32 + 32 * i, res, 32);
          if (keys) {
            uint64_t kk = 0;
            if (s.res32)
              for (int t = 0; t < 8; ++t) kk = (kk << 8) | res[t];
            else
              memcpy(&kk, res, 8);
            keys[i] = kk;
          }
        },
        &pr);
    s.n = 0, s.used = 0, s.chunks = 0, s.content = 0;
    s.idx.clear();
    s.src = nullptr;
    return r;
  };
  // the copy into pinned staging is the host-side cost of this path: it runs
  // on the I/O threads, one slot at a time, while the GPU hashes the other
  auto fill_submit = [&](Slot& s) -> int {
    if (direct) {
      s.src = blob + base;
    } else {
      c->pool->run(s.n, [&](size_t k) {
        memcpy(s.h + s.offs()[k], blob + offsets[s.idx[k]], s.lens()[k]);
      });
    }
    return slot_submit(c, s, out32 != nullptr);
  };
  bool cancelled = false;
  if ((rc = begin(c->slots[cur]))) return rc;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t L = lens[i];
    if (L > big_cut) {
      big.push_back({L, i});
      continue;
    }
    Slot* s = &c->slots[cur];
    const uint64_t end = direct ? offsets[i] + L - (s->n ? base : offsets[i]) : s->used + align16(L);
    if (s->n && (end > scap || s->n == cap_n)) {
      if ((rc = fill_submit(*s))) return rc;
      cur ^= 1;
      s = &c->slots[cur];
      if ((rc = begin(*s))) return rc;
      if ((cancelled = c->cancelled())) break;
    }
    if (direct && s->n == 0) base = offsets[i];
    s->offs()[s->n] = direct ? offsets[i] - base : s->used;
    s->lens()[s->n] = L;
    s->idx.push_back(i);
    s->n++;
    s->used = direct ? offsets[i] + L - base : s->used + align16(L);
    s->chunks += chunks_of(L);
    s->content += L;
  }
  if (!cancelled && (rc = fill_submit(c->slots[cur]))) return rc;
  for (Slot& s : c->slots)
    if ((rc = begin(s))) return rc;
  if (!cancelled && !big.empty()) {
    std::vector<uint8_t> d32(32 * n);
    rc = run_big(c, big, d32.data(),
                 [&](size_t k, uint8_t* dst, uint64_t off, uint32_t len) {
                   memcpy(dst, blob + offsets[big[k].out_index] + off, len);
                   return 0;
                 },
                 nullptr, pr, &cancelled);
    if (rc) return rc;
    for (auto& b : big) {
      if (out32) memcpy(out32 + 32 * b.out_index, &d32[32 * b.out_index], 32);
      if (keys) {
        uint64_t k = 0;
        for (int t = 0; t < 8; ++t) k = (k << 8) | d32[32 * b.out_index + t];
        keys[b.out_index] = k;
      }
    }
  }
  return cancelled ? c->fail(SDCAS_E_CANCELLED, "cancelled") : SDCAS_OK;
}

int sdcas_hash_messages(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* lens, size_t n,
                        uint8_t* out32) {
  if (!out32 && n) return SDCAS_E_INVALID;
  return hash_host_messages(c, blob, offsets, lens, n, out32, nullptr);
}

int sdcas_cas_ids_from_messages(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* lens,
                                size_t n, uint64_t* out_keys) {
  if (!out_keys && n) return SDCAS_E_INVALID;
  return hash_host_messages(c, blob, offsets, lens, n, nullptr, out_keys);
}

// SDCAS_TRACE_IO=1: per-call wall time of sdcas_cas_ids' phases on stderr
// (measurement aid for the page-cache path; no effect otherwise)
static bool last_parts() {
  static const bool on = [] {
    const char* v = getenv("SDCAS_LAST_PARTS");
    return v && strcmp(v, "1") == 0;
  }();
  return on;
}

struct IoTrace {
  bool on = getenv("SDCAS_TRACE_IO") != nullptr;
  double t[5] = {0, 0, 0, 0, 0};  // drain, plan, read, bookkeeping, submit
  std::chrono::steady_clock::time_point m = std::chrono::steady_clock::now();
  void lap(int k) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    t[k] += std::chrono::duration<double, std::milli>(now - m).count();
    m = now;
  }
  ~IoTrace() {
    if (on)
      fprintf(stderr, "sdcas_cas_ids trace ms: drain %.3f plan %.3f read %.3f book %.3f submit %.3f\n", t[0], t[1],
              t[2], t[3], t[4]);
  }
};

// The cas_ids of n files whose sizes are known, under a PathCall. fds (may be
// null): a file already open (fds[i] >= 0, `aligned[i]` = opened with
// O_DIRECT; sdcas_file_metadata) is read through its descriptor; any other
// is opened by path.
// meta (sdcas_file_metadata): `sizes` only plan the staging; each read takes
// the file's metadata from fstat of its descriptor (meta->sizes, meta->flags)
struct Meta {
  uint64_t* sizes;
  uint8_t* flags;
};

static int cas_ids_core(sdcas_ctx* c, const char* const* paths, const int* fds, const uint8_t* aligned,
                        const uint64_t* sizes, size_t n, uint64_t* out_keys, int32_t* out_status,
                        const Meta* meta = nullptr) {
  const uint64_t cap = c->staging_bytes;
  const size_t cap_n = (size_t)(cap / 128) + 1;
  int rc;
  if ((rc = slots_prepare(c, cap, cap_n))) return rc;
  // slot sizes: the message the indexer's size predicts (cas.rs:27); a file
  // that grew is retried in a later batch with its actual size
  std::vector<uint64_t> want(n);
  Progress pr{c};
  // (+1: room for the byte that tells a grown file from an unchanged one)
  for (size_t i = 0; i < n; ++i) {
    want[i] = sdcas_cas_message_len(sizes[i]) + (sizes[i] <= kMin ? 1 : 0);
    pr.total += sdcas_cas_message_len(sizes[i]) - 8;  // file bytes cas.rs reads
  }
  std::vector<size_t> todo(n);
  for (size_t i = 0; i < n; ++i) todo[i] = i;
  const uint64_t scap = split_cap(want.data(), nullptr, n, cap);
  int cur = 0;
  auto drain = [&](Slot& s) -> int {
    return slot_complete(c, s, [&](size_t k, const uint8_t* r) { memcpy(&out_keys[s.idx[k]], r, 8); }, &pr);
  };
  bool cancelled = false;
  IoTrace tr;
  for (int round = 0; round < 4 && !todo.empty() && !cancelled; ++round) {
    std::vector<size_t> retry;
    size_t p = 0;
    while (p < todo.size()) {
      // batch [p, q) fitting one staging slot (a message larger than the slot
      // — a whole-file cas message of a file grown past it — gets its own)
      Slot& s = c->slots[cur];
      tr.lap(4);
      if ((rc = drain(s))) return rc;
      tr.lap(0);
      if ((cancelled = c->cancelled())) {
        for (size_t k = p; k < todo.size(); ++k) out_status[todo[k]] = SDCAS_STATUS_CANCELLED;
        for (size_t i : retry) out_status[i] = SDCAS_STATUS_CANCELLED;
        retry.clear();
        break;
      }
      std::vector<uint64_t> slot_off;
      uint64_t used = 0;
      const size_t q = plan_batch(want.data(), todo.data(), p, todo.size(), scap, cap_n, slot_off, &used);
      if ((rc = slot_prepare(c, s, std::max<uint64_t>(used, cap), cap_n))) return rc;
      const size_t m = q - p;
      std::vector<uint64_t> mlen(m), retry_len(m);
      std::vector<int32_t> st(m);
      tr.lap(1);
      auto read_files = [&](size_t k0, size_t k1) {
        c->pool->run(k1 - k0, [&](size_t kk) {
          const size_t k = k0 + kk, i = todo[p + k];
          if (meta) {
            bool dir = false;
            st[k] = sdcas_io::read_file_metadata(paths[i], c->direct_io, s.h + slot_off[k], align16(want[i]),
                                                  &mlen[k], &retry_len[k], &meta->sizes[i], &dir);
            meta->flags[i] = dir ? SDCAS_META_DIR : 0;
            return;
          }
          st[k] = fds && fds[i] >= 0 ? sdcas_io::read_cas_message_fd(fds[i], aligned[i] != 0, sizes[i],
                                                                     s.h + slot_off[k], align16(want[i]), &mlen[k],
                                                                     &retry_len[k])
                                     : read_cas_message(paths[i], sizes[i], s.h + slot_off[k], align16(want[i]),
                                                        &mlen[k], &retry_len[k], c->direct_io);
        });
      };
      // A call that fits one slot is latency-bound: read -> upload -> hash in
      // series. Its files are then read in upload_parts parts of about equal
      // bytes, each part's bytes going up while the next part is read, so that
      // only the last part's upload stands between the reads and the kernels.
      const Slot& other = &s == &c->slots[0] ? c->slots[1] : c->slots[0];
      // (only for a call that fits this one slot: in a call of several slots
      // the next slot's reads already overlap this one's upload and kernels,
      // and the parts measured slower there, profiles/r03_small_calls.json)
      const uint32_t parts = c->upload_parts;
      // the flag is set only once every part is enqueued: a failed part
      // returns with it clear, so no later submit of this slot skips an upload
      s.blob_uploaded = false;
      // (and, SDCAS_LAST_PARTS=1, the last slot of a longer call: its upload
      // is the call's tail, the reads being over when it starts)
      const bool in_parts = parts > 1 && (!other.busy || last_parts()) && (p == 0 || last_parts()) &&
                            q == todo.size() && round == 0 && used >= kUploadSplitMin && m >= parts;
      if (in_parts) {
        size_t k0 = 0;
        for (uint32_t part = 1; part <= parts && k0 < m; ++part) {
          size_t k1 = k0 + 1;
          const uint64_t edge = used / parts * part;
          while (k1 < m && (part == parts || slot_off[k1] < edge)) ++k1;
          read_files(k0, k1);
          const uint64_t b0 = slot_off[k0], b1 = k1 < m ? slot_off[k1] : used;
          hipError_t e = hipMemcpyAsync(s.d_blob.p + b0, s.h + b0, b1 - b0, hipMemcpyHostToDevice, c->stream);
          if (e) return c->hip_fail(e, "H2D part");
          k0 = k1;
        }
        s.blob_uploaded = true;
      } else {
        read_files(0, m);
      }
      tr.lap(2);
      s.n = 0, s.chunks = 0, s.used = used, s.content = 0;
      s.idx.clear();
      for (size_t k = 0; k < m; ++k) {
        const size_t i = todo[p + k];
        if (retry_len[k] && !st[k]) {
          want[i] = retry_len[k];
          retry.push_back(i);
          continue;
        }
        out_status[i] = st[k];
        s.content += sdcas_cas_message_len(sizes[i]) - 8;
        if (st[k]) continue;
        if (meta && mlen[k] == 0) continue;  // a directory or an empty file: no cas_id
        if (meta) meta->flags[i] = SDCAS_META_HAS_CAS_ID;
        s.offs()[s.n] = slot_off[k];
        s.lens()[s.n] = mlen[k];
        s.idx.push_back(i);
        s.n++;
        s.chunks += chunks_of(mlen[k]);
      }
      tr.lap(3);
      if ((rc = slot_submit(c, s, false))) return rc;
      if (!s.n) pr.add(s.content);  // nothing to hash: the slot's files are final now
      cur ^= 1;
      p = q;
    }
    for (Slot& s : c->slots)
      if ((rc = drain(s))) return rc;
    todo.swap(retry);
  }
  for (size_t i : todo) out_status[i] = cancelled ? SDCAS_STATUS_CANCELLED : EAGAIN;  // EAGAIN: kept growing
  return cancelled ? c->fail(SDCAS_E_CANCELLED, "cancelled") : SDCAS_OK;
}

int sdcas_cas_ids(sdcas_ctx* c, const char* const* paths, const uint64_t* sizes, size_t n, uint64_t* out_keys,
                  int32_t* out_status) {
  if (!c || (n && (!paths || !sizes || !out_keys || !out_status))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "batch of %zu files exceeds 2^31 - 1", n);
  PathCall call(c);
  if (call.rc) return call.rc;
  return cas_ids_core(c, paths, nullptr, nullptr, sizes, n, out_keys, out_status);
}

int sdcas_file_metadata(sdcas_ctx* c, const char* const* paths, const uint64_t* size_hints, size_t n,
                        uint64_t* out_sizes, uint64_t* out_keys, int32_t* out_status, uint8_t* out_flags) {
  if (!c || (n && (!paths || !out_sizes || !out_keys || !out_status || !out_flags))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "batch of %zu files exceeds 2^31 - 1", n);
  PathCall call(c);
  if (call.rc) return call.rc;
  std::fill(out_sizes, out_sizes + n, 0);
  std::fill(out_keys, out_keys + n, 0);
  std::fill(out_flags, out_flags + n, 0);
  // the staging plan: the caller's sizes (the indexer's), else one fstatat
  // pass; either way each read takes the metadata from fstat of its own
  // descriptor and a file of another size is read again with room for it
  std::vector<uint64_t> plan(n);
  if (size_hints) {
    std::copy(size_hints, size_hints + n, plan.begin());
  } else {
    c->pool->run(n, [&](size_t i) {
      struct stat sb;
      plan[i] = stat(paths[i], &sb) == 0 && S_ISREG(sb.st_mode) ? (uint64_t)sb.st_size : 0;
    });
  }
  Meta meta{out_sizes, out_flags};
  return cas_ids_core(c, paths, nullptr, nullptr, plan.data(), n, out_keys, out_status, &meta);
}

int sdcas_checksums(sdcas_ctx* c, const char* const* paths, size_t n, uint8_t* out32, int32_t* out_status) {
  if (!c || (n && (!paths || !out32 || !out_status))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "batch of %zu files exceeds 2^31 - 1", n);
  PathCall call(c);
  if (call.rc) return call.rc;
  const uint64_t cap = c->staging_bytes, big_cut = 1024ull * kTile;
  const size_t cap_n = (size_t)(cap / 128) + 1;
  int rc;
  if ((rc = slots_prepare(c, cap, cap_n))) return rc;
  // file lengths first (hash.rs reads to EOF; a regular file's EOF is its length)
  std::vector<uint64_t> flen(n);
  std::vector<int32_t> fst(n);
  c->pool->run(n, [&](size_t i) {
    struct stat sb;
    if (stat(paths[i], &sb) != 0) fst[i] = errno;
    else if (S_ISDIR(sb.st_mode)) fst[i] = EISDIR;
    else flen[i] = (uint64_t)sb.st_size, fst[i] = 0;
  });
  std::vector<size_t> small;
  std::vector<BigItem> big;
  std::vector<uint64_t> fneed(n);  // staging bytes: the stat length + the byte that tells a grown file
  Progress pr{c};
  for (size_t i = 0; i < n; ++i) {
    out_status[i] = fst[i];
    fneed[i] = flen[i] + 1;
    if (fst[i]) continue;
    pr.total += flen[i];
    if (flen[i] > big_cut) big.push_back({flen[i], i});
    else small.push_back(i);
  }
  const uint64_t scap = split_cap(fneed.data(), small.data(), small.size(), cap);
  int cur = 0;
  auto drain = [&](Slot& s) -> int {
    return slot_complete(c, s, [&](size_t k, const uint8_t* r) { memcpy(out32 + 32 * s.idx[k], r, 32); }, &pr);
  };
  bool cancelled = false;
  size_t p = 0;
  while (p < small.size()) {
    Slot& s = c->slots[cur];
    if ((rc = drain(s))) return rc;
    if ((cancelled = c->cancelled())) break;
    std::vector<uint64_t> slot;
    uint64_t used = 0;
    const size_t q = plan_batch(fneed.data(), small.data(), p, small.size(), scap, cap_n, slot, &used);
    const size_t m = q - p;
    std::vector<uint64_t> got(m);
    std::vector<int32_t> st(m);
    c->pool->run(m, [&](size_t k) {
      const size_t i = small[p + k];
      bool isd = false;
      const int fd = open_for_read(paths[i], c->direct_io, &isd);
      if (fd < 0) {
        st[k] = -fd;
        return;
      }
      bool over = false;
      // hash.rs stops at its first short read; a file that grew since the
      // stat above is hashed over its stat length (sdcas.h)
      st[k] = read_whole_any(fd, isd, s.h + slot[k], flen[i] + 1, flen[i], &got[k], &over);
      if (over) got[k] = flen[i];
      close(fd);
    });
    s.n = 0, s.chunks = 0, s.used = used, s.content = 0;
    s.idx.clear();
    for (size_t k = 0; k < m; ++k) {
      const size_t i = small[p + k];
      out_status[i] = st[k];
      s.content += flen[i];
      if (st[k]) continue;
      s.offs()[s.n] = slot[k];
      s.lens()[s.n] = got[k];
      s.idx.push_back(i);
      s.n++;
      s.chunks += chunks_of(got[k]);
    }
    if ((rc = slot_submit(c, s, true))) return rc;
    if (!s.n) pr.add(s.content);
    cur ^= 1;
    p = q;
  }
  for (Slot& s : c->slots)
    if ((rc = drain(s))) return rc;
  if (cancelled) {
    for (size_t k = p; k < small.size(); ++k) out_status[small[k]] = SDCAS_STATUS_CANCELLED;
    for (auto& b : big) out_status[b.out_index] = SDCAS_STATUS_CANCELLED;
    return c->fail(SDCAS_E_CANCELLED, "cancelled");
  }
  if (!big.empty()) {
    // hash.rs reads the file to EOF in 1 MiB blocks; here a window's 1 MiB
    // pieces are read in parallel, with O_DIRECT when asked for and accepted
    std::vector<int> fds(big.size(), -1), oerr(big.size(), 0);
    std::vector<uint8_t> direct(big.size(), 0);
    for (size_t k = 0; k < big.size(); ++k) {
      bool d = false;
      fds[k] = open_for_read(paths[big[k].out_index], c->direct_io, &d);
      if (fds[k] < 0) oerr[k] = -fds[k];
      direct[k] = d;
    }
    std::vector<uint8_t> d32(32 * n);
    rc = run_big(c, big, d32.data(),
                 [&](size_t k, uint8_t* dst, uint64_t off, uint32_t len) -> int {
                   if (fds[k] < 0) return oerr[k];
                   return direct[k] ? pread_direct(fds[k], dst, len, off) : pread_exact(fds[k], dst, len, off);
                 },
                 out_status, pr, &cancelled);
    for (int fd : fds)
      if (fd >= 0) close(fd);
    if (rc) return rc;
    for (auto& b : big)
      if (!out_status[b.out_index]) memcpy(out32 + 32 * b.out_index, &d32[32 * b.out_index], 32);
  }
  return cancelled ? c->fail(SDCAS_E_CANCELLED, "cancelled") : SDCAS_OK;
}

static_assert(SDCAS_IDENTIFY_MAX_SAMPLED == kIdentifyMaxSampled, "sdcas.h and b3_batch.h");

// Enqueue a slot of whole file contents (s.n files at s.offs()/s.lens()) for
// sdcas_identify_checksums: the bytes and the metadata go up as in
// slot_submit, identify_hash produces digest k at result byte 32 * k and cas
// key k at 32 * s.n + 8 * k (s.n <= s.cap_n / 2, so both fit the slot's
// result words), and one copy brings them back.
static int identify_submit(sdcas_ctx* c, Slot& s) {
  s.res32 = true;
  s.blob_uploaded = false;
  if (!s.n) return SDCAS_OK;
  if (2 * s.n > s.cap_n) return c->fail(SDCAS_E_CAPACITY, "identify slot of %zu files", s.n);
  int rc;
  hipError_t e;
  hipStream_t st = c->stream;
  // each plan takes half of the workspace's slots; the files above 100 KiB
  // run as two ordinary batches (their gathered cas messages, their contents)
  uint64_t chunks_a = 0, chunks_s = 0;
  uint32_t sampled = 0;
  for (size_t k = 0; k < s.n; ++k) {
    const uint64_t len = s.lens()[k];
    if (len >= 1 && len <= kMin) {
      chunks_a += chunks_of(len + 8);
    } else {
      chunks_a += 1;
      if (len) chunks_s += std::max<uint64_t>(chunks_of(len), chunks_of(SDCAS_SAMPLED_MESSAGE_LEN)), ++sampled;
    }
  }
  const uint64_t need_chunks = std::max<uint64_t>(2 * (chunks_a + 2 * kTile), chunks_s);
  if (s.n > c->ws.cap_msgs || need_chunks > c->ws.cap_chunks) {
    if ((e = hipStreamSynchronize(st))) return c->hip_fail(e, "sync");
    if ((rc = reserve_ws(c, std::max<size_t>(s.n, c->ws.cap_msgs), std::max<uint64_t>(need_chunks, c->ws.cap_chunks))))
      return rc;
  }
  memcpy(s.hm + s.n, s.lens(), 8 * s.n);  // the lengths behind the offsets: one copy
  if ((e = slot_upload(c, s, [&](hipStream_t cs) {
         hipError_t r = hipMemcpyAsync(s.d_blob.p, s.h, s.used, hipMemcpyHostToDevice, cs);
         return r ? r : hipMemcpyAsync(s.d_meta.p, s.hm, 16 * s.n, hipMemcpyHostToDevice, cs);
       })))
    return c->hip_fail(e, "H2D");
  uint8_t* d32 = s.d_res.p;
  uint64_t* dkeys = reinterpret_cast<uint64_t*>(s.d_res.p + 32 * s.n);
  if ((rc = identify_launch(c, s.d_blob.p, s.d_meta.p, s.d_meta.p + s.n, (uint32_t)s.n, sampled, dkeys, d32, nullptr,
                            st)))
    return rc;
  if ((e = hipMemcpyAsync(s.res(), s.d_res.p, 40 * s.n, hipMemcpyDeviceToHost, st)) || (e = hipEventRecord(s.ev, st)))
    return c->hip_fail(e, "D2H");
  s.busy = true;
  return SDCAS_OK;
}

int sdcas_identify_checksums(sdcas_ctx* c, const char* const* paths, const uint64_t* size_hints, size_t n,
                             uint64_t* out_sizes, uint64_t* out_keys, uint8_t* out32, int32_t* out_status,
                             uint8_t* out_flags) {
  if (!c || (n && (!paths || !out_sizes || !out_keys || !out32 || !out_status || !out_flags))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "batch of %zu files exceeds 2^31 - 1", n);
  PathCall call(c);
  if (call.rc) return call.rc;
  std::fill(out_sizes, out_sizes + n, 0);
  std::fill(out_keys, out_keys + n, 0);
  std::fill(out_flags, out_flags + n, 0);
  std::fill(out_status, out_status + n, 0);
  memset(out32, 0, 32 * n);
  const uint64_t cap = c->staging_bytes, big_cut = 1024ull * kTile;
  const size_t cap_n = (size_t)(cap / 128) + 1;
  int rc;
  if ((rc = slots_prepare(c, cap, cap_n))) return rc;
  // the staging plan: the caller's sizes (the indexer's), else one stat pass;
  // a file planned above 1 MiB gets no room (it is streamed, or read again
  // with room if it is smaller now)
  std::vector<uint64_t> want(n);
  if (size_hints) {
    std::copy(size_hints, size_hints + n, want.begin());
  } else {
    c->pool->run(n, [&](size_t i) {
      struct stat sb;
      want[i] = stat(paths[i], &sb) == 0 && S_ISREG(sb.st_mode) ? (uint64_t)sb.st_size : 0;
    });
  }
  Progress pr{c};
  for (size_t i = 0; i < n; ++i) {
    pr.total += want[i];
    if (want[i] > big_cut) want[i] = 0;
  }
  struct Big {
    size_t i;
    uint64_t len;
    int fd;
    bool aligned;
  };
  std::vector<Big> bigs;
  std::vector<size_t> todo(n);
  for (size_t i = 0; i < n; ++i) todo[i] = i;
  const uint64_t scap = split_cap(want.data(), nullptr, n, cap);
  int cur = 0;
  auto drain = [&](Slot& s) -> int {
    if (!s.busy) return SDCAS_OK;
    s.busy = false;
    hipError_t e = hipEventSynchronize(s.ev);
    if (e) return c->hip_fail(e, "identify batch");
    for (size_t k = 0; k < s.n; ++k) {
      const size_t i = s.idx[k];
      memcpy(out32 + 32 * i, s.res() + 32 * k, 32);
      out_flags[i] |= SDCAS_META_HAS_CHECKSUM;
      if (s.lens()[k]) {
        memcpy(&out_keys[i], s.res() + 32 * s.n + 8 * k, 8);
        out_flags[i] |= SDCAS_META_HAS_CAS_ID;
      }
    }
    pr.add(s.content);
    return SDCAS_OK;
  };
  auto close_bigs = [&]() {
    for (Big& b : bigs)
      if (b.fd >= 0) close(b.fd), b.fd = -1;
  };
  bool cancelled = false;
  for (int round = 0; round < 4 && !todo.empty() && !cancelled; ++round) {
    std::vector<size_t> retry;
    size_t p = 0;
    while (p < todo.size()) {
      Slot& s = c->slots[cur];
      if ((rc = drain(s))) return close_bigs(), rc;
      if ((cancelled = c->cancelled())) {
        for (size_t k = p; k < todo.size(); ++k) out_status[todo[k]] = SDCAS_STATUS_CANCELLED;
        for (size_t i : retry) out_status[i] = SDCAS_STATUS_CANCELLED;
        retry.clear();
        break;
      }
      std::vector<uint64_t> slot_off;
      uint64_t used = 0;
      const size_t q = plan_batch(want.data(), todo.data(), p, todo.size(), scap, cap_n / 2, slot_off, &used);
      if ((rc = slot_prepare(c, s, std::max<uint64_t>(used, cap), cap_n))) return close_bigs(), rc;
      const size_t m = q - p;
      std::vector<sdcas_io::IdentifyRead> rd(m);
      std::vector<int32_t> st(m);
      c->pool->run(m, [&](size_t k) {
        const size_t i = todo[p + k];
        st[k] = sdcas_io::read_identify(paths[i], c->direct_io, s.h + slot_off[k], align16(want[i]), big_cut, &rd[k]);
      });
      s.n = 0, s.chunks = 0, s.used = used, s.content = 0;
      s.idx.clear();
      for (size_t k = 0; k < m; ++k) {
        const size_t i = todo[p + k];
        const sdcas_io::IdentifyRead& r = rd[k];
        if (!st[k] && r.need) {
          want[i] = r.need;
          retry.push_back(i);
          continue;
        }
        out_status[i] = st[k];
        out_sizes[i] = r.size;
        if (r.kind == sdcas_io::kKindDir) out_flags[i] = SDCAS_META_DIR;
        if (r.fd >= 0) {
          bigs.push_back(Big{i, r.size, r.fd, r.aligned});
          continue;
        }
        s.content += r.size;
        if (st[k] || r.kind != sdcas_io::kKindRegular || !r.opened) continue;
        s.offs()[s.n] = slot_off[k];
        s.lens()[s.n] = r.size;
        s.idx.push_back(i);
        s.n++;
      }
      if ((rc = identify_submit(c, s))) return close_bigs(), rc;
      if (!s.n) pr.add(s.content);
      cur ^= 1;
      p = q;
    }
    for (Slot& s : c->slots)
      if ((rc = drain(s))) return close_bigs(), rc;
    todo.swap(retry);
  }
  for (size_t i : todo) out_status[i] = cancelled ? SDCAS_STATUS_CANCELLED : EAGAIN;  // EAGAIN: kept changing size
  if (cancelled) {
    for (Big& b : bigs) out_status[b.i] = SDCAS_STATUS_CANCELLED;
    close_bigs();
    return c->fail(SDCAS_E_CANCELLED, "cancelled");
  }
  if (bigs.empty()) return SDCAS_OK;
  // Files above 1 MiB: the cas message (cas.rs:35-58's windows) is read
  // through the file's descriptor into a normal slot, the checksum streams
  // through run_big from the same descriptor (every such file stays open
  // until then, as sdcas_checksums keeps its big files open).
  {
    std::vector<uint64_t> mwant(bigs.size(), SDCAS_SAMPLED_MESSAGE_LEN);
    auto kdrain = [&](Slot& s) -> int {
      return slot_complete(c, s, [&](size_t k, const uint8_t* r) {
        const size_t i = bigs[s.idx[k]].i;
        memcpy(&out_keys[i], r, 8);
        out_flags[i] |= SDCAS_META_HAS_CAS_ID;
      });
    };
    size_t p = 0;
    while (p < bigs.size()) {
      Slot& s = c->slots[cur];
      if ((rc = kdrain(s))) return close_bigs(), rc;
      std::vector<uint64_t> slot_off;
      uint64_t used = 0;
      const size_t q = plan_batch(mwant.data(), nullptr, p, bigs.size(), cap, cap_n, slot_off, &used);
      const size_t m = q - p;
      std::vector<uint64_t> mlen(m), rl(m);
      std::vector<int32_t> st(m);
      c->pool->run(m, [&](size_t k) {
        const Big& b = bigs[p + k];
        st[k] = sdcas_io::read_cas_message_fd(b.fd, b.aligned, b.len, s.h + slot_off[k],
                                              align16(SDCAS_SAMPLED_MESSAGE_LEN), &mlen[k], &rl[k]);
      });
      s.n = 0, s.chunks = 0, s.used = used, s.content = 0;
      s.idx.clear();
      for (size_t k = 0; k < m; ++k) {
        const Big& b = bigs[p + k];
        out_status[b.i] = st[k];
        if (st[k]) continue;
        s.offs()[s.n] = slot_off[k];
        s.lens()[s.n] = mlen[k];
        s.idx.push_back(p + k);
        s.n++;
        s.chunks += chunks_of(mlen[k]);
      }
      if ((rc = slot_submit(c, s, false))) return close_bigs(), rc;
      cur ^= 1;
      p = q;
    }
    for (Slot& s : c->slots)
      if ((rc = kdrain(s))) return close_bigs(), rc;
  }
  std::vector<BigItem> items;
  std::vector<size_t> item_big;
  for (size_t k = 0; k < bigs.size(); ++k)
    if (!out_status[bigs[k].i]) items.push_back({bigs[k].len, bigs[k].i}), item_big.push_back(k);
  std::vector<uint8_t> d32(32 * n);
  rc = run_big(c, items, d32.data(),
               [&](size_t k, uint8_t* dst, uint64_t off, uint32_t len) -> int {
                 const Big& b = bigs[item_big[k]];
                 return b.aligned ? pread_direct(b.fd, dst, len, off) : pread_exact(b.fd, dst, len, off);
               },
               out_status, pr, &cancelled);
  close_bigs();
  if (rc) return rc;
  for (const BigItem& it : items) {
    const size_t i = it.out_index;
    if (!out_status[i]) {
      memcpy(out32 + 32 * i, &d32[32 * i], 32);
      out_flags[i] |= SDCAS_META_HAS_CHECKSUM;
    } else {
      out_flags[i] = 0;  // a status means neither result
      out_keys[i] = 0;
    }
  }
  return cancelled ? c->fail(SDCAS_E_CANCELLED, "cancelled") : SDCAS_OK;
}


// ---- dedup -----------------------------------------------------------------
//
// One implementation: the hash-table group-by of dist_dedup.hip. A single
// rank (this call) runs it fused (dd_local: files and existing Objects go
// straight into the resolve table; one insert pass per side, one apply
// pass); a node of ranks runs the same stages split at the exchange
// (sdcas_dev_dedup_combine / resolve / apply).

__global__ void k_iota64(uint64_t* __restrict__ p, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}

static hipError_t iota(DevBuf<uint64_t>& b, size_t n, hipStream_t st) {
  hipError_t e = b.ensure(std::max<size_t>(n, 1));
  if (e || !n) return e;
  hipLaunchKernelGGL(k_iota64, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, b.p, (uint32_t)n);
  return hipGetLastError();
}

// the resolve table holds 2 * (files + existing) entries, at most 2^31
static bool dedup_fits(size_t n, size_t ne) { return (uint64_t)n + ne <= (1ull << 30); }

int sdcas_dedup_window(sdcas_ctx* c, const uint64_t* keys, const uint8_t* has_key, const int32_t* status, size_t n,
                       size_t chunk_size, const uint64_t* existing_keys, size_t n_existing, sdcas_job_window* win,
                       int64_t* out_link, int64_t* out_created, int64_t* out_linked) {
  if (!c || (n && (!keys || !has_key || !out_link)) || (n_existing && !existing_keys)) return SDCAS_E_INVALID;
  if (!dedup_fits(n, n_existing))
    return c->fail(SDCAS_E_CAPACITY, "dedup of %zu files + %zu Objects exceeds 2^30", n, n_existing);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  if (chunk_size == 0) chunk_size = SDCAS_IDENTIFIER_CHUNK_SIZE;
  hipError_t e;
  hipStream_t st = call.st;
  unsigned long long cnt[2] = {0, 0};
  uint64_t hdr[kPlanHeader] = {};
  Parts p(c, st, "dedup");
  const auto d_keys = p.in(keys, n);
  const auto d_has = p.in(has_key, n);
  const auto d_status = p.in(status, n);
  const auto d_ekeys = p.in(existing_keys, n_existing);
  const auto d_link = p.out(out_link, n);
  const auto d_cnt = p.out(cnt, 2);
  if (int rc = p.reserve()) return rc;
  if (int rc = p.upload()) return rc;
  if ((e = hipMemsetAsync(d_cnt, 0, sizeof cnt, st))) return c->hip_fail(e, "dedup counts");
  // files are ordinals 0..n-1 in orphan order, existing Objects 0..ne-1 in DB
  // order: one iota serves both (ids of the first min(n, ne) coincide)
  if ((e = iota(c->dd_ids, std::max(n, n_existing), st))) return c->hip_fail(e, "dedup ids");
  StepWindow sw;
  sw.n_total = n;
  sw.max_steps = win ? win->max_steps : 0;
  sw.more = win ? win->more : 0;
  if ((e = dd_local(c->dist, d_keys, d_has, d_status, c->dd_ids.p, (uint32_t)n, d_ekeys, c->dd_ids.p,
                    (uint32_t)n_existing, chunk_size, sw, d_link, d_cnt, st)))
    return c->hip_fail(e, "dedup");
  if (int rc = p.fetch(hdr, c->dist.plan.p, kPlanHeader)) return rc;
  if (int rc = p.download()) return rc;
  if (out_created) *out_created = (int64_t)cnt[0];
  if (out_linked) *out_linked = (int64_t)cnt[1];
  if (win) {
    win->steps = hdr[kPlanSteps];
    win->rows = hdr[kPlanRows];
    win->rereads = hdr[kPlanRereadsRun];
  }
  return SDCAS_OK;
}

int sdcas_dedup(sdcas_ctx* c, const uint64_t* keys, const uint8_t* has_key, const int32_t* status, size_t n,
                size_t chunk_size, const uint64_t* existing_keys, size_t n_existing, int64_t* out_link,
                int64_t* out_created, int64_t* out_linked) {
  return sdcas_dedup_window(c, keys, has_key, status, n, chunk_size, existing_keys, n_existing, nullptr, out_link,
                            out_created, out_linked);
}

int sdcas_dev_dedup(sdcas_ctx* c, const uint64_t* d_keys, const uint8_t* d_has_key, const int32_t* d_status,
                    size_t n, size_t chunk_size, int64_t* d_out_link, uint64_t* d_counts, void* stream) {
  if (!c || (n && (!d_keys || !d_has_key || !d_out_link))) return SDCAS_E_INVALID;
  if (!dedup_fits(n, 0)) return c->fail(SDCAS_E_CAPACITY, "dev_dedup of %zu files exceeds 2^30", n);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (chunk_size == 0) chunk_size = SDCAS_IDENTIFIER_CHUNK_SIZE;
  hipError_t e;
  if (d_counts && (e = hipMemsetAsync(d_counts, 0, 2 * sizeof(uint64_t), call.st))) return c->hip_fail(e, "counts");
  if ((e = iota(c->dd_ids, n, call.st))) return c->hip_fail(e, "dev_dedup ids");
  e = dd_local(c->dist, d_keys, d_has_key, d_status, c->dd_ids.p, (uint32_t)n, nullptr, nullptr, 0, chunk_size,
               StepWindow{}, d_out_link, (unsigned long long*)d_counts, call.st);
  return e ? c->hip_fail(e, "dev_dedup") : SDCAS_OK;
}

// ---- duplicates confirmed by checksum (confirm.hip) ------------------------------

// the group-by's workspace grown to n files
static int confirm_ws(sdcas_ctx* c, size_t n, hipStream_t st) {
  return grow_synced(c, c->cf_ws, (size_t)confirm_ws_words(n), st, "confirm workspace");
}

int sdcas_dev_confirm_duplicates(sdcas_ctx* c, const uint64_t* d_keys, const uint8_t* d_digests32,
                                 const uint8_t* d_valid, size_t n, int64_t* d_out_rep, int64_t* d_out_key_rep,
                                 uint8_t* d_out_flags, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  if (n > kConfirmMaxFiles) return c->fail(SDCAS_E_CAPACITY, "dev_confirm_duplicates of %zu files exceeds 2^30", n);
  if (n && (!d_keys || !d_digests32)) return c->fail(SDCAS_E_INVALID, "dev_confirm_duplicates: null keys or digests");
  if (n && ((uintptr_t)d_digests32 & 15))
    return c->fail(SDCAS_E_INVALID, "dev_confirm_duplicates: digests not 16-byte aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e;
  if (n == 0) {
    if (d_counts && (e = hipMemsetAsync(d_counts, 0, kConfirmCounts * sizeof(uint64_t), call.st)))
      return c->hip_fail(e, "counts");
    return SDCAS_OK;
  }
  if (int rc = confirm_ws(c, n, call.st)) return rc;
  e = confirm_duplicates(c->cf_ws.p, d_keys, d_digests32, d_valid, (uint32_t)n, d_out_rep, d_out_key_rep, d_out_flags,
                         (unsigned long long*)d_counts, call.st);
  return e ? c->hip_fail(e, "dev_confirm_duplicates") : SDCAS_OK;
}

int sdcas_confirm_duplicates(sdcas_ctx* c, const uint64_t* keys, const uint8_t* digests32, const uint8_t* valid,
                             size_t n, int64_t* out_rep, int64_t* out_key_rep, uint8_t* out_flags,
                             sdcas_confirm_counts* out_counts) {
  static_assert(sizeof(sdcas_confirm_counts) == kConfirmCounts * sizeof(uint64_t), "six u64 counts");
  if (!c) return SDCAS_E_INVALID;
  if (n > kConfirmMaxFiles) return c->fail(SDCAS_E_CAPACITY, "confirm_duplicates of %zu files exceeds 2^30", n);
  if (n && (!keys || !digests32)) return c->fail(SDCAS_E_INVALID, "confirm_duplicates: null keys or digests");
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  if (n == 0) return SDCAS_OK;
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  Parts p(c, st, "confirm_duplicates");
  const auto d_keys = p.in(keys, n);
  const auto d_digests = p.in(digests32, 32 * n);
  const auto d_valid = p.in(valid, n);
  const auto d_rep = p.out(out_rep, n);
  const auto d_krep = p.out(out_key_rep, n);
  const auto d_flags = p.out(out_flags, n);
  const auto d_cts = p.out(out_counts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = confirm_ws(c, n, st)) return rc;
  if (int rc = p.upload()) return rc;
  if (hipError_t e = confirm_duplicates(c->cf_ws.p, d_keys, d_digests, d_valid, (uint32_t)n, d_rep, d_krep, d_flags,
                                        d_cts.as<unsigned long long>(), st))
    return c->hip_fail(e, "confirm_duplicates");
  return p.download();
}

// ---- duplicate sets (dupsets.hip) ----------------------------------------------

// the workspace grown to n files
static int dupsets_ws(sdcas_ctx* c, size_t n, hipStream_t st) {
  return grow_synced(c, c->ds_ws, (size_t)dupsets_ws_words(n), st, "duplicate sets workspace");
}

static int dupsets_args(sdcas_ctx* c, const char* who, const void* rep, const void* sizes, size_t n, uint32_t order) {
  if (order != SDCAS_SETS_BY_REP && order != SDCAS_SETS_BY_RECLAIMABLE)
    return c->fail(SDCAS_E_INVALID, "%s: unknown order %u", who, order);
  if (order == SDCAS_SETS_BY_RECLAIMABLE && !sizes)
    return c->fail(SDCAS_E_INVALID, "%s: the order by reclaimable bytes needs sizes", who);
  if (n > kDupsetsMaxFiles) return c->fail(SDCAS_E_CAPACITY, "%s of %zu files exceeds 2^30", who, n);
  if (n && !rep) return c->fail(SDCAS_E_INVALID, "%s: null rep", who);
  return SDCAS_OK;
}

int sdcas_dev_duplicate_sets(sdcas_ctx* c, const int64_t* d_rep, const uint64_t* d_sizes, size_t n, uint32_t order,
                             int64_t* d_set_rep, uint64_t* d_set_offsets, uint64_t* d_set_bytes, int64_t* d_members,
                             uint64_t* d_counts, void* stream) {
  static_assert(SDCAS_SETS_BY_REP == kDupsetsBySetRep && SDCAS_SETS_BY_RECLAIMABLE == kDupsetsByReclaimable, "orders");
  if (!c) return SDCAS_E_INVALID;
  if (int rc = dupsets_args(c, "dev_duplicate_sets", d_rep, d_sizes, n, order)) return rc;
  if (((uintptr_t)d_rep | (uintptr_t)d_sizes | (uintptr_t)d_set_rep | (uintptr_t)d_set_offsets |
       (uintptr_t)d_set_bytes | (uintptr_t)d_members | (uintptr_t)d_counts) & 7)
    return c->fail(SDCAS_E_INVALID, "dev_duplicate_sets: an array is not 8-byte aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e;
  if (n == 0) {
    if (d_counts && (e = hipMemsetAsync(d_counts, 0, kDupsetsCounts * sizeof(uint64_t), call.st)))
      return c->hip_fail(e, "counts");
    if (d_set_offsets && (e = hipMemsetAsync(d_set_offsets, 0, sizeof(uint64_t), call.st)))
      return c->hip_fail(e, "set_offsets");
    return SDCAS_OK;
  }
  if (int rc = dupsets_ws(c, n, call.st)) return rc;
  e = duplicate_sets(c->ds_ws.p, d_rep, d_sizes, (uint32_t)n, order, d_set_rep, d_set_offsets, d_set_bytes, d_members,
                     (unsigned long long*)d_counts, call.st);
  return e ? c->hip_fail(e, "dev_duplicate_sets") : SDCAS_OK;
}

int sdcas_duplicate_sets(sdcas_ctx* c, const int64_t* rep, const uint64_t* sizes, size_t n, uint32_t order,
                         int64_t* out_set_rep, uint64_t* out_set_offsets, uint64_t* out_set_bytes,
                         int64_t* out_members, sdcas_sets_counts* out_counts) {
  static_assert(sizeof(sdcas_sets_counts) == kDupsetsCounts * sizeof(uint64_t), "six u64 counts");
  if (!c) return SDCAS_E_INVALID;
  if (int rc = dupsets_args(c, "duplicate_sets", rep, sizes, n, order)) return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  if (n == 0) {
    if (out_set_offsets) out_set_offsets[0] = 0;
    return SDCAS_OK;
  }
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t h = n / 2;  // no more sets than that
  sdcas_sets_counts cts;
  Parts p(c, st, "duplicate_sets");
  const auto d_rep = p.in(rep, n);
  const auto d_sizes = p.in(sizes, n);
  const auto d_set_rep = p.out(out_set_rep, h);
  const auto d_set_offsets = p.out(out_set_offsets, h + 1);
  const auto d_set_bytes = p.out(out_set_bytes, h);
  const auto d_members = p.out(out_members, n);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = dupsets_ws(c, n, st)) return rc;
  if (int rc = p.upload()) return rc;
  if (hipError_t e = duplicate_sets(c->ds_ws.p, d_rep, d_sizes, (uint32_t)n, order, d_set_rep, d_set_offsets,
                                    d_set_bytes, d_members, d_cts.as<unsigned long long>(), st))
    return c->hip_fail(e, "duplicate_sets");
  if (int rc = p.counts(d_cts)) return rc;
  if (cts.sets > h || cts.members > n) return c->fail(SDCAS_E_HIP, "duplicate_sets: counts out of range");
  d_set_rep.first(cts.sets), d_set_offsets.first(cts.sets + 1), d_set_bytes.first(cts.sets);
  d_members.first(cts.members);
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

// ---- directory digests and top-most duplicates (dirtree.hip) ---------------------

int sdcas_tree_plan(const int64_t* parent, const uint8_t* is_dir, size_t n, uint32_t* out_depth,
                    uint64_t* out_children, uint64_t* out_levels) {
  static_assert(SDCAS_TREE_MAX_DEPTH == kTreeMaxDepth, "depth limit");
  TreeShape s;
  const TreeShapeError err = tree_shape(parent, is_dir, n, false, s, nullptr);
  if (err) return err == kTreeCapacity ? SDCAS_E_CAPACITY : SDCAS_E_INVALID;
  if (out_depth && n) memcpy(out_depth, s.depth.data(), n * sizeof(uint32_t));
  if (out_children && n) memcpy(out_children, s.children.data(), n * sizeof(uint64_t));
  if (out_levels) *out_levels = s.levels;
  return SDCAS_OK;
}

static int tree_shape_checked(sdcas_ctx* c, const char* who, const int64_t* parent, const uint8_t* is_dir, size_t n,
                              TreeShape& s) {
  const char* why = "";
  const TreeShapeError err = tree_shape(parent, is_dir, n, true, s, &why);
  if (err) return c->fail(err == kTreeCapacity ? SDCAS_E_CAPACITY : SDCAS_E_INVALID, "%s: %s", who, why);
  return SDCAS_OK;
}

// Enqueue the whole of tree_digests on st (device arrays, a checked shape, n != 0).
static int tree_enqueue(sdcas_ctx* c, const char* who, const TreeShape& s, const uint8_t* is_dir, TreeArgs a,
                        uint64_t* d_counts, hipStream_t st) {
  static_assert(SDCAS_TREE_DIR == kTreeDir && SDCAS_TREE_INCOMPLETE == kTreeIncomplete &&
                    SDCAS_TREE_EMPTY == kTreeEmpty && SDCAS_TOP_DUP == kTopDup && SDCAS_TOP_NESTED == kTopNested,
                "flags");
  const TreeLayout l = tree_layout(s.n, s.dirs, s.max_level_dirs, s.max_level_bytes);
  hipError_t e;
  // an earlier call's kernels may still use what is about to be freed
  const bool grow_ws = l.bytes > c->tr_ws.cap;
  const bool grow_batch =
      s.dirs && (!c->ws.S || s.max_level_dirs > c->ws.cap_msgs || s.max_level_chunks > c->ws.cap_chunks);
  if (grow_ws || grow_batch) {
    if ((e = c->scratch_sync()) || (e = hipStreamSynchronize(st))) return c->hip_fail(e, "tree workspace");
    if (grow_ws && (e = c->tr_ws.ensure(l.bytes))) return c->hip_fail(e, "tree workspace");
    if (grow_batch)
      if (int rc = reserve_ws(c, std::max<size_t>(s.max_level_dirs, c->ws.cap_msgs),
                              std::max<uint64_t>(s.max_level_chunks, c->ws.cap_chunks)))
        return rc;
  }
  a.ws = c->tr_ws.p;
  {
    // the shape's arrays are laid out in the pinned buffer itself
    uint8_t* meta = nullptr;
    if ((e = c->tr_stage.reserve(l.meta_bytes, &meta))) return c->hip_fail(e, "tree shape upload");
    tree_meta_fill(s, is_dir, l, meta);
    if ((e = c->tr_stage.send(l.meta_bytes, a.ws, st))) return c->hip_fail(e, "tree shape upload");
  }
  if ((e = tree_begin(s, l, a, st))) return c->hip_fail(e, who);
  for (uint32_t depth = s.dir_levels; depth-- > 0;) {
    const uint32_t nd = s.level_first[depth + 1] - s.level_first[depth];
    if (!nd) continue;
    if ((e = tree_level_gather(s, l, a, depth, st))) return c->hip_fail(e, who);
    if (int rc = launch_batch(c, a.ws + l.blob, reinterpret_cast<const uint64_t*>(a.ws + l.offs),
                              reinterpret_cast<const uint64_t*>(a.ws + l.lens), nd, a.ws + l.tdig, nullptr, st,
                              s.level_chunks[depth]))
      return rc;
    if ((e = tree_level_finish(s, l, a, depth, st))) return c->hip_fail(e, who);
  }
  if (d_counts && (e = hipMemcpyAsync(d_counts, a.ws + l.counts, kTreeCounts * sizeof(uint64_t),
                                      hipMemcpyDeviceToDevice, st)))
    return c->hip_fail(e, who);
  return SDCAS_OK;
}

int sdcas_dev_tree_digests(sdcas_ctx* c, const int64_t* parent, const uint8_t* is_dir, const uint8_t* d_name32,
                           const uint64_t* d_sizes, size_t n, uint64_t* d_keys, uint8_t* d_digests32,
                           uint8_t* d_valid, uint64_t* d_out_tree_bytes, uint64_t* d_out_tree_files,
                           uint8_t* d_out_flags, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  TreeShape s;
  if (int rc = tree_shape_checked(c, "dev_tree_digests", parent, is_dir, n, s)) return rc;
  if (n && (!d_name32 || !d_digests32)) return c->fail(SDCAS_E_INVALID, "dev_tree_digests: null name32 or digests32");
  if (((uintptr_t)d_name32 | (uintptr_t)d_digests32) & 15)
    return c->fail(SDCAS_E_INVALID, "dev_tree_digests: name32 or digests32 not 16-byte aligned");
  if (((uintptr_t)d_sizes | (uintptr_t)d_keys | (uintptr_t)d_out_tree_bytes | (uintptr_t)d_out_tree_files |
       (uintptr_t)d_counts) & 7)
    return c->fail(SDCAS_E_INVALID, "dev_tree_digests: an array is not 8-byte aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (n == 0) {
    hipError_t e;
    if (d_counts && (e = hipMemsetAsync(d_counts, 0, kTreeCounts * sizeof(uint64_t), call.st)))
      return c->hip_fail(e, "counts");
    return SDCAS_OK;
  }
  return tree_enqueue(c, "dev_tree_digests", s, is_dir,
                      TreeArgs{nullptr, d_name32, d_sizes, d_keys, d_digests32, d_valid, d_out_tree_bytes,
                               d_out_tree_files, d_out_flags},
                      d_counts, call.st);
}

int sdcas_tree_digests(sdcas_ctx* c, const int64_t* parent, const uint8_t* is_dir, const uint8_t* name32,
                       const uint64_t* sizes, size_t n, uint64_t* keys, uint8_t* digests32, uint8_t* valid,
                       uint64_t* out_tree_bytes, uint64_t* out_tree_files, uint8_t* out_flags,
                       sdcas_tree_counts* out_counts) {
  static_assert(sizeof(sdcas_tree_counts) == kTreeCounts * sizeof(uint64_t), "six u64 counts");
  if (!c) return SDCAS_E_INVALID;
  TreeShape s;
  if (int rc = tree_shape_checked(c, "tree_digests", parent, is_dir, n, s)) return rc;
  if (n && (!name32 || !digests32)) return c->fail(SDCAS_E_INVALID, "tree_digests: null name32 or digests32");
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  if (n == 0) return SDCAS_OK;
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  Parts p(c, st, "tree_digests");
  const auto d_name = p.in(name32, 32 * n);
  const auto d_sizes = p.in(sizes, n);
  // (the file entries' slots of these three come back as they went up)
  const auto d_keys = p.inout(keys, n);
  const auto d_digests = p.inout(digests32, 32 * n);
  const auto d_valid = p.inout(valid, n);
  const auto d_tb = p.out(out_tree_bytes, n);
  const auto d_tf = p.out(out_tree_files, n);
  const auto d_flags = p.out(out_flags, n);
  const auto d_cts = p.out(out_counts, 1, true);
  if (int rc = p.reserve()) return rc;
  if (int rc = p.upload()) return rc;
  const TreeArgs a{nullptr, d_name, d_sizes, d_keys, d_digests, d_valid, d_tb, d_tf, d_flags};
  if (int rc = tree_enqueue(c, "tree_digests", s, is_dir, a, d_cts.as<uint64_t>(), st)) return rc;
  return p.download();
}

// the workspace grown to n entries
static int tree_top_ws(sdcas_ctx* c, size_t n, hipStream_t st) {
  return grow_synced(c, c->tt_ws, (size_t)tree_top_ws_words(n), st, "tree_top workspace");
}

int sdcas_dev_tree_top(sdcas_ctx* c, const int64_t* d_parent, const int64_t* d_rep, size_t n, int64_t* d_out_top_rep,
                       uint8_t* d_out_flags, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  if (n > kTreeMaxEntries) return c->fail(SDCAS_E_CAPACITY, "dev_tree_top of %zu entries exceeds 2^30", n);
  if (n && (!d_parent || !d_rep)) return c->fail(SDCAS_E_INVALID, "dev_tree_top: null parent or rep");
  if (((uintptr_t)d_parent | (uintptr_t)d_rep | (uintptr_t)d_out_top_rep | (uintptr_t)d_counts) & 7)
    return c->fail(SDCAS_E_INVALID, "dev_tree_top: an array is not 8-byte aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e;
  if (n == 0) {
    if (d_counts && (e = hipMemsetAsync(d_counts, 0, kTreeCounts * sizeof(uint64_t), call.st)))
      return c->hip_fail(e, "counts");
    return SDCAS_OK;
  }
  if (int rc = tree_top_ws(c, n, call.st)) return rc;
  e = tree_top(c->tt_ws.p, d_parent, d_rep, (uint32_t)n, d_out_top_rep, d_out_flags, (unsigned long long*)d_counts,
               call.st);
  return e ? c->hip_fail(e, "dev_tree_top") : SDCAS_OK;
}

int sdcas_tree_top(sdcas_ctx* c, const int64_t* parent, const int64_t* rep, size_t n, int64_t* out_top_rep,
                   uint8_t* out_flags, sdcas_top_counts* out_counts) {
  static_assert(sizeof(sdcas_top_counts) == kTreeCounts * sizeof(uint64_t), "six u64 counts");
  if (!c) return SDCAS_E_INVALID;
  if (n > kTreeMaxEntries) return c->fail(SDCAS_E_CAPACITY, "tree_top of %zu entries exceeds 2^30", n);
  if (n && (!parent || !rep)) return c->fail(SDCAS_E_INVALID, "tree_top: null parent or rep");
  for (size_t i = 0; i < n; ++i)
    if (parent[i] < -1 || parent[i] >= (int64_t)n) return c->fail(SDCAS_E_INVALID, "tree_top: a parent outside [-1, n)");
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  if (n == 0) return SDCAS_OK;
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  Parts p(c, st, "tree_top");
  const auto d_parent = p.in(parent, n);
  const auto d_rep = p.in(rep, n);
  const auto d_top = p.out(out_top_rep, n);
  const auto d_flags = p.out(out_flags, n);
  const auto d_cts = p.out(out_counts, 1, true);
  if (int rc = p.reserve()) return rc;
  if (int rc = tree_top_ws(c, n, st)) return rc;
  if (int rc = p.upload()) return rc;
  if (hipError_t e = tree_top(c->tt_ws.p, d_parent, d_rep, (uint32_t)n, d_top, d_flags,
                              d_cts.as<unsigned long long>(), st))
    return c->hip_fail(e, "tree_top");
  return p.download();
}

// ---- content-defined chunks and their sharing (cdc.hip) ---------------------------

static CdcParams chunk_params(const sdcas_chunk_params* p) {
  const sdcas_chunk_params d = SDCAS_CHUNK_PARAMS_DEFAULT;
  if (!p) p = &d;
  return CdcParams{p->min_len, p->avg_bits, p->max_len};
}

int sdcas_chunk_plan(const uint64_t* lens, size_t n, const sdcas_chunk_params* params, uint64_t* out_max_chunks,
                     uint64_t* out_max_slots) {
  static_assert(SDCAS_CHUNK_MAX_CHUNKS == kCdcMaxChunks && SDCAS_CHUNK_GEAR_TILE == kCdcTile &&
                    SDCAS_CHUNK_GEAR_STRIP == kCdcStrip,
                "chunk constants");
  const CdcPlanError err = cdc_plan(lens, n, chunk_params(params), out_max_chunks, out_max_slots);
  return err == kCdcOk ? SDCAS_OK : err == kCdcCapacity ? SDCAS_E_CAPACITY : SDCAS_E_INVALID;
}

// the packed bytes one hash batch may hold (SDCAS_CHUNK_PACK_BYTES, read per call)
static uint64_t chunk_pack_cap() {
  const char* v = getenv("SDCAS_CHUNK_PACK_BYTES");
  const unsigned long long x = v ? strtoull(v, nullptr, 10) : 0;
  return x ? x : 256ull << 20;
}

// Enqueue the whole of a chunk call on st (device arrays, valid parameters,
// n != 0); waits for st once when keys or digests are asked for.
// win: the call is over windows (sdcas_dev_chunk_windows), cut in segments.
static int chunk_enqueue(sdcas_ctx* c, const char* who, CdcArgs a, uint64_t* d_keys, uint8_t* d_digests32,
                         uint64_t* d_counts, hipStream_t st, const CdcWinArgs* win = nullptr) {
  CdcWinLayout w{};
  if (win) {
    w = cdc_win_layout(a.n, a.max_chunks, a.file_slots, a.p, win->seg);
    if (w.max_segs > 0xFFFFFFFEull) return c->fail(SDCAS_E_CAPACITY, "%s: more than 2^32 segments", who);
  }
  const CdcLayout l = win ? w.l : cdc_layout(a.n, a.max_chunks, a.file_slots);
  const uint64_t ws_bytes = win ? w.bytes : l.bytes;
  hipError_t e;
  if (ws_bytes > c->cd_ws.cap) {
    // an earlier call's kernels may still use what is about to be freed
    if ((e = c->scratch_sync()) || (e = hipStreamSynchronize(st)) || (e = c->cd_ws.ensure(ws_bytes)))
      return c->hip_fail(e, "chunk workspace");
  }
  a.ws = c->cd_ws.p;
  if ((e = win ? cdc_chunk_windows(w, a, *win, st) : cdc_chunk(l, a, st))) return c->hip_fail(e, who);
  if (d_counts &&
      (e = hipMemcpyAsync(d_counts, a.ws + l.counts, kCdcCounts * sizeof(uint64_t), hipMemcpyDeviceToDevice, st)))
    return c->hip_fail(e, who);
  if ((!d_keys && !d_digests32) || a.max_chunks == 0) return SDCAS_OK;

  // the one wait: the counts and the chunk lengths down, the batches planned here
  uint64_t cts[8] = {};
  std::vector<uint64_t> len(a.max_chunks);
  if ((e = hipMemcpyAsync(cts, a.ws + l.counts, sizeof cts, hipMemcpyDeviceToHost, st)) ||
      (e = hipMemcpyAsync(len.data(), a.ws + l.wlen, 8 * a.max_chunks, hipMemcpyDeviceToHost, st)) ||
      (e = hipStreamSynchronize(st)))
    return c->hip_fail(e, "chunk lengths");
  const uint64_t m = cts[1];
  if (m > a.max_chunks || cts[7])
    return c->fail(SDCAS_E_CAPACITY, "%s: the lengths on the device need more than max_chunks / max_slots", who);
  if (m == 0) return SDCAS_OK;
  // batches of consecutive chunks, each chunk at the next 16-byte boundary of its batch
  struct Batch {
    uint64_t c0, bytes, b3_chunks;
    uint32_t nb;
  };
  const uint64_t cap = chunk_pack_cap();
  std::vector<Batch> batches;
  uint8_t* stage = nullptr;
  if ((e = c->cd_stage.reserve(8 * m, &stage))) return c->hip_fail(e, "chunk pack upload");
  uint64_t* po = reinterpret_cast<uint64_t*>(stage);
  Batch b{0, 0, 0, 0};
  uint64_t max_bytes = 0, max_b3 = 0;
  uint32_t max_nb = 0;
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t padded = (len[k] + 15) & ~15ull;
    if (b.nb && (b.bytes + padded > cap || b.nb == SDCAS_MAX_BATCH)) {
      batches.push_back(b);
      b = Batch{k, 0, 0, 0};
    }
    po[k] = b.bytes;
    b.bytes += padded, b.b3_chunks += chunks_of(len[k]), ++b.nb;
    max_bytes = std::max(max_bytes, b.bytes), max_b3 = std::max(max_b3, b.b3_chunks), max_nb = std::max(max_nb, b.nb);
  }
  batches.push_back(b);
  if ((e = c->cd_stage.send(8 * m, a.ws + l.po, st))) return c->hip_fail(e, "chunk pack upload");
  // (the stream is idle and waited for every earlier call: nothing uses what is freed here)
  if (max_bytes + kSlack > c->cd_pack.cap && (e = c->cd_pack.ensure(max_bytes + kSlack)))
    return c->hip_fail(e, "chunk pack scratch");
  if (!c->ws.S || max_nb > c->ws.cap_msgs || max_b3 > c->ws.cap_chunks)
    if (int rc = reserve_ws(c, std::max<size_t>(max_nb, c->ws.cap_msgs), std::max<uint64_t>(max_b3, c->ws.cap_chunks)))
      return rc;
  for (const Batch& x : batches) {
    if ((e = cdc_pack(l, a, x.c0, x.nb, x.bytes, c->cd_pack.p, st))) return c->hip_fail(e, who);
    if (int rc = launch_batch(c, c->cd_pack.p, reinterpret_cast<const uint64_t*>(a.ws + l.po) + x.c0,
                              reinterpret_cast<const uint64_t*>(a.ws + l.wlen) + x.c0, x.nb,
                              d_digests32 ? d_digests32 + 32 * x.c0 : nullptr, d_keys ? d_keys + x.c0 : nullptr, st,
                              x.b3_chunks))
      return rc;
  }
  return SDCAS_OK;
}

// the checks both chunk calls share; *slots <- max_slots - max_chunks
static int chunk_args(sdcas_ctx* c, const char* who, const void* offs, const void* lens, size_t n, const CdcParams& p,
                      uint64_t max_chunks, uint64_t max_slots, uint64_t* slots) {
  if (!cdc_params_valid(p)) return c->fail(SDCAS_E_INVALID, "%s: invalid chunk parameters", who);
  if (n && (!offs || !lens)) return c->fail(SDCAS_E_INVALID, "%s: null offsets or lens", who);
  if (n >= 0xFFFFFFFFull) return c->fail(SDCAS_E_CAPACITY, "%s of %zu files exceeds 2^32 - 2", who, n);
  if (max_chunks > kCdcMaxChunks) return c->fail(SDCAS_E_CAPACITY, "%s: more than 2^30 chunks", who);
  if (max_slots < max_chunks || max_slots - max_chunks > 0xFFFFFFFEull)
    return c->fail(SDCAS_E_CAPACITY, "%s: max_slots is below max_chunks or above 2^32", who);
  *slots = max_slots - max_chunks;
  return SDCAS_OK;
}

int sdcas_dev_chunk(sdcas_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, const uint64_t* d_lens, size_t n,
                    const sdcas_chunk_params* params, uint64_t max_chunks, uint64_t max_slots, uint64_t* d_file_chunks,
                    uint64_t* d_chunk_off, uint64_t* d_chunk_len, uint32_t* d_chunk_file, uint64_t* d_keys,
                    uint8_t* d_digests32, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  const CdcParams p = chunk_params(params);
  uint64_t slots = 0;
  if (int rc = chunk_args(c, "dev_chunk", d_offsets, d_lens, n, p, max_chunks, max_slots, &slots)) return rc;
  if (n && !d_blob) return c->fail(SDCAS_E_INVALID, "dev_chunk: null blob");
  if (((uintptr_t)d_blob | (uintptr_t)d_digests32) & 15)
    return c->fail(SDCAS_E_INVALID, "dev_chunk: blob or digests not 16-byte aligned");
  if ((((uintptr_t)d_offsets | (uintptr_t)d_lens | (uintptr_t)d_file_chunks | (uintptr_t)d_chunk_off |
        (uintptr_t)d_chunk_len | (uintptr_t)d_keys | (uintptr_t)d_counts) & 7) || ((uintptr_t)d_chunk_file & 3))
    return c->fail(SDCAS_E_INVALID, "dev_chunk: an array is not 8-byte (chunk_file: 4-byte) aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (n == 0) {
    hipError_t e;
    if ((d_counts && (e = hipMemsetAsync(d_counts, 0, kCdcCounts * sizeof(uint64_t), call.st))) ||
        (d_file_chunks && (e = hipMemsetAsync(d_file_chunks, 0, sizeof(uint64_t), call.st))))
      return c->hip_fail(e, "dev_chunk");
    return SDCAS_OK;
  }
  return chunk_enqueue(c, "dev_chunk",
                       CdcArgs{nullptr, d_blob, d_offsets, d_lens, (uint32_t)n, p, max_chunks, slots, d_file_chunks,
                               d_chunk_off, d_chunk_len, d_chunk_file},
                       d_keys, d_digests32, d_counts, call.st);
}

// the segment length of a windows call (SDCAS_CHUNK_SEG_BYTES, read per call)
static uint64_t chunk_seg(const CdcParams& p) {
  const char* v = getenv("SDCAS_CHUNK_SEG_BYTES");
  return cdc_seg_bytes(p, v ? strtoull(v, nullptr, 10) : 0);
}

uint64_t sdcas_chunk_seg_bytes(const sdcas_chunk_params* params) {
  const CdcParams p = chunk_params(params);
  return cdc_params_valid(p) ? chunk_seg(p) : 0;
}

// sdcas_chunk_messages (windows false: final and out_consumed are null) and
// sdcas_chunk_windows over host arrays
static int chunk_host(sdcas_ctx* c, const char* who, bool windows, const uint8_t* blob, const uint64_t* offsets,
                      const uint64_t* lens, const uint8_t* final, size_t n, const sdcas_chunk_params* params,
                      uint64_t* out_file_chunks, uint64_t* out_chunk_off, uint64_t* out_chunk_len,
                      uint32_t* out_chunk_file, uint64_t* out_keys, uint8_t* out_digests32, uint64_t* out_consumed,
                      sdcas_chunk_counts* out_counts) {
  static_assert(sizeof(sdcas_chunk_counts) == kCdcCounts * sizeof(uint64_t), "six u64 counts");
  if (!c) return SDCAS_E_INVALID;
  const CdcParams p = chunk_params(params);
  if (!cdc_params_valid(p)) return c->fail(SDCAS_E_INVALID, "%s: invalid chunk parameters", who);
  if (n && (!offsets || !lens)) return c->fail(SDCAS_E_INVALID, "%s: null offsets or lens", who);
  uint64_t max_chunks = 0, max_slots = 0, slots = 0;
  if (cdc_plan(lens, n, p, &max_chunks, &max_slots) != kCdcOk)
    return c->fail(SDCAS_E_CAPACITY, "%s: more than 2^30 chunks", who);
  // every file at a 16-byte aligned place of the device copy, 64 readable bytes behind it
  std::vector<uint64_t> at(n);
  uint64_t bytes = 0, content = 0;
  for (size_t i = 0; i < n; ++i) {
    at[i] = bytes;
    bytes += (lens[i] + kSlack + 15) & ~15ull;
    content += lens[i];
  }
  if (content && !blob) return c->fail(SDCAS_E_INVALID, "%s: null blob", who);
  if (int rc = chunk_args(c, who, offsets, lens, n, p, max_chunks, max_slots, &slots)) return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  if (n == 0) {
    if (out_file_chunks) out_file_chunks[0] = 0;
    return SDCAS_OK;
  }
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipError_t e;
  hipStream_t st = call.st;
  const uint64_t mc = max_chunks;
  sdcas_chunk_counts cts;
  Parts pt(c, st, who);
  const auto d_blob = pt.room<uint8_t>(bytes);
  const auto d_offs = pt.in(at.data(), n);
  const auto d_lens = pt.in(lens, n);
  const auto d_final = pt.in(final, n);
  const auto d_fc = pt.out(out_file_chunks, n + 1, true);
  const auto d_off = pt.out(out_chunk_off, mc, true);
  const auto d_len = pt.out(out_chunk_len, mc, true);
  const auto d_file = pt.out(out_chunk_file, mc, true);
  const auto d_keys = pt.out(out_keys, mc);
  const auto d_digests = pt.out(out_digests32, 32 * mc);
  const auto d_consumed = pt.out(out_consumed, n, windows);
  const auto d_cts = pt.out(&cts, 1);
  if (int rc = pt.reserve()) return rc;
  {
    // the files, packed on the host, in one upload
    std::vector<uint8_t> img(bytes, 0);
    for (size_t i = 0; i < n; ++i)
      if (lens[i]) memcpy(img.data() + at[i], blob + offsets[i], lens[i]);
    if ((e = hipMemcpyAsync(d_blob, img.data(), bytes, hipMemcpyHostToDevice, st))) return hip_fail_at(c, e, who, " H2D");
    if (int rc = pt.upload()) return rc;
    if (int rc = pt.sync(" H2D")) return rc;
  }
  const CdcWinArgs win{d_final, d_consumed, windows ? chunk_seg(p) : 0};
  const CdcArgs a{nullptr, d_blob, d_offs, d_lens, (uint32_t)n, p, max_chunks, slots, d_fc, d_off, d_len, d_file};
  if (int rc = chunk_enqueue(c, who, a, d_keys, d_digests, d_cts.as<uint64_t>(), st, windows ? &win : nullptr))
    return rc;
  if (int rc = pt.counts(d_cts)) return rc;
  const uint64_t m = cts.chunks;
  if (m > mc) return c->fail(SDCAS_E_HIP, "%s: counts out of range", who);
  d_off.first(m), d_len.first(m), d_file.first(m), d_keys.first(m), d_digests.first(32 * m);
  std::vector<uint32_t> file(out_chunk_off ? m : 0);
  if (int rc = pt.fetch(file.data(), d_file, file.size())) return rc;
  if (int rc = pt.download()) return rc;
  // offsets in the caller's blob, not in the device copy
  if (out_chunk_off)
    for (uint64_t k = 0; k < m; ++k)
      if (file[k] < n) out_chunk_off[k] = out_chunk_off[k] - at[file[k]] + offsets[file[k]];
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

int sdcas_chunk_messages(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* lens, size_t n,
                         const sdcas_chunk_params* params, uint64_t* out_file_chunks, uint64_t* out_chunk_off,
                         uint64_t* out_chunk_len, uint32_t* out_chunk_file, uint64_t* out_keys, uint8_t* out_digests32,
                         sdcas_chunk_counts* out_counts) {
  return chunk_host(c, "chunk_messages", false, blob, offsets, lens, nullptr, n, params, out_file_chunks, out_chunk_off,
                    out_chunk_len, out_chunk_file, out_keys, out_digests32, nullptr, out_counts);
}

int sdcas_chunk_windows(sdcas_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* lens,
                        const uint8_t* final, size_t n, const sdcas_chunk_params* params, uint64_t* out_file_chunks,
                        uint64_t* out_chunk_off, uint64_t* out_chunk_len, uint32_t* out_chunk_file, uint64_t* out_keys,
                        uint8_t* out_digests32, uint64_t* out_consumed, sdcas_chunk_counts* out_counts) {
  return chunk_host(c, "chunk_windows", true, blob, offsets, lens, final, n, params, out_file_chunks, out_chunk_off,
                    out_chunk_len, out_chunk_file, out_keys, out_digests32, out_consumed, out_counts);
}

int sdcas_dev_chunk_windows(sdcas_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, const uint64_t* d_lens,
                            const uint8_t* d_final, size_t n, const sdcas_chunk_params* params, uint64_t max_chunks,
                            uint64_t max_slots, uint64_t* d_file_chunks, uint64_t* d_chunk_off, uint64_t* d_chunk_len,
                            uint32_t* d_chunk_file, uint64_t* d_keys, uint8_t* d_digests32, uint64_t* d_consumed,
                            uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  const CdcParams p = chunk_params(params);
  uint64_t slots = 0;
  if (int rc = chunk_args(c, "dev_chunk_windows", d_offsets, d_lens, n, p, max_chunks, max_slots, &slots)) return rc;
  if (n && !d_blob) return c->fail(SDCAS_E_INVALID, "dev_chunk_windows: null blob");
  if (((uintptr_t)d_blob | (uintptr_t)d_digests32) & 15)
    return c->fail(SDCAS_E_INVALID, "dev_chunk_windows: blob or digests not 16-byte aligned");
  if ((((uintptr_t)d_offsets | (uintptr_t)d_lens | (uintptr_t)d_file_chunks | (uintptr_t)d_chunk_off |
        (uintptr_t)d_chunk_len | (uintptr_t)d_keys | (uintptr_t)d_consumed | (uintptr_t)d_counts) & 7) ||
      ((uintptr_t)d_chunk_file & 3))
    return c->fail(SDCAS_E_INVALID, "dev_chunk_windows: an array is not 8-byte (chunk_file: 4-byte) aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (n == 0) {
    hipError_t e;
    if ((d_counts && (e = hipMemsetAsync(d_counts, 0, kCdcCounts * sizeof(uint64_t), call.st))) ||
        (d_file_chunks && (e = hipMemsetAsync(d_file_chunks, 0, sizeof(uint64_t), call.st))))
      return c->hip_fail(e, "dev_chunk_windows");
    return SDCAS_OK;
  }
  const CdcWinArgs win{d_final, d_consumed, chunk_seg(p)};
  return chunk_enqueue(c, "dev_chunk_windows",
                       CdcArgs{nullptr, d_blob, d_offsets, d_lens, (uint32_t)n, p, max_chunks, slots, d_file_chunks,
                               d_chunk_off, d_chunk_len, d_chunk_file},
                       d_keys, d_digests32, d_counts, call.st, &win);
}

static int sharing_args(sdcas_ctx* c, const char* who, const void* chunk_file, const void* chunk_len, const void* rep,
                        size_t m, size_t n_files) {
  if (m > kCdcMaxChunks) return c->fail(SDCAS_E_CAPACITY, "%s of %zu chunks exceeds 2^30", who, m);
  if (n_files >= 0xFFFFFFFFull) return c->fail(SDCAS_E_CAPACITY, "%s of %zu files exceeds 2^32 - 2", who, n_files);
  if (m && (!chunk_file || !chunk_len || !rep)) return c->fail(SDCAS_E_INVALID, "%s: null chunk_file, chunk_len or rep", who);
  return SDCAS_OK;
}

// the workspace grown to m chunks of n_files files
static int sharing_ws(sdcas_ctx* c, size_t m, size_t n_files, hipStream_t st) {
  return grow_synced(c, c->cs_ws, (size_t)cdc_share_ws_bytes(m, n_files), st, "chunk sharing workspace");
}

int sdcas_dev_chunk_sharing(sdcas_ctx* c, const uint32_t* d_chunk_file, const uint64_t* d_chunk_len,
                            const int64_t* d_rep, size_t m, size_t n_files, uint64_t* d_new_bytes,
                            uint64_t* d_self_bytes, uint64_t* d_other_bytes, int64_t* d_peer, uint64_t* d_peer_bytes,
                            uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  if (int rc = sharing_args(c, "dev_chunk_sharing", d_chunk_file, d_chunk_len, d_rep, m, n_files)) return rc;
  if ((((uintptr_t)d_chunk_len | (uintptr_t)d_rep | (uintptr_t)d_new_bytes | (uintptr_t)d_self_bytes |
        (uintptr_t)d_other_bytes | (uintptr_t)d_peer | (uintptr_t)d_peer_bytes | (uintptr_t)d_counts) & 7) ||
      ((uintptr_t)d_chunk_file & 3))
    return c->fail(SDCAS_E_INVALID, "dev_chunk_sharing: an array is not 8-byte (chunk_file: 4-byte) aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = sharing_ws(c, m, n_files, call.st)) return rc;
  hipError_t e = cdc_sharing(c->cs_ws.p, d_chunk_file, d_chunk_len, d_rep, (uint32_t)m, (uint32_t)n_files, d_new_bytes,
                             d_self_bytes, d_other_bytes, d_peer, d_peer_bytes, (unsigned long long*)d_counts, call.st);
  return e ? c->hip_fail(e, "dev_chunk_sharing") : SDCAS_OK;
}

int sdcas_chunk_sharing(sdcas_ctx* c, const uint32_t* chunk_file, const uint64_t* chunk_len, const int64_t* rep,
                        size_t m, size_t n_files, uint64_t* out_new_bytes, uint64_t* out_self_bytes,
                        uint64_t* out_other_bytes, int64_t* out_peer, uint64_t* out_peer_bytes,
                        sdcas_sharing_counts* out_counts) {
  static_assert(sizeof(sdcas_sharing_counts) == kCdcCounts * sizeof(uint64_t), "six u64 counts");
  if (!c) return SDCAS_E_INVALID;
  if (int rc = sharing_args(c, "chunk_sharing", chunk_file, chunk_len, rep, m, n_files)) return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t nf = n_files;
  Parts p(c, st, "chunk_sharing");
  const auto d_file = p.in(chunk_file, m);
  const auto d_len = p.in(chunk_len, m);
  const auto d_rep = p.in(rep, m);
  const auto d_new = p.out(out_new_bytes, nf, true);
  const auto d_self = p.out(out_self_bytes, nf, true);
  const auto d_other = p.out(out_other_bytes, nf, true);
  const auto d_peer = p.out(out_peer, nf, true);
  const auto d_pb = p.out(out_peer_bytes, nf, true);
  const auto d_cts = p.out(out_counts, 1, true);
  if (int rc = p.reserve()) return rc;
  if (int rc = sharing_ws(c, m, n_files, st)) return rc;
  if (int rc = p.upload()) return rc;
  if (hipError_t e = cdc_sharing(c->cs_ws.p, d_file, d_len, d_rep, (uint32_t)m, (uint32_t)n_files, d_new, d_self,
                                 d_other, d_peer, d_pb, d_cts.as<unsigned long long>(), st))
    return c->hip_fail(e, "chunk_sharing");
  return p.download();
}

// ---- the chunk index (chunk_index.hip) ----------------------------------------------

uint32_t sdcas_chunk_index_dir_bits(uint64_t n) { return index_dir_bits(n); }

int sdcas_chunk_index_check(const uint64_t* keys, const uint8_t* digests32, const uint32_t* dir, uint64_t n,
                            uint32_t bits, uint64_t* out_first_bad) {
  static_assert(SDCAS_INDEX_MAX_ENTRIES == kIndexMaxEntries && SDCAS_INDEX_MAX_BITS == kIndexMaxBits, "index limits");
  if (n > kIndexMaxEntries || bits > kIndexMaxBits) return SDCAS_E_CAPACITY;
  if (!dir || (n && (!keys || !digests32))) return SDCAS_E_INVALID;
  uint64_t bad = 0;
  if (index_check(keys, digests32, dir, n, bits, &bad)) {
    if (out_first_bad) *out_first_bad = bad;
    return SDCAS_E_INVALID;
  }
  return SDCAS_OK;
}

// an index argument (host or device): its limits, and the arrays a lookup reads
static int index_view_args(sdcas_ctx* c, const char* who, const void* keys, const void* digests, const void* dir,
                           uint64_t n, uint32_t bits) {
  if (n > kIndexMaxEntries) return c->fail(SDCAS_E_CAPACITY, "%s: an index of %llu entries exceeds 2^30", who, (unsigned long long)n);
  if (bits > kIndexMaxBits) return c->fail(SDCAS_E_CAPACITY, "%s: a directory of %u bits exceeds 28", who, bits);
  if (n && (!keys || !digests || !dir)) return c->fail(SDCAS_E_INVALID, "%s: null index keys, digests or directory", who);
  return SDCAS_OK;
}
static int index_batch_args(sdcas_ctx* c, const char* who, const void* keys, const void* digests, size_t m) {
  if (m > kIndexMaxEntries) return c->fail(SDCAS_E_CAPACITY, "%s: a batch of %zu exceeds 2^30", who, m);
  if (m && (!keys || !digests)) return c->fail(SDCAS_E_INVALID, "%s: null keys or digests", who);
  return SDCAS_OK;
}
static bool index_ranges_meet(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}
// the add's arguments: limits, the arrays it needs, old against new
static int index_add_args(sdcas_ctx* c, const char* who, const void* old_keys, const void* old_digests,
                          const void* old_values, const void* old_dir, uint64_t n_old, uint32_t bits_old,
                          const void* keys, const void* digests, size_t m, const void* new_keys,
                          const void* new_digests, const void* new_values, const void* new_dir, uint32_t bits_new) {
  if (int rc = index_view_args(c, who, old_keys, old_digests, old_dir, n_old, bits_old)) return rc;
  if (int rc = index_batch_args(c, who, keys, digests, m)) return rc;
  if (bits_new > kIndexMaxBits) return c->fail(SDCAS_E_CAPACITY, "%s: a directory of %u bits exceeds 28", who, bits_new);
  const uint64_t cap = n_old + m;
  if (cap > kIndexMaxEntries) return c->fail(SDCAS_E_CAPACITY, "%s: %llu old entries and a batch of %zu exceed 2^30", who, (unsigned long long)n_old, m);
  if (!new_dir || (cap && (!new_keys || !new_digests || !new_values)))
    return c->fail(SDCAS_E_INVALID, "%s: null array of the new index", who);
  const void* o[4] = {old_keys, old_digests, old_values, old_dir};
  const uint64_t ob[4] = {8 * n_old, 32 * n_old, 8 * n_old, n_old ? 4 * index_dir_slots(bits_old) : 0};
  const void* w[4] = {new_keys, new_digests, new_values, new_dir};
  const uint64_t wb[4] = {8 * cap, 32 * cap, 8 * cap, 4 * index_dir_slots(bits_new)};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      if (index_ranges_meet(o[i], ob[i], w[j], wb[j]))
        return c->fail(SDCAS_E_INVALID, "%s: the old and the new index overlap", who);
  return SDCAS_OK;
}

// The chunk index holds pairs, the holders index (chunk_holders.hip) triples:
// every add and match entry point of the two is one body, told which by this.
enum IndexKind { kPairs, kTriples };

static int holders_ws(sdcas_ctx* c, size_t need, hipStream_t st) {
  return grow_synced(c, c->ch_ws, need, st, "chunk holders workspace");
}
// the add's workspace (for pairs the group-by's too) grown to a batch of m
static int index_add_ws(sdcas_ctx* c, IndexKind kind, size_t m, hipStream_t st) {
  if (kind == kTriples) return holders_ws(c, (size_t)holders_add_layout(m).bytes, st);
  if (int rc = grow_synced(c, c->ci_ws, (size_t)index_add_layout(m).bytes, st, "chunk index workspace")) return rc;
  return m ? confirm_ws(c, m, st) : SDCAS_OK;
}
static hipError_t index_add_kind(sdcas_ctx* c, IndexKind kind, const IndexView& old, const uint64_t* keys,
                                 const uint8_t* digests, const uint64_t* values, const uint8_t* valid, uint32_t m,
                                 const IndexOut& out, int64_t* pos, uint8_t* flags, unsigned long long* counts,
                                 hipStream_t st) {
  if (kind == kTriples)
    return holders_add(c->ch_ws.p, old, keys, digests, values, valid, m, out, pos, flags, counts, st);
  return index_add(c->ci_ws.p, c->cf_ws.p, old, keys, digests, values, valid, m, out, pos, flags, counts, st);
}
static hipError_t index_match_kind(IndexKind kind, const IndexView& v, const uint64_t* keys, const uint8_t* digests,
                                   const uint8_t* valid, uint32_t m, int64_t* pos, uint64_t* value, uint32_t* holders,
                                   unsigned long long* counts, hipStream_t st) {
  if (kind == kTriples) return holders_match(v, keys, digests, valid, m, pos, value, holders, counts, st);
  return index_match(v, keys, digests, valid, m, pos, value, counts, st);
}

// a pointer of the first group off 16 bytes, of the second off 8, of the third
// off 4 (a null pointer passes)
static bool index_misaligned(std::initializer_list<const void*> p16, std::initializer_list<const void*> p8,
                             std::initializer_list<const void*> p4) {
  uintptr_t a = 0, b = 0, d = 0;
  for (const void* p : p16) a |= (uintptr_t)p;
  for (const void* p : p8) b |= (uintptr_t)p;
  for (const void* p : p4) d |= (uintptr_t)p;
  return (a & 15) || (b & 7) || (d & 3);
}

namespace {
// a host index a call reads, among the call's parts
struct IndexIn {
  Parts::Part<const uint64_t> k;
  Parts::Part<const uint8_t> d;
  Parts::Part<const uint64_t> v;
  Parts::Part<const uint32_t> dir;
  uint32_t n, bits;
  IndexView view() const { return IndexView{k, d, v, dir, n, bits}; }
};
// the index of up to `cap` entries a call writes
struct IndexNew {
  Parts::Part<uint64_t> k;
  Parts::Part<uint8_t> d;
  Parts::Part<uint64_t> v;
  Parts::Part<uint32_t> dir;
  uint32_t bits;
  IndexOut out() const { return IndexOut{k, d, v, dir, bits}; }
  // nn entries come down (the directory whole)
  void first(size_t nn) const { k.first(nn), d.first(32 * nn), v.first(nn); }
};
}  // namespace

// (an index of no entries is read without its directory)
static IndexIn index_in(Parts& p, const uint64_t* keys, const uint8_t* digests, const uint64_t* values,
                        const uint32_t* dir, size_t n, uint32_t bits) {
  return IndexIn{p.in(keys, n), p.in(digests, 32 * n), p.in(values, n),
                 p.in(dir, n ? (size_t)index_dir_slots(bits) : 0), (uint32_t)n, bits};
}
static IndexNew index_new(Parts& p, uint64_t* keys, uint8_t* digests, uint64_t* values, uint32_t* dir, size_t cap,
                          uint32_t bits) {
  return IndexNew{p.out(keys, cap), p.out(digests, 32 * cap), p.out(values, cap),
                  p.out(dir, (size_t)index_dir_slots(bits)), bits};
}

static int index_dev_match(sdcas_ctx* c, IndexKind kind, const char* who, const uint64_t* d_idx_keys,
                           const uint8_t* d_idx_digests32, const uint64_t* d_idx_values, const uint32_t* d_idx_dir,
                           uint64_t n, uint32_t bits, const uint64_t* d_keys, const uint8_t* d_digests32,
                           const uint8_t* d_valid, size_t m, int64_t* d_out_pos, uint64_t* d_out_value,
                           uint32_t* d_out_holders, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  if (int rc = index_view_args(c, who, d_idx_keys, d_idx_digests32, d_idx_dir, n, bits)) return rc;
  if (int rc = index_batch_args(c, who, d_keys, d_digests32, m)) return rc;
  if (index_misaligned({d_idx_digests32, d_digests32},
                       {d_idx_keys, d_idx_values, d_keys, d_out_pos, d_out_value, d_counts},
                       {d_idx_dir, d_out_holders}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (digests 16 B, %s 4 B, others 8 B)", who,
                   kind == kTriples ? "directory and holders" : "directory");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e;
  if (m == 0) {
    if (d_counts && (e = hipMemsetAsync(d_counts, 0, kIndexMatchCounts * sizeof(uint64_t), call.st)))
      return c->hip_fail(e, "counts");
    return SDCAS_OK;
  }
  const IndexView v{d_idx_keys, d_idx_digests32, d_idx_values, d_idx_dir, (uint32_t)n, bits};
  e = index_match_kind(kind, v, d_keys, d_digests32, d_valid, (uint32_t)m, d_out_pos, d_out_value, d_out_holders,
                       (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

static int index_host_match(sdcas_ctx* c, IndexKind kind, const char* who, const uint64_t* idx_keys,
                            const uint8_t* idx_digests32, const uint64_t* idx_values, const uint32_t* idx_dir,
                            uint64_t n, uint32_t bits, const uint64_t* keys, const uint8_t* digests32,
                            const uint8_t* valid, size_t m, int64_t* out_pos, uint64_t* out_value,
                            uint32_t* out_holders, sdcas_index_match_counts* out_counts) {
  static_assert(sizeof(sdcas_index_match_counts) == kIndexMatchCounts * sizeof(uint64_t), "four u64 counts");
  if (!c) return SDCAS_E_INVALID;
  if (int rc = index_view_args(c, who, idx_keys, idx_digests32, idx_dir, n, bits)) return rc;
  if (int rc = index_batch_args(c, who, keys, digests32, m)) return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  if (m == 0) return SDCAS_OK;
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  Parts p(c, st, who);
  const IndexIn idx = index_in(p, idx_keys, idx_digests32, idx_values, idx_dir, n, bits);
  const auto d_keys = p.in(keys, m);
  const auto d_digests = p.in(digests32, 32 * m);
  const auto d_valid = p.in(valid, m);
  const auto d_pos = p.out(out_pos, m);
  const auto d_value = p.out(out_value, m);
  const auto d_holders = p.out(out_holders, m);
  const auto d_cts = p.out(out_counts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = p.upload()) return rc;
  if (hipError_t e = index_match_kind(kind, idx.view(), d_keys, d_digests, d_valid, (uint32_t)m, d_pos, d_value,
                                      d_holders, d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  return p.download();
}

static int index_dev_add(sdcas_ctx* c, IndexKind kind, const char* who, const uint64_t* d_old_keys,
                         const uint8_t* d_old_digests32, const uint64_t* d_old_values, const uint32_t* d_old_dir,
                         uint64_t n_old, uint32_t bits_old, const uint64_t* d_keys, const uint8_t* d_digests32,
                         const uint64_t* d_values, const uint8_t* d_valid, size_t m, uint64_t* d_new_keys,
                         uint8_t* d_new_digests32, uint64_t* d_new_values, uint32_t* d_new_dir, uint32_t bits_new,
                         int64_t* d_out_pos, uint8_t* d_out_flags, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  if (int rc = index_add_args(c, who, d_old_keys, d_old_digests32, d_old_values, d_old_dir, n_old, bits_old, d_keys,
                              d_digests32, m, d_new_keys, d_new_digests32, d_new_values, d_new_dir, bits_new))
    return rc;
  if (index_misaligned({d_old_digests32, d_digests32, d_new_digests32},
                       {d_old_keys, d_old_values, d_keys, d_values, d_new_keys, d_new_values, d_out_pos, d_counts},
                       {d_old_dir, d_new_dir}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (digests 16 B, directories 4 B, others 8 B)", who);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = index_add_ws(c, kind, m, call.st)) return rc;
  const IndexView old{d_old_keys, d_old_digests32, d_old_values, d_old_dir, (uint32_t)n_old, bits_old};
  const IndexOut out{d_new_keys, d_new_digests32, d_new_values, d_new_dir, bits_new};
  hipError_t e = index_add_kind(c, kind, old, d_keys, d_digests32, d_values, d_valid, (uint32_t)m, out, d_out_pos,
                                d_out_flags, (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

static int index_host_add(sdcas_ctx* c, IndexKind kind, const char* who, const uint64_t* old_keys,
                          const uint8_t* old_digests32, const uint64_t* old_values, const uint32_t* old_dir,
                          uint64_t n_old, uint32_t bits_old, const uint64_t* keys, const uint8_t* digests32,
                          const uint64_t* values, const uint8_t* valid, size_t m, uint64_t* new_keys,
                          uint8_t* new_digests32, uint64_t* new_values, uint32_t* new_dir, uint32_t bits_new,
                          int64_t* out_pos, uint8_t* out_flags, sdcas_index_add_counts* out_counts) {
  static_assert(sizeof(sdcas_index_add_counts) == kIndexAddCounts * sizeof(uint64_t), "six u64 counts");
  if (!c) return SDCAS_E_INVALID;
  if (int rc = index_add_args(c, who, old_keys, old_digests32, old_values, old_dir, n_old, bits_old, keys, digests32,
                              m, new_keys, new_digests32, new_values, new_dir, bits_new))
    return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t cap = n_old + m;
  sdcas_index_add_counts cts;
  Parts p(c, st, who);
  const IndexIn old = index_in(p, old_keys, old_digests32, old_values, old_dir, n_old, bits_old);
  const auto d_keys = p.in(keys, m);
  const auto d_digests = p.in(digests32, 32 * m);
  const auto d_values = p.in(values, m);
  const auto d_valid = p.in(valid, m);
  const IndexNew nw = index_new(p, new_keys, new_digests32, new_values, new_dir, cap, bits_new);
  const auto d_pos = p.out(out_pos, m);
  const auto d_flags = p.out(out_flags, m);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = index_add_ws(c, kind, m, st)) return rc;
  if (int rc = p.upload()) return rc;
  if (hipError_t e = index_add_kind(c, kind, old.view(), d_keys, d_digests, d_values, d_valid, (uint32_t)m, nw.out(),
                                    d_pos, d_flags, d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.counts(d_cts)) return rc;
  if (cts.entries_new > cap) return c->fail(SDCAS_E_HIP, "%s: counts out of range", who);
  nw.first((size_t)cts.entries_new);
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

int sdcas_dev_chunk_index_match(sdcas_ctx* c, const uint64_t* d_idx_keys, const uint8_t* d_idx_digests32,
                                const uint64_t* d_idx_values, const uint32_t* d_idx_dir, uint64_t n, uint32_t bits,
                                const uint64_t* d_keys, const uint8_t* d_digests32, const uint8_t* d_valid, size_t m,
                                int64_t* d_out_pos, uint64_t* d_out_value, uint64_t* d_counts, void* stream) {
  return index_dev_match(c, kPairs, "dev_chunk_index_match", d_idx_keys, d_idx_digests32, d_idx_values, d_idx_dir, n,
                         bits, d_keys, d_digests32, d_valid, m, d_out_pos, d_out_value, nullptr, d_counts, stream);
}

int sdcas_chunk_index_match(sdcas_ctx* c, const uint64_t* idx_keys, const uint8_t* idx_digests32,
                            const uint64_t* idx_values, const uint32_t* idx_dir, uint64_t n, uint32_t bits,
                            const uint64_t* keys, const uint8_t* digests32, const uint8_t* valid, size_t m,
                            int64_t* out_pos, uint64_t* out_value, sdcas_index_match_counts* out_counts) {
  return index_host_match(c, kPairs, "chunk_index_match", idx_keys, idx_digests32, idx_values, idx_dir, n, bits, keys,
                          digests32, valid, m, out_pos, out_value, nullptr, out_counts);
}

int sdcas_dev_chunk_index_add(sdcas_ctx* c, const uint64_t* d_old_keys, const uint8_t* d_old_digests32,
                              const uint64_t* d_old_values, const uint32_t* d_old_dir, uint64_t n_old,
                              uint32_t bits_old, const uint64_t* d_keys, const uint8_t* d_digests32,
                              const uint64_t* d_values, const uint8_t* d_valid, size_t m, uint64_t* d_new_keys,
                              uint8_t* d_new_digests32, uint64_t* d_new_values, uint32_t* d_new_dir,
                              uint32_t bits_new, int64_t* d_out_pos, uint8_t* d_out_flags, uint64_t* d_counts,
                              void* stream) {
  return index_dev_add(c, kPairs, "dev_chunk_index_add", d_old_keys, d_old_digests32, d_old_values, d_old_dir, n_old,
                       bits_old, d_keys, d_digests32, d_values, d_valid, m, d_new_keys, d_new_digests32, d_new_values,
                       d_new_dir, bits_new, d_out_pos, d_out_flags, d_counts, stream);
}

int sdcas_chunk_index_add(sdcas_ctx* c, const uint64_t* old_keys, const uint8_t* old_digests32,
                          const uint64_t* old_values, const uint32_t* old_dir, uint64_t n_old, uint32_t bits_old,
                          const uint64_t* keys, const uint8_t* digests32, const uint64_t* values,
                          const uint8_t* valid, size_t m, uint64_t* new_keys, uint8_t* new_digests32,
                          uint64_t* new_values, uint32_t* new_dir, uint32_t bits_new, int64_t* out_pos,
                          uint8_t* out_flags, sdcas_index_add_counts* out_counts) {
  return index_host_add(c, kPairs, "chunk_index_add", old_keys, old_digests32, old_values, old_dir, n_old, bits_old,
                        keys, digests32, values, valid, m, new_keys, new_digests32, new_values, new_dir, bits_new,
                        out_pos, out_flags, out_counts);
}

// ---- the holders index (chunk_holders.hip) --------------------------------------------

int sdcas_chunk_holders_check(const uint64_t* keys, const uint8_t* digests32, const uint64_t* values,
                              const uint32_t* dir, uint64_t n, uint32_t bits, uint64_t* out_first_bad) {
  if (n > kIndexMaxEntries || bits > kIndexMaxBits) return SDCAS_E_CAPACITY;
  if (!dir || (n && (!keys || !digests32))) return SDCAS_E_INVALID;
  uint64_t bad = 0;
  if (holders_check(keys, digests32, values, dir, n, bits, &bad)) {
    if (out_first_bad) *out_first_bad = bad;
    return SDCAS_E_INVALID;
  }
  return SDCAS_OK;
}

// the remove's arguments: limits, the arrays it needs, old and removed against new
static int holders_remove_args(sdcas_ctx* c, const char* who, const void* old_keys, const void* old_digests,
                               const void* old_values, const void* old_dir, uint64_t n_old, uint32_t bits_old,
                               const void* removed, size_t r, const void* new_keys, const void* new_digests,
                               const void* new_values, const void* new_dir, uint32_t bits_new) {
  if (int rc = index_view_args(c, who, old_keys, old_digests, old_dir, n_old, bits_old)) return rc;
  if (bits_new > kIndexMaxBits) return c->fail(SDCAS_E_CAPACITY, "%s: a directory of %u bits exceeds 28", who, bits_new);
  if (r > kIndexMaxEntries) return c->fail(SDCAS_E_CAPACITY, "%s: %zu removed values exceed 2^30", who, r);
  if (r && !removed) return c->fail(SDCAS_E_INVALID, "%s: null removed values", who);
  if (!new_dir || (n_old && (!new_keys || !new_digests || !new_values)))
    return c->fail(SDCAS_E_INVALID, "%s: null array of the new index", who);
  const void* o[5] = {old_keys, old_digests, old_values, old_dir, removed};
  const uint64_t ob[5] = {8 * n_old, 32 * n_old, 8 * n_old, n_old ? 4 * index_dir_slots(bits_old) : 0, 8 * (uint64_t)r};
  const void* w[4] = {new_keys, new_digests, new_values, new_dir};
  const uint64_t wb[4] = {8 * n_old, 32 * n_old, 8 * n_old, 4 * index_dir_slots(bits_new)};
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 4; ++j)
      if (index_ranges_meet(o[i], ob[i], w[j], wb[j]))
        return c->fail(SDCAS_E_INVALID, "%s: the new index overlaps the old one or the removed values", who);
  return SDCAS_OK;
}

int sdcas_dev_chunk_holders_match(sdcas_ctx* c, const uint64_t* d_idx_keys, const uint8_t* d_idx_digests32,
                                  const uint64_t* d_idx_values, const uint32_t* d_idx_dir, uint64_t n, uint32_t bits,
                                  const uint64_t* d_keys, const uint8_t* d_digests32, const uint8_t* d_valid,
                                  size_t m, int64_t* d_out_pos, uint64_t* d_out_value, uint32_t* d_out_holders,
                                  uint64_t* d_counts, void* stream) {
  return index_dev_match(c, kTriples, "dev_chunk_holders_match", d_idx_keys, d_idx_digests32, d_idx_values, d_idx_dir,
                         n, bits, d_keys, d_digests32, d_valid, m, d_out_pos, d_out_value, d_out_holders, d_counts,
                         stream);
}

int sdcas_chunk_holders_match(sdcas_ctx* c, const uint64_t* idx_keys, const uint8_t* idx_digests32,
                              const uint64_t* idx_values, const uint32_t* idx_dir, uint64_t n, uint32_t bits,
                              const uint64_t* keys, const uint8_t* digests32, const uint8_t* valid, size_t m,
                              int64_t* out_pos, uint64_t* out_value, uint32_t* out_holders,
                              sdcas_index_match_counts* out_counts) {
  return index_host_match(c, kTriples, "chunk_holders_match", idx_keys, idx_digests32, idx_values, idx_dir, n, bits,
                          keys, digests32, valid, m, out_pos, out_value, out_holders, out_counts);
}

int sdcas_dev_chunk_holders_add(sdcas_ctx* c, const uint64_t* d_old_keys, const uint8_t* d_old_digests32,
                                const uint64_t* d_old_values, const uint32_t* d_old_dir, uint64_t n_old,
                                uint32_t bits_old, const uint64_t* d_keys, const uint8_t* d_digests32,
                                const uint64_t* d_values, const uint8_t* d_valid, size_t m, uint64_t* d_new_keys,
                                uint8_t* d_new_digests32, uint64_t* d_new_values, uint32_t* d_new_dir,
                                uint32_t bits_new, int64_t* d_out_pos, uint8_t* d_out_flags, uint64_t* d_counts,
                                void* stream) {
  return index_dev_add(c, kTriples, "dev_chunk_holders_add", d_old_keys, d_old_digests32, d_old_values, d_old_dir,
                       n_old, bits_old, d_keys, d_digests32, d_values, d_valid, m, d_new_keys, d_new_digests32,
                       d_new_values, d_new_dir, bits_new, d_out_pos, d_out_flags, d_counts, stream);
}

int sdcas_chunk_holders_add(sdcas_ctx* c, const uint64_t* old_keys, const uint8_t* old_digests32,
                            const uint64_t* old_values, const uint32_t* old_dir, uint64_t n_old, uint32_t bits_old,
                            const uint64_t* keys, const uint8_t* digests32, const uint64_t* values,
                            const uint8_t* valid, size_t m, uint64_t* new_keys, uint8_t* new_digests32,
                            uint64_t* new_values, uint32_t* new_dir, uint32_t bits_new, int64_t* out_pos,
                            uint8_t* out_flags, sdcas_index_add_counts* out_counts) {
  return index_host_add(c, kTriples, "chunk_holders_add", old_keys, old_digests32, old_values, old_dir, n_old,
                        bits_old, keys, digests32, values, valid, m, new_keys, new_digests32, new_values, new_dir,
                        bits_new, out_pos, out_flags, out_counts);
}

int sdcas_dev_chunk_holders_remove(sdcas_ctx* c, const uint64_t* d_old_keys, const uint8_t* d_old_digests32,
                                   const uint64_t* d_old_values, const uint32_t* d_old_dir, uint64_t n_old,
                                   uint32_t bits_old, const uint64_t* d_removed, size_t r, uint64_t* d_new_keys,
                                   uint8_t* d_new_digests32, uint64_t* d_new_values, uint32_t* d_new_dir,
                                   uint32_t bits_new, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  if (int rc = holders_remove_args(c, "dev_chunk_holders_remove", d_old_keys, d_old_digests32, d_old_values, d_old_dir,
                                   n_old, bits_old, d_removed, r, d_new_keys, d_new_digests32, d_new_values, d_new_dir,
                                   bits_new))
    return rc;
  if (index_misaligned({d_old_digests32, d_new_digests32},
                       {d_old_keys, d_old_values, d_removed, d_new_keys, d_new_values, d_counts},
                       {d_old_dir, d_new_dir}))
    return c->fail(SDCAS_E_INVALID, "dev_chunk_holders_remove: an array is misaligned (digests 16 B, directories 4 B, others 8 B)");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = holders_ws(c, (size_t)holders_remove_layout(n_old).bytes, call.st)) return rc;
  const IndexView old{d_old_keys, d_old_digests32, d_old_values, d_old_dir, (uint32_t)n_old, bits_old};
  const IndexOut out{d_new_keys, d_new_digests32, d_new_values, d_new_dir, bits_new};
  hipError_t e = holders_remove(c->ch_ws.p, old, d_removed, (uint32_t)r, out, (unsigned long long*)d_counts, call.st);
  return e ? c->hip_fail(e, "dev_chunk_holders_remove") : SDCAS_OK;
}

int sdcas_chunk_holders_remove(sdcas_ctx* c, const uint64_t* old_keys, const uint8_t* old_digests32,
                               const uint64_t* old_values, const uint32_t* old_dir, uint64_t n_old,
                               uint32_t bits_old, const uint64_t* removed, size_t r, uint64_t* new_keys,
                               uint8_t* new_digests32, uint64_t* new_values, uint32_t* new_dir, uint32_t bits_new,
                               sdcas_holders_remove_counts* out_counts) {
  static_assert(sizeof(sdcas_holders_remove_counts) == kHoldersRemoveCounts * sizeof(uint64_t), "four u64 counts");
  const char* who = "chunk_holders_remove";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = holders_remove_args(c, who, old_keys, old_digests32, old_values, old_dir, n_old, bits_old, removed, r,
                                   new_keys, new_digests32, new_values, new_dir, bits_new))
    return rc;
  for (size_t i = 1; i < r; ++i)
    if (removed[i - 1] >= removed[i])
      return c->fail(SDCAS_E_INVALID, "chunk_holders_remove: removed value %zu does not ascend", i);
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t n = n_old;
  sdcas_holders_remove_counts cts;
  Parts p(c, st, who);
  const IndexIn old = index_in(p, old_keys, old_digests32, old_values, old_dir, n, bits_old);
  const auto d_removed = p.in(removed, r);
  const IndexNew nw = index_new(p, new_keys, new_digests32, new_values, new_dir, n, bits_new);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = holders_ws(c, (size_t)holders_remove_layout(n).bytes, st)) return rc;
  if (int rc = p.upload()) return rc;
  if (hipError_t e = holders_remove(c->ch_ws.p, old.view(), d_removed, (uint32_t)r, nw.out(),
                                    d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.counts(d_cts)) return rc;
  if (cts.entries_new > n) return c->fail(SDCAS_E_HIP, "%s: counts out of range", who);
  nw.first((size_t)cts.entries_new);
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

// ---- the chunk peers (chunk_peers.hip) ------------------------------------------------

// the request's ranges, GPU-free: SDCAS_OK, or the code with *why set
static int peers_range(uint64_t m, uint64_t n_files, uint32_t k, uint32_t max_holders, uint64_t max_pairs,
                       const char** why) {
  static_assert(SDCAS_PEERS_MAX_K == kPeersMaxK && SDCAS_PEERS_MAX_HOLDERS == kPeersMaxHolders &&
                    SDCAS_PEERS_MAX_PAIRS == kPeersMaxPairs && SDCAS_PEERS_EARLIER == kPeersEarlier &&
                    SDCAS_PEERS_ALL == kPeersAll,
                "peers limits");
  if (k < 1 || k > kPeersMaxK) return *why = "k is not in [1, 64]", SDCAS_E_INVALID;
  if (max_holders < 1 || max_holders > kPeersMaxHolders) return *why = "max_holders is not in [1, 2^20]", SDCAS_E_INVALID;
  if (m > kIndexMaxEntries) return *why = "a batch of more than 2^30 chunks", SDCAS_E_CAPACITY;
  if (n_files >= 0xFFFFFFFFull) return *why = "more than 2^32 - 2 files", SDCAS_E_CAPACITY;
  if (max_pairs > kPeersMaxPairs) return *why = "max_pairs exceeds 2^30", SDCAS_E_CAPACITY;
  return SDCAS_OK;
}

int sdcas_chunk_peers_plan(uint64_t m, uint64_t n_files, uint32_t k, uint32_t max_holders, uint64_t* out_max_pairs,
                           uint64_t* out_workspace_bytes) {
  const char* why = nullptr;
  if (int rc = peers_range(m, n_files, k, max_holders, 0, &why)) return rc;
  const uint64_t q = peers_pair_bound(m, max_holders);
  if (out_max_pairs) *out_max_pairs = q;
  if (out_workspace_bytes) *out_workspace_bytes = peers_layout(m, q).bytes;
  return SDCAS_OK;
}

// a call's arguments (host or device arrays): the ranges, then the arrays it needs
static int peers_args(sdcas_ctx* c, const char* who, const void* idx_keys, const void* idx_digests, const void* idx_dir,
                      uint64_t n, uint32_t bits, const void* keys, const void* digests, const void* chunk_file,
                      const void* chunk_len, size_t m, const void* file_ids, size_t n_files, uint32_t k,
                      uint32_t max_holders, uint32_t mode, uint64_t max_pairs) {
  const char* why = nullptr;
  if (mode != kPeersEarlier && mode != kPeersAll) return c->fail(SDCAS_E_INVALID, "%s: unknown mode %u", who, mode);
  if (int rc = peers_range(m, n_files, k, max_holders, max_pairs, &why)) return c->fail(rc, "%s: %s", who, why);
  if (int rc = index_view_args(c, who, idx_keys, idx_digests, idx_dir, n, bits)) return rc;
  if (int rc = index_batch_args(c, who, keys, digests, m)) return rc;
  if (m && (!chunk_file || !chunk_len)) return c->fail(SDCAS_E_INVALID, "%s: null chunk_file or chunk_len", who);
  if (m && n_files && !file_ids) return c->fail(SDCAS_E_INVALID, "%s: null file_ids", who);
  return SDCAS_OK;
}

int sdcas_dev_chunk_peers(sdcas_ctx* c, const uint64_t* d_idx_keys, const uint8_t* d_idx_digests32,
                          const uint64_t* d_idx_values, const uint32_t* d_idx_dir, uint64_t n, uint32_t bits,
                          const uint64_t* d_keys, const uint8_t* d_digests32, const uint8_t* d_valid,
                          const uint32_t* d_chunk_file, const uint64_t* d_chunk_len, size_t m,
                          const uint64_t* d_file_ids, size_t n_files, uint32_t k, uint32_t max_holders, uint32_t mode,
                          uint64_t max_pairs, uint32_t* d_out_peer_count, uint64_t* d_out_peers,
                          uint64_t* d_out_peer_bytes, uint64_t* d_out_shared_bytes, uint64_t* d_out_unique_bytes,
                          uint64_t* d_out_common_bytes, uint64_t* d_counts, void* stream) {
  const char* who = "dev_chunk_peers";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = peers_args(c, who, d_idx_keys, d_idx_digests32, d_idx_dir, n, bits, d_keys, d_digests32, d_chunk_file,
                          d_chunk_len, m, d_file_ids, n_files, k, max_holders, mode, max_pairs))
    return rc;
  if (index_misaligned({d_idx_digests32, d_digests32},
                       {d_idx_keys, d_idx_values, d_keys, d_chunk_len, d_file_ids, d_out_peers, d_out_peer_bytes,
                        d_out_shared_bytes, d_out_unique_bytes, d_out_common_bytes, d_counts},
                       {d_idx_dir, d_chunk_file, d_out_peer_count}))
    return c->fail(SDCAS_E_INVALID,
                   "%s: an array is misaligned (digests 16 B, directory, chunk_file and peer_count 4 B, others 8 B)", who);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->cp_ws, (size_t)peers_layout(m, max_pairs).bytes, call.st, "chunk peers workspace"))
    return rc;
  const IndexView v{d_idx_keys, d_idx_digests32, d_idx_values, d_idx_dir, (uint32_t)n, bits};
  const PeersIn in{d_keys, d_digests32, d_valid, d_chunk_file, d_chunk_len, d_file_ids, (uint32_t)m,
                   (uint32_t)n_files, k, max_holders, mode};
  const PeersOut out{d_out_peer_count, d_out_peers, d_out_peer_bytes, d_out_shared_bytes, d_out_unique_bytes,
                     d_out_common_bytes};
  hipError_t e = chunk_peers(c->cp_ws.p, v, in, (uint32_t)max_pairs, out, (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

int sdcas_chunk_peers(sdcas_ctx* c, const uint64_t* idx_keys, const uint8_t* idx_digests32, const uint64_t* idx_values,
                      const uint32_t* idx_dir, uint64_t n, uint32_t bits, const uint64_t* keys,
                      const uint8_t* digests32, const uint8_t* valid, const uint32_t* chunk_file,
                      const uint64_t* chunk_len, size_t m, const uint64_t* file_ids, size_t n_files, uint32_t k,
                      uint32_t max_holders, uint32_t mode, uint64_t max_pairs, uint32_t* out_peer_count,
                      uint64_t* out_peers, uint64_t* out_peer_bytes, uint64_t* out_shared_bytes,
                      uint64_t* out_unique_bytes, uint64_t* out_common_bytes, sdcas_peers_counts* out_counts) {
  static_assert(sizeof(sdcas_peers_counts) == kPeersCounts * sizeof(uint64_t), "seven u64 counts");
  const char* who = "chunk_peers";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = peers_args(c, who, idx_keys, idx_digests32, idx_dir, n, bits, keys, digests32, chunk_file, chunk_len, m,
                          file_ids, n_files, k, max_holders, mode, max_pairs))
    return rc;
  if (!max_pairs) max_pairs = peers_pair_bound(m, max_holders);
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t nf = n_files;
  sdcas_peers_counts cts;
  Parts p(c, st, who);
  const IndexIn idx = index_in(p, idx_keys, idx_digests32, idx_values, idx_dir, n, bits);
  const auto d_keys = p.in(keys, m);
  const auto d_digests = p.in(digests32, 32 * m);
  const auto d_valid = p.in(valid, m);
  const auto d_file = p.in(chunk_file, m);
  const auto d_len = p.in(chunk_len, m);
  const auto d_ids = p.in(file_ids, nf);
  const auto d_pc = p.out(out_peer_count, nf);
  const auto d_peers = p.out(out_peers, nf * k);
  const auto d_pb = p.out(out_peer_bytes, nf * k);
  const auto d_shared = p.out(out_shared_bytes, nf);
  const auto d_unique = p.out(out_unique_bytes, nf);
  const auto d_common = p.out(out_common_bytes, nf);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->cp_ws, (size_t)peers_layout(m, max_pairs).bytes, st, "chunk peers workspace"))
    return rc;
  if (int rc = p.upload()) return rc;
  const PeersIn in{d_keys, d_digests, d_valid, d_file, d_len, d_ids, (uint32_t)m, (uint32_t)n_files, k, max_holders,
                   mode};
  const PeersOut out{d_pc, d_peers, d_pb, d_shared, d_unique, d_common};
  if (hipError_t e = chunk_peers(c->cp_ws.p, idx.view(), in, (uint32_t)max_pairs, out,
                                 d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  if (cts.overflow)
    return c->fail(SDCAS_E_CAPACITY, "%s: %llu (chunk, holder) pairs exceed max_pairs %llu", who,
                   (unsigned long long)cts.pairs, (unsigned long long)max_pairs);
  return SDCAS_OK;
}

// ---- the file families (families.hip) -------------------------------------------------

// the request's ranges, GPU-free: SDCAS_OK, or the code with *why set
static int families_range(uint64_t n, uint32_t k, const char** why) {
  static_assert(kFamiliesMaxFiles == (1ull << 30) && kFamiliesMaxPasses == 30, "families limits");
  if (k < 1 || k > kPeersMaxK) return *why = "k is not in [1, 64]", SDCAS_E_INVALID;
  if (n > kFamiliesMaxFiles) return *why = "more than 2^30 files", SDCAS_E_CAPACITY;
  return SDCAS_OK;
}

int sdcas_file_families_plan(uint64_t n, uint32_t k, uint64_t* out_workspace_bytes) {
  const char* why = nullptr;
  if (int rc = families_range(n, k, &why)) return rc;
  if (out_workspace_bytes) *out_workspace_bytes = families_layout(n).bytes;
  return SDCAS_OK;
}

// a call's arguments (host or device arrays): the ranges, then the arrays it needs
static int families_args(sdcas_ctx* c, const char* who, const void* ids, const void* sizes, const void* peer_count,
                         const void* peers, const void* peer_bytes, size_t n, uint32_t k, uint32_t num, uint32_t den) {
  const char* why = nullptr;
  if (int rc = families_range(n, k, &why)) return c->fail(rc, "%s: %s", who, why);
  if (den < 1 || num > den) return c->fail(SDCAS_E_INVALID, "%s: the threshold %u / %u is not in [0, 1]", who, num, den);
  if (n && (!ids || !sizes || !peer_count || !peers || !peer_bytes))
    return c->fail(SDCAS_E_INVALID, "%s: null ids, sizes, peer_count, peers or peer_bytes", who);
  return SDCAS_OK;
}

int sdcas_dev_file_families(sdcas_ctx* c, const uint64_t* d_ids, const uint64_t* d_sizes, const uint32_t* d_peer_count,
                            const uint64_t* d_peers, const uint64_t* d_peer_bytes, size_t n, uint32_t k, uint32_t num,
                            uint32_t den, int64_t* d_out_family, uint32_t* d_out_family_size, uint64_t* d_counts,
                            void* stream) {
  const char* who = "dev_file_families";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = families_args(c, who, d_ids, d_sizes, d_peer_count, d_peers, d_peer_bytes, n, k, num, den)) return rc;
  if (index_misaligned({}, {d_ids, d_sizes, d_peers, d_peer_bytes, d_out_family, d_counts},
                       {d_peer_count, d_out_family_size}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (peer_count and family_size 4 B, others 8 B)", who);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->ff_ws, (size_t)families_layout(n).bytes, call.st, "file families workspace")) return rc;
  const FamiliesIn in{d_ids, d_sizes, d_peer_count, d_peers, d_peer_bytes, (uint32_t)n, k, num, den};
  hipError_t e = file_families(c->ff_ws.p, in, d_out_family, d_out_family_size, (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

int sdcas_file_families(sdcas_ctx* c, const uint64_t* ids, const uint64_t* sizes, const uint32_t* peer_count,
                        const uint64_t* peers, const uint64_t* peer_bytes, size_t n, uint32_t k, uint32_t num,
                        uint32_t den, int64_t* out_family, uint32_t* out_family_size,
                        sdcas_families_counts* out_counts) {
  static_assert(sizeof(sdcas_families_counts) == kFamiliesCounts * sizeof(uint64_t), "ten u64 counts");
  const char* who = "file_families";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = families_args(c, who, ids, sizes, peer_count, peers, peer_bytes, n, k, num, den)) return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  // the order the device form checks on the device, here before anything is uploaded
  for (size_t i = 1; i < n; ++i)
    if (!(ids[i - 1] < ids[i])) {
      if (out_counts) out_counts->files = n, out_counts->unsorted = 1;
      return c->fail(SDCAS_E_INVALID, "%s: ids are not strictly ascending at row %zu", who, i);
    }
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  sdcas_families_counts cts;
  Parts p(c, st, who);
  const auto d_ids = p.in(ids, n);
  const auto d_sizes = p.in(sizes, n);
  const auto d_pc = p.in(peer_count, n);
  const auto d_peers = p.in(peers, n * k);
  const auto d_pb = p.in(peer_bytes, n * k);
  const auto d_family = p.out(out_family, n);
  const auto d_fs = p.out(out_family_size, n);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->ff_ws, (size_t)families_layout(n).bytes, st, "file families workspace")) return rc;
  if (int rc = p.upload()) return rc;
  const FamiliesIn in{d_ids, d_sizes, d_pc, d_peers, d_pb, (uint32_t)n, k, num, den};
  if (hipError_t e = file_families(c->ff_ws.p, in, d_family, d_fs, d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

// ---- the family bytes (family_bytes.hip) -----------------------------------------------

// the request's ranges, GPU-free: SDCAS_OK, or the code with *why set
static int family_bytes_range(uint64_t m, uint64_t n_files, const char** why) {
  static_assert(kFamilyBytesMaxChunks == (1ull << 30) && kFamilyBytesMaxFiles == (1ull << 30), "family bytes limits");
  if (m > kFamilyBytesMaxChunks) return *why = "more than 2^30 chunks", SDCAS_E_CAPACITY;
  if (n_files > kFamilyBytesMaxFiles) return *why = "more than 2^30 files", SDCAS_E_CAPACITY;
  return SDCAS_OK;
}

int sdcas_family_bytes_plan(uint64_t m, uint64_t n_files, uint64_t* out_workspace_bytes) {
  const char* why = nullptr;
  if (int rc = family_bytes_range(m, n_files, &why)) return rc;
  if (out_workspace_bytes) *out_workspace_bytes = family_bytes_layout(m, n_files).bytes;
  return SDCAS_OK;
}

// a call's arguments (host or device arrays): the ranges, then the arrays it needs
static int family_bytes_args(sdcas_ctx* c, const char* who, const void* chunk_file, const void* chunk_len,
                             const void* rep, size_t m, const void* family, size_t n_files) {
  const char* why = nullptr;
  if (int rc = family_bytes_range(m, n_files, &why)) return c->fail(rc, "%s: %s", who, why);
  if (m && (!chunk_file || !chunk_len || !rep))
    return c->fail(SDCAS_E_INVALID, "%s: null chunk_file, chunk_len or rep", who);
  if (n_files && !family) return c->fail(SDCAS_E_INVALID, "%s: null family", who);
  return SDCAS_OK;
}

int sdcas_dev_family_bytes(sdcas_ctx* c, const uint32_t* d_chunk_file, const uint64_t* d_chunk_len,
                           const int64_t* d_rep, size_t m, const int64_t* d_family, size_t n_files,
                           uint64_t* d_file_bytes, uint64_t* d_delta_bytes, uint64_t* d_self_bytes,
                           uint64_t* d_inherited_bytes, int64_t* d_set_rep, uint32_t* d_set_files,
                           uint64_t* d_set_total, uint64_t* d_set_stored, uint64_t* d_counts, void* stream) {
  const char* who = "dev_family_bytes";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = family_bytes_args(c, who, d_chunk_file, d_chunk_len, d_rep, m, d_family, n_files)) return rc;
  if (index_misaligned({},
                       {d_chunk_len, d_rep, d_family, d_file_bytes, d_delta_bytes, d_self_bytes, d_inherited_bytes,
                        d_set_rep, d_set_total, d_set_stored, d_counts},
                       {d_chunk_file, d_set_files}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (chunk_file and set_files 4 B, others 8 B)", who);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->fb_ws, (size_t)family_bytes_layout(m, n_files).bytes, call.st,
                           "family bytes workspace"))
    return rc;
  const FamilyBytesIn in{d_chunk_file, d_chunk_len, d_rep, d_family, (uint32_t)m, (uint32_t)n_files};
  const FamilyBytesOut out{d_file_bytes, d_delta_bytes, d_self_bytes, d_inherited_bytes,
                           d_set_rep,    d_set_files,   d_set_total,  d_set_stored};
  hipError_t e = family_bytes(c->fb_ws.p, in, out, (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

int sdcas_family_bytes(sdcas_ctx* c, const uint32_t* chunk_file, const uint64_t* chunk_len, const int64_t* rep,
                       size_t m, const int64_t* family, size_t n_files, uint64_t* out_file_bytes,
                       uint64_t* out_delta_bytes, uint64_t* out_self_bytes, uint64_t* out_inherited_bytes,
                       int64_t* out_set_rep, uint32_t* out_set_files, uint64_t* out_set_total,
                       uint64_t* out_set_stored, sdcas_family_bytes_counts* out_counts) {
  static_assert(sizeof(sdcas_family_bytes_counts) == kFamilyBytesCounts * sizeof(uint64_t), "nine u64 counts");
  const char* who = "family_bytes";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = family_bytes_args(c, who, chunk_file, chunk_len, rep, m, family, n_files)) return rc;
  if (index_misaligned({},
                       {chunk_len, rep, family, out_file_bytes, out_delta_bytes, out_self_bytes, out_inherited_bytes,
                        out_set_rep, out_set_total, out_set_stored, out_counts},
                       {chunk_file, out_set_files}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (chunk_file and set_files 4 B, others 8 B)", who);
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t nf = n_files, h = n_files / 2;  // no more sets than that
  sdcas_family_bytes_counts cts;
  Parts p(c, st, who);
  const auto d_file = p.in(chunk_file, m);
  const auto d_len = p.in(chunk_len, m);
  const auto d_rep = p.in(rep, m);
  const auto d_family = p.in(family, nf);
  const auto d_fb = p.out(out_file_bytes, nf);
  const auto d_delta = p.out(out_delta_bytes, nf);
  const auto d_self = p.out(out_self_bytes, nf);
  const auto d_inh = p.out(out_inherited_bytes, nf);
  const auto d_set_rep = p.out(out_set_rep, h);
  const auto d_set_files = p.out(out_set_files, h);
  const auto d_set_total = p.out(out_set_total, h);
  const auto d_set_stored = p.out(out_set_stored, h);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->fb_ws, (size_t)family_bytes_layout(m, n_files).bytes, st, "family bytes workspace"))
    return rc;
  if (int rc = p.upload()) return rc;
  const FamilyBytesIn in{d_file, d_len, d_rep, d_family, (uint32_t)m, (uint32_t)n_files};
  const FamilyBytesOut out{d_fb, d_delta, d_self, d_inh, d_set_rep, d_set_files, d_set_total, d_set_stored};
  if (hipError_t e = family_bytes(c->fb_ws.p, in, out, d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.counts(d_cts)) return rc;
  if (cts.sets > h || cts.members > nf) return c->fail(SDCAS_E_HIP, "%s: counts out of range", who);
  d_set_rep.first(cts.sets), d_set_files.first(cts.sets), d_set_total.first(cts.sets), d_set_stored.first(cts.sets);
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

// ---- the family recipes (family_recipes.hip) -------------------------------------------

int sdcas_family_recipes_plan(uint64_t m, uint64_t n_files, uint64_t* out_workspace_bytes) {
  const char* why = nullptr;
  if (int rc = family_bytes_range(m, n_files, &why)) return rc;
  if (out_workspace_bytes) *out_workspace_bytes = family_recipes_layout(m, n_files).bytes;
  return SDCAS_OK;
}

// a call's arguments (host or device arrays): family_bytes' and the offsets
static int family_recipes_args(sdcas_ctx* c, const char* who, const void* chunk_file, const void* chunk_off,
                               const void* chunk_len, const void* rep, size_t m, const void* family, size_t n_files) {
  if (int rc = family_bytes_args(c, who, chunk_file, chunk_len, rep, m, family, n_files)) return rc;
  if (m && !chunk_off) return c->fail(SDCAS_E_INVALID, "%s: null chunk_off", who);
  return SDCAS_OK;
}

int sdcas_dev_family_recipes(sdcas_ctx* c, const uint32_t* d_chunk_file, const uint64_t* d_chunk_off,
                             const uint64_t* d_chunk_len, const int64_t* d_rep, size_t m, const int64_t* d_family,
                             size_t n_files, uint32_t* d_op_chunk, uint32_t* d_op_src_chunk, uint32_t* d_op_row,
                             uint32_t* d_op_src_row, uint64_t* d_op_dst_off, uint64_t* d_op_src_off,
                             uint64_t* d_op_len, uint32_t* d_chunk_op, uint32_t* d_row_ops, uint32_t* d_row_first_op,
                             uint64_t* d_counts, void* stream) {
  const char* who = "dev_family_recipes";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = family_recipes_args(c, who, d_chunk_file, d_chunk_off, d_chunk_len, d_rep, m, d_family, n_files))
    return rc;
  if (index_misaligned({}, {d_chunk_off, d_chunk_len, d_rep, d_family, d_op_dst_off, d_op_src_off, d_op_len, d_counts},
                       {d_chunk_file, d_op_chunk, d_op_src_chunk, d_op_row, d_op_src_row, d_chunk_op, d_row_ops,
                        d_row_first_op}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (u32 arrays 4 B, others 8 B)", who);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->fr_ws, (size_t)family_recipes_layout(m, n_files).bytes, call.st,
                           "family recipes workspace"))
    return rc;
  const FamilyRecipesIn in{{d_chunk_file, d_chunk_len, d_rep, d_family, (uint32_t)m, (uint32_t)n_files}, d_chunk_off};
  const FamilyRecipesOut out{d_op_chunk,   d_op_src_chunk, d_op_row,   d_op_src_row, d_op_dst_off,
                             d_op_src_off, d_op_len,       d_chunk_op, d_row_ops,    d_row_first_op};
  hipError_t e = family_recipes(c->fr_ws.p, in, out, (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

int sdcas_family_recipes(sdcas_ctx* c, const uint32_t* chunk_file, const uint64_t* chunk_off,
                         const uint64_t* chunk_len, const int64_t* rep, size_t m, const int64_t* family,
                         size_t n_files, uint32_t* out_op_chunk, uint32_t* out_op_src_chunk, uint32_t* out_op_row,
                         uint32_t* out_op_src_row, uint64_t* out_op_dst_off, uint64_t* out_op_src_off,
                         uint64_t* out_op_len, uint32_t* out_chunk_op, uint32_t* out_row_ops,
                         uint32_t* out_row_first_op, sdcas_family_recipes_counts* out_counts) {
  static_assert(sizeof(sdcas_family_recipes_counts) == kFamilyRecipesCounts * sizeof(uint64_t), "eight u64 counts");
  const char* who = "family_recipes";
  if (!c) return SDCAS_E_INVALID;
  if (int rc = family_recipes_args(c, who, chunk_file, chunk_off, chunk_len, rep, m, family, n_files)) return rc;
  if (index_misaligned({}, {chunk_off, chunk_len, rep, family, out_op_dst_off, out_op_src_off, out_op_len, out_counts},
                       {chunk_file, out_op_chunk, out_op_src_chunk, out_op_row, out_op_src_row, out_chunk_op,
                        out_row_ops, out_row_first_op}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (u32 arrays 4 B, others 8 B)", who);
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t nf = n_files;
  sdcas_family_recipes_counts cts;
  Parts p(c, st, who);
  const auto d_file = p.in(chunk_file, m);
  const auto d_off = p.in(chunk_off, m);
  const auto d_len = p.in(chunk_len, m);
  const auto d_rep = p.in(rep, m);
  const auto d_family = p.in(family, nf);
  const auto d_op_chunk = p.out(out_op_chunk, m);  // no more ops than chunks
  const auto d_op_src_chunk = p.out(out_op_src_chunk, m);
  const auto d_op_row = p.out(out_op_row, m);
  const auto d_op_src_row = p.out(out_op_src_row, m);
  const auto d_op_dst_off = p.out(out_op_dst_off, m);
  const auto d_op_src_off = p.out(out_op_src_off, m);
  const auto d_op_len = p.out(out_op_len, m);
  const auto d_chunk_op = p.out(out_chunk_op, m);
  const auto d_row_ops = p.out(out_row_ops, nf);
  const auto d_row_first = p.out(out_row_first_op, nf);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->fr_ws, (size_t)family_recipes_layout(m, n_files).bytes, st,
                           "family recipes workspace"))
    return rc;
  if (int rc = p.upload()) return rc;
  const FamilyRecipesIn in{{d_file, d_len, d_rep, d_family, (uint32_t)m, (uint32_t)n_files}, d_off};
  const FamilyRecipesOut out{d_op_chunk,   d_op_src_chunk, d_op_row,   d_op_src_row, d_op_dst_off,
                             d_op_src_off, d_op_len,       d_chunk_op, d_row_ops,    d_row_first};
  if (hipError_t e = family_recipes(c->fr_ws.p, in, out, d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.counts(d_cts)) return rc;
  if (cts.ops > m || cts.chunks > m || cts.files > nf) return c->fail(SDCAS_E_HIP, "%s: counts out of range", who);
  d_op_chunk.first(cts.ops), d_op_src_chunk.first(cts.ops), d_op_row.first(cts.ops), d_op_src_row.first(cts.ops);
  d_op_dst_off.first(cts.ops), d_op_src_off.first(cts.ops), d_op_len.first(cts.ops);
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

// ---- the family store (family_store.hip) -----------------------------------------------

uint64_t sdcas_family_store_tile_bytes(void) { return kFamilyStoreTile; }

static int family_store_range(uint64_t max_ops, uint64_t m, uint64_t n_files, const char** why) {
  if (max_ops > kFamilyStoreMaxOps) return *why = "more than 2^30 ops", SDCAS_E_CAPACITY;
  if (m > kFamilyStoreMaxOps) return *why = "more than 2^30 chunks", SDCAS_E_CAPACITY;
  if (n_files > kFamilyStoreMaxFiles) return *why = "more than 2^30 files", SDCAS_E_CAPACITY;
  return SDCAS_OK;
}

int sdcas_family_store_plan(uint64_t max_ops, uint64_t n_files, uint64_t* out_workspace_bytes) {
  const char* why = nullptr;
  if (int rc = family_store_range(max_ops, 0, n_files, &why)) return rc;
  if (out_workspace_bytes) *out_workspace_bytes = family_store_layout(max_ops).bytes;
  return SDCAS_OK;
}

// the layout call's arguments (host or device arrays)
static int family_store_layout_args(sdcas_ctx* c, const char* who, const FamilyStoreOps& o, const void* chunk_op,
                                    size_t m, size_t max_ops, const void* store_off, const void* counts) {
  const char* why = nullptr;
  if (int rc = family_store_range(max_ops, m, 0, &why)) return c->fail(rc, "%s: %s", who, why);
  if (max_ops && (!o.op_chunk || !o.op_src_chunk || !o.op_row || !o.op_src_row || !o.op_dst_off || !o.op_src_off ||
                  !o.op_len || !o.d_ops))
    return c->fail(SDCAS_E_INVALID, "%s: a null op array or null ops", who);
  if (m && !chunk_op) return c->fail(SDCAS_E_INVALID, "%s: null chunk_op", who);
  if (index_misaligned({}, {o.op_dst_off, o.op_src_off, o.op_len, o.d_ops, store_off, counts},
                       {o.op_chunk, o.op_src_chunk, o.op_row, o.op_src_row, chunk_op}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (u32 arrays 4 B, others 8 B)", who);
  return SDCAS_OK;
}

// a mover call's arguments (device arrays; the host forms check their own before they stage them)
static int family_store_move_args(sdcas_ctx* c, const char* who, bool restore, const FamilyStoreOps& o,
                                  const void* store_off, size_t max_ops, const FamilyStoreRows& r, size_t n_files,
                                  const void* blob, uint64_t blob_bytes, const void* store, uint64_t store_bytes,
                                  const void* counts, bool device) {
  const char* why = nullptr;
  if (int rc = family_store_range(max_ops, 0, n_files, &why)) return c->fail(rc, "%s: %s", who, why);
  if (max_ops && (!o.op_row || !o.op_dst_off || !o.op_len || !store_off || !o.d_ops ||
                  (!restore && (!o.op_chunk || !o.op_src_chunk))))
    return c->fail(SDCAS_E_INVALID, "%s: a null op array, null store offsets or null ops", who);
  if (n_files && (!r.row_at || !r.row_len)) return c->fail(SDCAS_E_INVALID, "%s: null row_at or row_len", who);
  if ((blob_bytes && !blob) || (store_bytes && !store)) return c->fail(SDCAS_E_INVALID, "%s: null blob or store", who);
  if (index_misaligned({device ? blob : nullptr, device ? store : nullptr},
                       {o.op_dst_off, o.op_len, o.d_ops, store_off, r.row_at, r.row_base, r.row_len, counts},
                       {o.op_chunk, o.op_src_chunk, o.op_row}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (blob and store 16 B, u32 arrays 4 B, others 8 B)",
                   who);
  return SDCAS_OK;
}

int sdcas_dev_family_store_layout(sdcas_ctx* c, const uint32_t* d_op_chunk, const uint32_t* d_op_src_chunk,
                                  const uint32_t* d_op_row, const uint32_t* d_op_src_row,
                                  const uint64_t* d_op_dst_off, const uint64_t* d_op_src_off,
                                  const uint64_t* d_op_len, const uint32_t* d_chunk_op, size_t m,
                                  const uint64_t* d_ops, size_t max_ops, uint64_t* d_op_store_off,
                                  uint64_t* d_counts, void* stream) {
  const char* who = "dev_family_store_layout";
  if (!c) return SDCAS_E_INVALID;
  const FamilyStoreOps ops{d_op_chunk,   d_op_src_chunk, d_op_row, d_op_src_row,     d_op_dst_off,
                           d_op_src_off, d_op_len,       d_ops,    (uint32_t)max_ops};
  if (int rc = family_store_layout_args(c, who, ops, d_chunk_op, m, max_ops, d_op_store_off, d_counts)) return rc;
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->fs_ws, (size_t)family_store_layout(max_ops).bytes, call.st, "family store workspace"))
    return rc;
  hipError_t e = family_store_offsets(c->fs_ws.p, ops, d_chunk_op, (uint32_t)m, d_op_store_off,
                                      (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

static int family_store_dev_move(sdcas_ctx* c, const char* who, bool restore, const FamilyStoreOps& ops,
                                 const uint64_t* d_op_store_off, size_t max_ops, const FamilyStoreRows& rows,
                                 size_t n_files, uint8_t* d_blob, uint64_t blob_bytes, uint8_t* d_store,
                                 uint64_t store_bytes, uint64_t* d_counts, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  if (int rc = family_store_move_args(c, who, restore, ops, d_op_store_off, max_ops, rows, n_files, d_blob, blob_bytes,
                                      d_store, store_bytes, d_counts, true))
    return rc;
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->fs_ws, (size_t)family_store_layout(max_ops).bytes, call.st, "family store workspace"))
    return rc;
  hipError_t e = family_store_move(c->fs_ws.p, ops, d_op_store_off, rows, d_blob, blob_bytes, d_store, store_bytes,
                                   restore, (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

int sdcas_dev_family_pack(sdcas_ctx* c, const uint32_t* d_op_chunk, const uint32_t* d_op_src_chunk,
                          const uint32_t* d_op_row, const uint64_t* d_op_dst_off, const uint64_t* d_op_len,
                          const uint64_t* d_op_store_off, const uint64_t* d_ops, size_t max_ops,
                          const uint64_t* d_row_at, const uint64_t* d_row_base, const uint64_t* d_row_len,
                          size_t n_files, const uint8_t* d_blob, uint64_t blob_bytes, uint8_t* d_store,
                          uint64_t store_capacity, uint64_t* d_counts, void* stream) {
  const FamilyStoreOps ops{d_op_chunk, d_op_src_chunk, d_op_row, nullptr,          d_op_dst_off,
                           nullptr,    d_op_len,       d_ops,    (uint32_t)max_ops};
  const FamilyStoreRows rows{d_row_at, d_row_base, d_row_len, (uint32_t)n_files};
  return family_store_dev_move(c, "dev_family_pack", false, ops, d_op_store_off, max_ops, rows, n_files,
                               const_cast<uint8_t*>(d_blob), blob_bytes, d_store, store_capacity, d_counts, stream);
}

int sdcas_dev_family_restore(sdcas_ctx* c, const uint32_t* d_op_row, const uint64_t* d_op_dst_off,
                             const uint64_t* d_op_len, const uint64_t* d_op_store_off, const uint64_t* d_ops,
                             size_t max_ops, const uint64_t* d_row_at, const uint64_t* d_row_base,
                             const uint64_t* d_row_len, size_t n_files, const uint8_t* d_store,
                             uint64_t store_bytes, uint8_t* d_blob, uint64_t blob_bytes, uint64_t* d_counts,
                             void* stream) {
  const FamilyStoreOps ops{nullptr, nullptr, d_op_row, nullptr, d_op_dst_off, nullptr, d_op_len, d_ops,
                           (uint32_t)max_ops};
  const FamilyStoreRows rows{d_row_at, d_row_base, d_row_len, (uint32_t)n_files};
  return family_store_dev_move(c, "dev_family_restore", true, ops, d_op_store_off, max_ops, rows, n_files, d_blob,
                               blob_bytes, const_cast<uint8_t*>(d_store), store_bytes, d_counts, stream);
}

int sdcas_family_store_layout(sdcas_ctx* c, const uint32_t* op_chunk, const uint32_t* op_src_chunk,
                              const uint32_t* op_row, const uint32_t* op_src_row, const uint64_t* op_dst_off,
                              const uint64_t* op_src_off, const uint64_t* op_len, size_t n_ops,
                              const uint32_t* chunk_op, size_t m, uint64_t* out_op_store_off,
                              sdcas_family_store_counts* out_counts) {
  static_assert(sizeof(sdcas_family_store_counts) == kFamilyStoreLayoutCounts * sizeof(uint64_t), "six u64 counts");
  const char* who = "family_store_layout";
  if (!c) return SDCAS_E_INVALID;
  const uint64_t h_ops = n_ops;
  const FamilyStoreOps h{op_chunk, op_src_chunk, op_row, op_src_row, op_dst_off, op_src_off, op_len, &h_ops, 0};
  if (int rc = family_store_layout_args(c, who, h, chunk_op, m, n_ops, out_op_store_off, out_counts)) return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  sdcas_family_store_counts cts;
  Parts p(c, st, who);
  const auto d_op_chunk = p.in(op_chunk, n_ops);
  const auto d_op_src_chunk = p.in(op_src_chunk, n_ops);
  const auto d_op_row = p.in(op_row, n_ops);
  const auto d_op_src_row = p.in(op_src_row, n_ops);
  const auto d_op_dst_off = p.in(op_dst_off, n_ops);
  const auto d_op_src_off = p.in(op_src_off, n_ops);
  const auto d_op_len = p.in(op_len, n_ops);
  const auto d_chunk_op = p.in(chunk_op, m);
  const auto d_ops = p.in(&h_ops, 1);
  const auto d_off = p.out(out_op_store_off, n_ops);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->fs_ws, (size_t)family_store_layout(n_ops).bytes, st, "family store workspace"))
    return rc;
  if (int rc = p.upload()) return rc;
  const FamilyStoreOps ops{d_op_chunk,   d_op_src_chunk, d_op_row, d_op_src_row,   d_op_dst_off,
                           d_op_src_off, d_op_len,       d_ops,    (uint32_t)n_ops};
  if (hipError_t e = family_store_offsets(c->fs_ws.p, ops, d_chunk_op, (uint32_t)m, d_off,
                                          d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

static int family_store_host_move(sdcas_ctx* c, const char* who, bool restore, const uint32_t* op_chunk,
                                  const uint32_t* op_src_chunk, const uint32_t* op_row, const uint64_t* op_dst_off,
                                  const uint64_t* op_len, const uint64_t* op_store_off, size_t n_ops,
                                  const uint64_t* row_at, const uint64_t* row_base, const uint64_t* row_len,
                                  size_t n_files, uint8_t* blob, uint64_t blob_bytes, uint8_t* store,
                                  uint64_t store_bytes, sdcas_family_move_counts* out_counts) {
  static_assert(sizeof(sdcas_family_move_counts) == kFamilyStoreMoveCounts * sizeof(uint64_t), "four u64 counts");
  if (!c) return SDCAS_E_INVALID;
  const uint64_t h_ops = n_ops;
  const FamilyStoreOps h{op_chunk, op_src_chunk, op_row, nullptr, op_dst_off, nullptr, op_len, &h_ops, 0};
  const FamilyStoreRows hr{row_at, row_base, row_len, 0};
  if (int rc = family_store_move_args(c, who, restore, h, op_store_off, n_ops, hr, n_files, blob, blob_bytes, store,
                                      store_bytes, out_counts, false))
    return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  sdcas_family_move_counts cts;
  Parts p(c, st, who);
  const auto d_op_chunk = p.in(op_chunk, n_ops);
  const auto d_op_src_chunk = p.in(op_src_chunk, n_ops);
  const auto d_op_row = p.in(op_row, n_ops);
  const auto d_op_dst_off = p.in(op_dst_off, n_ops);
  const auto d_op_len = p.in(op_len, n_ops);
  const auto d_off = p.in(op_store_off, n_ops);
  const auto d_ops = p.in(&h_ops, 1);
  const auto d_row_at = p.in(row_at, n_files);
  const auto d_row_base = p.in(row_base, n_files);
  const auto d_row_len = p.in(row_len, n_files);
  // the source goes up, the destination goes up and comes down: what the call does not write stays
  const auto d_blob_in = p.in(restore ? nullptr : (const uint8_t*)blob, (size_t)blob_bytes);
  const auto d_store_in = p.in(restore ? (const uint8_t*)store : nullptr, (size_t)store_bytes);
  const auto d_blob_io = p.inout(restore ? blob : nullptr, (size_t)blob_bytes);
  const auto d_store_io = p.inout(restore ? nullptr : store, (size_t)store_bytes);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->fs_ws, (size_t)family_store_layout(n_ops).bytes, st, "family store workspace"))
    return rc;
  if (int rc = p.upload()) return rc;
  const FamilyStoreOps ops{d_op_chunk, d_op_src_chunk, d_op_row, nullptr,        d_op_dst_off,
                           nullptr,    d_op_len,       d_ops,    (uint32_t)n_ops};
  const FamilyStoreRows rows{d_row_at, d_row_base, d_row_len, (uint32_t)n_files};
  uint8_t* d_blob = restore ? (uint8_t*)d_blob_io : const_cast<uint8_t*>((const uint8_t*)d_blob_in);
  uint8_t* d_store = restore ? const_cast<uint8_t*>((const uint8_t*)d_store_in) : (uint8_t*)d_store_io;
  if (hipError_t e = family_store_move(c->fs_ws.p, ops, d_off, rows, d_blob, blob_bytes, d_store, store_bytes, restore,
                                       d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

int sdcas_family_pack(sdcas_ctx* c, const uint32_t* op_chunk, const uint32_t* op_src_chunk, const uint32_t* op_row,
                      const uint64_t* op_dst_off, const uint64_t* op_len, const uint64_t* op_store_off, size_t ops,
                      const uint64_t* row_at, const uint64_t* row_base, const uint64_t* row_len, size_t n_files,
                      const uint8_t* blob, uint64_t blob_bytes, uint8_t* store, uint64_t store_capacity,
                      sdcas_family_move_counts* out_counts) {
  return family_store_host_move(c, "family_pack", false, op_chunk, op_src_chunk, op_row, op_dst_off, op_len,
                                op_store_off, ops, row_at, row_base, row_len, n_files, const_cast<uint8_t*>(blob),
                                blob_bytes, store, store_capacity, out_counts);
}

int sdcas_family_restore(sdcas_ctx* c, const uint32_t* op_row, const uint64_t* op_dst_off, const uint64_t* op_len,
                         const uint64_t* op_store_off, size_t ops, const uint64_t* row_at, const uint64_t* row_base,
                         const uint64_t* row_len, size_t n_files, const uint8_t* store, uint64_t store_bytes,
                         uint8_t* blob, uint64_t blob_bytes, sdcas_family_move_counts* out_counts) {
  return family_store_host_move(c, "family_restore", true, nullptr, nullptr, op_row, op_dst_off, op_len, op_store_off,
                                ops, row_at, row_base, row_len, n_files, blob, blob_bytes,
                                const_cast<uint8_t*>(store), store_bytes, out_counts);
}

// ---- a family store that forgets rows (family_forget.hip) -------------------------------

static int family_forget_range(uint64_t m, uint64_t n_files, uint64_t max_ops, uint64_t max_new_ops,
                               const char** why) {
  if (m > kFamilyForgetMax) return *why = "more than 2^30 chunks", SDCAS_E_CAPACITY;
  if (n_files > kFamilyForgetMax) return *why = "more than 2^30 files", SDCAS_E_CAPACITY;
  if (max_ops > kFamilyForgetMax || max_new_ops > kFamilyForgetMax) return *why = "more than 2^30 ops", SDCAS_E_CAPACITY;
  return SDCAS_OK;
}

int sdcas_family_forget_plan(uint64_t m, uint64_t n_files, uint64_t* out_workspace_bytes) {
  const char* why = nullptr;
  if (int rc = family_forget_range(m, n_files, 0, 0, &why)) return rc;
  if (out_workspace_bytes) *out_workspace_bytes = family_forget_bytes(m, n_files);
  return SDCAS_OK;
}

// keep's arguments (host or device arrays)
static int family_keep_args(sdcas_ctx* c, const char* who, const FamilyKeepIn& in, size_t m, size_t n_files,
                            const FamilyKeepOut& out, const void* counts) {
  const char* why = nullptr;
  if (int rc = family_forget_range(m, n_files, 0, 0, &why)) return c->fail(rc, "%s: %s", who, why);
  if (m && (!in.chunk_file || !in.chunk_off || !in.chunk_len || !in.rep))
    return c->fail(SDCAS_E_INVALID, "%s: null chunk_file, chunk_off, chunk_len or rep", who);
  if (n_files && (!in.family || !in.keep)) return c->fail(SDCAS_E_INVALID, "%s: null family or keep", who);
  if (index_misaligned({}, {in.chunk_off, in.chunk_len, in.rep, in.family, out.family, out.chunk_off, out.chunk_len,
                            out.rep, counts},
                       {in.chunk_file, out.row_new, out.row_from, out.chunk_from, out.chunk_file}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (u32 arrays 4 B, u64 and int64 8 B)", who);
  return SDCAS_OK;
}

int sdcas_dev_family_chunks_keep(sdcas_ctx* c, const uint32_t* d_chunk_file, const uint64_t* d_chunk_off,
                                 const uint64_t* d_chunk_len, const int64_t* d_rep, size_t m, const int64_t* d_family,
                                 const uint8_t* d_keep, size_t n_files, uint32_t* d_row_new, uint32_t* d_row_from,
                                 int64_t* d_family_out, uint32_t* d_chunk_from, uint32_t* d_chunk_file_out,
                                 uint64_t* d_chunk_off_out, uint64_t* d_chunk_len_out, int64_t* d_rep_out,
                                 uint64_t* d_counts, void* stream) {
  const char* who = "dev_family_chunks_keep";
  if (!c) return SDCAS_E_INVALID;
  const FamilyKeepIn in{d_chunk_file, d_chunk_off, d_chunk_len, d_rep, d_family, d_keep, (uint32_t)m, (uint32_t)n_files};
  const FamilyKeepOut out{d_row_new,        d_row_from,      d_family_out,    d_chunk_from,
                          d_chunk_file_out, d_chunk_off_out, d_chunk_len_out, d_rep_out};
  if (int rc = family_keep_args(c, who, in, m, n_files, out, d_counts)) return rc;
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->fg_ws, (size_t)family_keep_layout(m, n_files).bytes, call.st, "family forget workspace"))
    return rc;
  hipError_t e = family_chunks_keep(c->fg_ws.p, in, out, (unsigned long long*)d_counts, call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

int sdcas_family_chunks_keep(sdcas_ctx* c, const uint32_t* chunk_file, const uint64_t* chunk_off,
                             const uint64_t* chunk_len, const int64_t* rep, size_t m, const int64_t* family,
                             const uint8_t* keep, size_t n_files, uint32_t* out_row_new, uint32_t* out_row_from,
                             int64_t* out_family, uint32_t* out_chunk_from, uint32_t* out_chunk_file,
                             uint64_t* out_chunk_off, uint64_t* out_chunk_len, int64_t* out_rep,
                             sdcas_family_keep_counts* out_counts) {
  static_assert(sizeof(sdcas_family_keep_counts) == kFamilyKeepCounts * sizeof(uint64_t), "six u64 counts");
  const char* who = "family_chunks_keep";
  if (!c) return SDCAS_E_INVALID;
  const FamilyKeepIn h{chunk_file, chunk_off, chunk_len, rep, family, keep, 0, 0};
  const FamilyKeepOut ho{out_row_new,    out_row_from,  out_family,    out_chunk_from,
                         out_chunk_file, out_chunk_off, out_chunk_len, out_rep};
  if (int rc = family_keep_args(c, who, h, m, n_files, ho, out_counts)) return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  const size_t nf = n_files;
  sdcas_family_keep_counts cts;
  Parts p(c, st, who);
  const auto d_file = p.in(chunk_file, m);
  const auto d_off = p.in(chunk_off, m);
  const auto d_len = p.in(chunk_len, m);
  const auto d_rep = p.in(rep, m);
  const auto d_family = p.in(family, nf);
  const auto d_keep = p.in(keep, nf);
  const auto d_row_new = p.out(out_row_new, nf);
  const auto d_row_from = p.out(out_row_from, nf);
  const auto d_fam_out = p.out(out_family, nf);
  const auto d_chunk_from = p.out(out_chunk_from, m);
  const auto d_file_out = p.out(out_chunk_file, m);
  const auto d_off_out = p.out(out_chunk_off, m);
  const auto d_len_out = p.out(out_chunk_len, m);
  const auto d_rep_out = p.out(out_rep, m);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->fg_ws, (size_t)family_keep_layout(m, n_files).bytes, st, "family forget workspace"))
    return rc;
  if (int rc = p.upload()) return rc;
  const FamilyKeepIn in{d_file, d_off, d_len, d_rep, d_family, d_keep, (uint32_t)m, (uint32_t)n_files};
  const FamilyKeepOut out{d_row_new, d_row_from, d_fam_out, d_chunk_from, d_file_out, d_off_out, d_len_out, d_rep_out};
  if (hipError_t e = family_chunks_keep(c->fg_ws.p, in, out, d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.counts(d_cts)) return rc;
  if (cts.rows_kept > nf || cts.chunks_kept > m) return c->fail(SDCAS_E_HIP, "%s: counts out of range", who);
  d_row_from.first(cts.rows_kept), d_fam_out.first(cts.rows_kept);
  d_chunk_from.first(cts.chunks_kept), d_file_out.first(cts.chunks_kept), d_off_out.first(cts.chunks_kept);
  d_len_out.first(cts.chunks_kept), d_rep_out.first(cts.chunks_kept);
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

// moves' arguments (host or device arrays)
static int family_moves_args(sdcas_ctx* c, const char* who, const FamilyMovesIn& in, size_t m, size_t max_ops,
                             size_t max_chunks, size_t max_new_ops, const void* move_dst, const void* move_src,
                             const void* move_len, const void* counts) {
  const char* why = nullptr;
  if (int rc = family_forget_range(m > max_chunks ? m : max_chunks, 0, max_ops, max_new_ops, &why))
    return c->fail(rc, "%s: %s", who, why);
  if (m && (!in.chunk_off || !in.chunk_op)) return c->fail(SDCAS_E_INVALID, "%s: null chunk_off or chunk_op", who);
  if (max_ops && (!in.op_dst_off || !in.op_store_off || !in.d_ops))
    return c->fail(SDCAS_E_INVALID, "%s: null op_dst_off, op_store_off or ops", who);
  if (max_chunks && (!in.nchunk_from || !in.nchunk_off || !in.nchunk_len || !in.nchunk_op || !in.d_chunks))
    return c->fail(SDCAS_E_INVALID, "%s: a null new chunk array or null new chunks", who);
  if (max_new_ops && (!in.nop_chunk || !in.nop_src_chunk || !in.nop_dst_off || !in.nop_store_off || !in.d_nops))
    return c->fail(SDCAS_E_INVALID, "%s: a null new op array or null new ops", who);
  if (index_misaligned({}, {in.chunk_off, in.op_dst_off, in.op_store_off, in.d_ops, in.nchunk_off, in.nchunk_len,
                            in.d_chunks, in.nop_dst_off, in.nop_store_off, in.d_nops, move_dst, move_src, move_len,
                            counts},
                       {in.chunk_op, in.nchunk_from, in.nchunk_op, in.nop_chunk, in.nop_src_chunk}))
    return c->fail(SDCAS_E_INVALID, "%s: an array is misaligned (u32 arrays 4 B, u64 8 B)", who);
  return SDCAS_OK;
}

int sdcas_dev_family_store_moves(sdcas_ctx* c, const uint64_t* d_chunk_off, const uint32_t* d_chunk_op, size_t m,
                                 const uint64_t* d_op_dst_off, const uint64_t* d_op_store_off, const uint64_t* d_ops,
                                 size_t max_ops, const uint32_t* d_new_chunk_from, const uint64_t* d_new_chunk_off,
                                 const uint64_t* d_new_chunk_len, const uint32_t* d_new_chunk_op,
                                 const uint64_t* d_new_chunks, size_t max_chunks, const uint32_t* d_new_op_chunk,
                                 const uint32_t* d_new_op_src_chunk, const uint64_t* d_new_op_dst_off,
                                 const uint64_t* d_new_op_store_off, const uint64_t* d_new_ops, size_t max_new_ops,
                                 uint64_t* d_move_dst, uint64_t* d_move_src, uint64_t* d_move_len, uint64_t* d_counts,
                                 void* stream) {
  const char* who = "dev_family_store_moves";
  if (!c) return SDCAS_E_INVALID;
  const FamilyMovesIn in{d_chunk_off,        d_chunk_op,       (uint32_t)m,          d_op_dst_off,     d_op_store_off,
                         d_ops,              (uint32_t)max_ops, d_new_chunk_from,    d_new_chunk_off,  d_new_chunk_len,
                         d_new_chunk_op,     d_new_chunks,     (uint32_t)max_chunks, d_new_op_chunk,   d_new_op_src_chunk,
                         d_new_op_dst_off,   d_new_op_store_off, d_new_ops,          (uint32_t)max_new_ops};
  if (int rc = family_moves_args(c, who, in, m, max_ops, max_chunks, max_new_ops, d_move_dst, d_move_src, d_move_len,
                                 d_counts))
    return rc;
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (int rc = grow_synced(c, c->fg_ws, (size_t)family_moves_layout(max_chunks).bytes, call.st,
                           "family forget workspace"))
    return rc;
  hipError_t e = family_store_moves(c->fg_ws.p, in, d_move_dst, d_move_src, d_move_len, (unsigned long long*)d_counts,
                                    call.st);
  return e ? hip_fail_at(c, e, who, "") : SDCAS_OK;
}

int sdcas_family_store_moves(sdcas_ctx* c, const uint64_t* chunk_off, const uint32_t* chunk_op, size_t m,
                             const uint64_t* op_dst_off, const uint64_t* op_store_off, size_t n_ops,
                             const uint32_t* new_chunk_from, const uint64_t* new_chunk_off,
                             const uint64_t* new_chunk_len, const uint32_t* new_chunk_op, size_t new_chunks,
                             const uint32_t* new_op_chunk, const uint32_t* new_op_src_chunk,
                             const uint64_t* new_op_dst_off, const uint64_t* new_op_store_off, size_t new_ops,
                             uint64_t* out_move_dst, uint64_t* out_move_src, uint64_t* out_move_len,
                             sdcas_family_moves_counts* out_counts) {
  static_assert(sizeof(sdcas_family_moves_counts) == kFamilyMovesCounts * sizeof(uint64_t), "six u64 counts");
  const char* who = "family_store_moves";
  if (!c) return SDCAS_E_INVALID;
  const uint64_t h_n[3] = {n_ops, new_chunks, new_ops};
  const FamilyMovesIn h{chunk_off,      chunk_op,     0, op_dst_off,   op_store_off,     &h_n[0],        0,
                        new_chunk_from, new_chunk_off, new_chunk_len, new_chunk_op,    &h_n[1],        0,
                        new_op_chunk,   new_op_src_chunk, new_op_dst_off, new_op_store_off, &h_n[2],   0};
  if (int rc = family_moves_args(c, who, h, m, n_ops, new_chunks, new_ops, out_move_dst, out_move_src, out_move_len,
                                 out_counts))
    return rc;
  if (out_counts) memset(out_counts, 0, sizeof *out_counts);
  DevCall call(c, nullptr);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  sdcas_family_moves_counts cts;
  Parts p(c, st, who);
  const auto d_chunk_off = p.in(chunk_off, m);
  const auto d_chunk_op = p.in(chunk_op, m);
  const auto d_op_dst = p.in(op_dst_off, n_ops);
  const auto d_op_off = p.in(op_store_off, n_ops);
  const auto d_from = p.in(new_chunk_from, new_chunks);
  const auto d_noff = p.in(new_chunk_off, new_chunks);
  const auto d_nlen = p.in(new_chunk_len, new_chunks);
  const auto d_nop = p.in(new_chunk_op, new_chunks);
  const auto d_nop_chunk = p.in(new_op_chunk, new_ops);
  const auto d_nop_src = p.in(new_op_src_chunk, new_ops);
  const auto d_nop_dst = p.in(new_op_dst_off, new_ops);
  const auto d_nop_off = p.in(new_op_store_off, new_ops);
  const auto d_n = p.in(h_n, 3);
  const auto d_dst = p.out(out_move_dst, new_chunks);
  const auto d_src = p.out(out_move_src, new_chunks);
  const auto d_len = p.out(out_move_len, new_chunks);
  const auto d_cts = p.out(&cts, 1);
  if (int rc = p.reserve()) return rc;
  if (int rc = grow_synced(c, c->fg_ws, (size_t)family_moves_layout(new_chunks).bytes, st, "family forget workspace"))
    return rc;
  if (int rc = p.upload()) return rc;
  const uint64_t* dn = d_n;
  const FamilyMovesIn in{d_chunk_off, d_chunk_op, (uint32_t)m, d_op_dst, d_op_off, dn, (uint32_t)n_ops,
                         d_from,      d_noff,     d_nlen,      d_nop,    dn + 1,   (uint32_t)new_chunks,
                         d_nop_chunk, d_nop_src,  d_nop_dst,   d_nop_off, dn + 2,  (uint32_t)new_ops};
  if (hipError_t e = family_store_moves(c->fg_ws.p, in, d_dst, d_src, d_len, d_cts.as<unsigned long long>(), st))
    return hip_fail_at(c, e, who, "");
  if (int rc = p.counts(d_cts)) return rc;
  if (cts.moves > new_chunks) return c->fail(SDCAS_E_HIP, "%s: counts out of range", who);
  d_dst.first(cts.moves), d_src.first(cts.moves), d_len.first(cts.moves);
  if (int rc = p.download()) return rc;
  if (out_counts) *out_counts = cts;
  return SDCAS_OK;
}

int sdcas_dev_set_sort(sdcas_ctx* c, int enable) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  c->ws.sort = enable ? 1 : 0;
  return SDCAS_OK;
}

int sdcas_dev_set_leaf_variant(sdcas_ctx* c, int variant) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  if (variant != -1 && !leaf_variant_available(variant))
    return c->fail(SDCAS_E_INVALID, "leaf variant %d is not in this build", variant);
  c->ws.variant = variant;
  return SDCAS_OK;
}

int sdcas_dev_set_piece_variant(sdcas_ctx* c, int variant) {
  if (!c) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  if (variant != -1 && !piece_variant_available(variant))
    return c->fail(SDCAS_E_INVALID, "piece variant %d is not in this build", variant);
  c->piece_variant = variant;
  return SDCAS_OK;
}

// ---- synthetic corpora -------------------------------------------------------

int sdcas_dev_synth_cas_messages(sdcas_ctx* c, const uint64_t* d_keys, const uint64_t* d_sizes,
                                 const uint64_t* d_offs, size_t n, uint8_t* d_blob, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  hipError_t e = synth_cas_messages(d_keys, d_sizes, d_offs, (uint32_t)n, d_blob, st);
  return e ? c->hip_fail(e, "synth") : SDCAS_OK;
}

int sdcas_dev_synth_content(sdcas_ctx* c, const uint64_t* d_keys, const uint64_t* d_starts, const uint64_t* d_lens,
                            const uint64_t* d_offs, size_t n, uint8_t* d_blob, void* stream) {
  if (!c) return SDCAS_E_INVALID;
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  hipError_t e = synth_content(d_keys, d_starts, d_lens, d_offs, (uint32_t)n, d_blob, st);
  return e ? c->hip_fail(e, "synth") : SDCAS_OK;
}

// ---- multi-GPU dedup stages -----------------------------------

int sdcas_dev_dedup_combine(sdcas_ctx* c, const uint64_t* d_keys, const uint8_t* d_has_key, const int32_t* d_status,
                            const uint64_t* d_ids, size_t n, uint32_t world, uint64_t* d_rec, uint32_t* d_slot,
                            uint64_t* out_starts, void* stream) {
  if (!c || world == 0 || !out_starts || (n && (!d_keys || !d_ids || !d_rec))) return SDCAS_E_INVALID;
  // record indices and slot codes are 32-bit
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "dedup_combine: %zu records exceed 2^31 - 1", n);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  uint64_t u = 0;
  hipError_t e = dd_combine(c->dist, d_keys, d_has_key, d_status, d_ids, (uint32_t)n, world, d_rec, d_slot,
                            out_starts, &u, call.st);
  return e ? c->hip_fail(e, "dedup_combine") : SDCAS_OK;
}

int sdcas_dev_dedup_combine_async(sdcas_ctx* c, const uint64_t* d_keys, const uint8_t* d_has_key,
                                  const int32_t* d_status, const uint64_t* d_ids, size_t n, uint32_t world,
                                  uint64_t* d_rec, uint32_t* d_slot, uint32_t* d_starts, void* stream) {
  if (!c || world == 0 || !d_starts || (n && (!d_keys || !d_ids || !d_rec))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "dedup_combine: %zu records exceed 2^31 - 1", n);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e = dd_combine_dev(c->dist, d_keys, d_has_key, d_status, d_ids, (uint32_t)n, world, d_rec, d_slot,
                                d_starts, call.st);
  return e ? c->hip_fail(e, "dedup_combine_async") : SDCAS_OK;
}

int sdcas_dev_dedup_combine_buckets(sdcas_ctx* c, const uint64_t* d_keys, const uint8_t* d_has_key,
                                    const int32_t* d_status, const uint64_t* d_ids, size_t n, uint32_t world,
                                    size_t cap, uint64_t* d_send, uint32_t* d_slot, int64_t* d_counts,
                                    uint32_t* d_overflow, void* stream) {
  if (!c || world == 0 || !d_counts || !d_overflow || (n && (!d_keys || !d_ids || !d_send))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH || (uint64_t)world * cap > SDCAS_MAX_BATCH)
    return c->fail(SDCAS_E_CAPACITY, "dedup_combine_buckets: %zu records / %u x %zu buckets exceed 2^31 - 1", n,
                   world, cap);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e = dd_combine_buckets(c->dist, d_keys, d_has_key, d_status, d_ids, (uint32_t)n, world, (uint32_t)cap,
                                    d_send, d_slot, d_counts, d_overflow, call.st);
  return e ? c->hip_fail(e, "dedup_combine_buckets") : SDCAS_OK;
}

int sdcas_dev_dedup_resolve(sdcas_ctx* c, const uint64_t* d_frec, size_t nf, const uint64_t* d_erec, size_t ne,
                            int64_t* d_result, void* stream) {
  if (!c || (nf && (!d_frec || !d_result)) || (ne && !d_erec)) return SDCAS_E_INVALID;
  if (!dedup_fits(nf, ne)) return c->fail(SDCAS_E_CAPACITY, "dedup_resolve: %zu + %zu records exceed 2^30", nf, ne);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e = dd_resolve(c->dist, d_frec, (uint32_t)nf, d_erec, (uint32_t)ne, d_result, call.st);
  return e ? c->hip_fail(e, "dedup_resolve") : SDCAS_OK;
}

int sdcas_dev_dedup_resolve_buckets(sdcas_ctx* c, const uint64_t* d_frec, size_t fcap, const int64_t* d_fcounts,
                                    const uint64_t* d_erec, size_t ecap, const int64_t* d_ecounts, uint32_t world,
                                    int64_t* d_result, void* stream) {
  if (!c || world == 0 || (fcap && (!d_frec || !d_fcounts || !d_result)) || (ecap && (!d_erec || !d_ecounts)))
    return SDCAS_E_INVALID;
  if (!dedup_fits((uint64_t)world * fcap, (uint64_t)world * ecap))
    return c->fail(SDCAS_E_CAPACITY, "dedup_resolve_buckets: %u x (%zu + %zu) records exceed 2^30", world, fcap, ecap);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e = dd_resolve_buckets(c->dist, d_frec, (uint32_t)fcap, d_fcounts, d_erec, (uint32_t)ecap, d_ecounts,
                                    world, d_result, call.st);
  return e ? c->hip_fail(e, "dedup_resolve_buckets") : SDCAS_OK;
}

int sdcas_dev_dedup_local(sdcas_ctx* c, const uint64_t* d_keys, const uint8_t* d_has_key, const int32_t* d_status,
                          const uint64_t* d_ids, size_t n, const uint64_t* d_ekeys, const uint64_t* d_eids, size_t ne,
                          size_t chunk_size, uint64_t n_total, uint64_t max_steps, uint32_t more, int64_t* d_link,
                          uint64_t* d_counts, uint64_t* d_plan_header, void* stream) {
  if (!c || (n && (!d_keys || !d_ids || !d_link)) || (ne && (!d_ekeys || !d_eids))) return SDCAS_E_INVALID;
  if (!dedup_fits(n, ne)) return c->fail(SDCAS_E_CAPACITY, "dedup_local: %zu + %zu records exceed 2^30", n, ne);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  StepWindow sw;
  sw.n_total = n_total;
  sw.max_steps = max_steps;
  sw.more = more;
  hipError_t e = dd_local(c->dist, d_keys, d_has_key, d_status, d_ids, (uint32_t)n, d_ekeys, d_eids, (uint32_t)ne,
                          chunk_size ? chunk_size : SDCAS_IDENTIFIER_CHUNK_SIZE, sw, d_link,
                          (unsigned long long*)d_counts, call.st);
  if (!e && d_plan_header)
    e = hipMemcpyAsync(d_plan_header, c->dist.plan.p, 8 * kPlanHeader, hipMemcpyDeviceToDevice, call.st);
  return e ? c->hip_fail(e, "dedup_local") : SDCAS_OK;
}

int sdcas_dev_dedup_stays(sdcas_ctx* c, const uint8_t* d_has_key, const int32_t* d_status, const uint64_t* d_ids,
                          size_t n, size_t cap, uint64_t* d_stays, int64_t* d_count, void* stream) {
  if (!c || (n && (d_has_key || d_status) && !d_ids) || (cap && !d_stays)) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH || cap > SDCAS_MAX_BATCH)
    return c->fail(SDCAS_E_CAPACITY, "dedup_stays: %zu files / %zu entries exceed 2^31 - 1", n, cap);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e = dd_stays(c->dist, d_has_key, d_status, d_ids, (uint32_t)n, (uint32_t)cap, d_stays, d_count, call.st);
  return e ? c->hip_fail(e, "dedup_stays") : SDCAS_OK;
}

int sdcas_dev_dedup_plan(sdcas_ctx* c, const uint64_t* d_stays, size_t n_stays, uint64_t n_total, size_t chunk_size,
                         uint64_t max_steps, uint32_t more, uint64_t* d_plan, void* stream) {
  if (!c || !d_plan || (n_stays && !d_stays)) return SDCAS_E_INVALID;
  if (n_stays > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "dedup_plan: %zu entries exceed 2^31 - 1", n_stays);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  StepWindow sw;
  sw.n_total = n_total;
  sw.max_steps = max_steps;
  sw.more = more;
  hipError_t e = dd_plan(c->dist, d_stays, (uint32_t)n_stays, chunk_size ? chunk_size : SDCAS_IDENTIFIER_CHUNK_SIZE,
                         sw, d_plan, call.st);
  return e ? c->hip_fail(e, "dedup_plan") : SDCAS_OK;
}

int sdcas_dev_dedup_apply(sdcas_ctx* c, const uint64_t* d_ids, const uint32_t* d_slot, size_t n,
                          const int64_t* d_result, size_t chunk_size, const uint64_t* d_plan, int64_t* d_link,
                          uint64_t* d_counts, void* stream) {
  if (!c || (n && (!d_ids || !d_slot || !d_link))) return SDCAS_E_INVALID;
  if (n > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "dedup_apply: %zu files exceed 2^31 - 1", n);
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  hipError_t e = dd_apply(c->dist, d_ids, d_slot, (uint32_t)n, d_result, chunk_size ? chunk_size : SDCAS_IDENTIFIER_CHUNK_SIZE,
                          d_plan, d_link, (unsigned long long*)d_counts, call.st);
  return e ? c->hip_fail(e, "dedup_apply") : SDCAS_OK;
}

// ---- device-resident big-message stream (C4, file_checksum of huge files) --------

// A device buffer about to grow is freed and reallocated: the context's
// enqueued work (any stream) must be done with it first. Growth happens on a
// session larger than every earlier one, so the steady state never waits.
}  // extern "C"
template <typename T>
static hipError_t grow(sdcas_ctx* c, DevBuf<T>& b, size_t n, hipStream_t st = nullptr) {
  if (n <= b.cap) return hipSuccess;
  hipError_t e;
  if (st && (e = hipStreamSynchronize(st))) return e;
  if ((e = c->scratch_sync())) return e;
  return b.ensure(n);
}
extern "C" {

// The session's message descriptors go up and its node list is cleared on
// the stream of the session's first device call (stream_begin names none):
// no host wait, ordered after the previous session's kernels by the fence.
static hipError_t stream_flush_begin(sdcas_ctx* c, hipStream_t st) {
  if (!c->sm_begin_pending) return hipSuccess;
  c->sm_begin_pending = false;
  hipError_t e;
  if (!c->sm_files.empty() &&
      (e = c->sm_stage.put(c->sm_files.data(), sizeof(FileDesc) * c->sm_files.size(), c->sm_d_files.p, st)))
    return e;
  // node entries no segment of this session writes stay zero, so that the
  // node lists of ranks that hashed disjoint pieces of the same messages add
  // up to the complete list (sdcas_dev_stream_import)
  if (c->sm_node_bytes && (e = hipMemsetAsync(c->sm_nodes.p, 0, c->sm_node_bytes, st))) return e;
  return hipSuccess;
}

int sdcas_dev_stream_begin(sdcas_ctx* c, const uint64_t* lens, size_t nfiles) {
  if (!c || (nfiles && !lens)) return SDCAS_E_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipSetDevice(c->device);
  std::vector<FileDesc> files(nfiles, FileDesc{});
  uint64_t nodes = 0;
  for (size_t i = 0; i < nfiles; ++i) {
    const uint64_t C = chunks_of(lens[i]);
    if (C <= kTile) return c->fail(SDCAS_E_INVALID, "stream message %zu: %llu bytes (must exceed 1 MiB)", i,
                                   (unsigned long long)lens[i]);
    files[i].C = C;
    files[i].node_base = nodes;
    files[i].out_index = i;
    nodes += bigfile_node_count(C);
  }
  // the descriptors and node list are rewritten in stream order by the
  // session's first device call (stream_flush_begin); only a buffer that must
  // grow waits for the previous session here
  hipError_t e;
  if ((e = grow(c, c->sm_nodes, 8 * nodes + 8)) || (e = grow(c, c->sm_d_files, nfiles + 1)) ||
      (e = grow(c, c->piece_ctr, 1)))
    return c->hip_fail(e, "stream workspace");
  c->sm_files.swap(files);
  c->sm_node_bytes = 32 * nodes;
  c->sm_active = true;
  c->sm_begin_pending = true;
  return SDCAS_OK;
}

size_t sdcas_dev_stream_node_bytes(sdcas_ctx* c) { return c && c->sm_active ? (size_t)c->sm_node_bytes : 0; }

int sdcas_dev_stream_export(sdcas_ctx* c, uint8_t* d_dst, size_t bytes, void* stream) {
  if (!c || (bytes && !d_dst)) return SDCAS_E_INVALID;
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (!c->sm_active || bytes != c->sm_node_bytes)
    return c->fail(SDCAS_E_INVALID, "stream_export: %zu bytes, the session's node list holds %llu", bytes,
                   (unsigned long long)c->sm_node_bytes);
  hipError_t e = stream_flush_begin(c, call.st);
  if (!e && bytes) e = hipMemcpyAsync(d_dst, c->sm_nodes.p, bytes, hipMemcpyDeviceToDevice, call.st);
  return e ? c->hip_fail(e, "stream_export") : SDCAS_OK;
}

int sdcas_dev_stream_import(sdcas_ctx* c, const uint8_t* d_src, size_t bytes, void* stream) {
  if (!c || (bytes && !d_src)) return SDCAS_E_INVALID;
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (!c->sm_active || bytes != c->sm_node_bytes)
    return c->fail(SDCAS_E_INVALID, "stream_import: %zu bytes, the session's node list holds %llu", bytes,
                   (unsigned long long)c->sm_node_bytes);
  hipError_t e = stream_flush_begin(c, call.st);
  if (!e && bytes) e = hipMemcpyAsync(c->sm_nodes.p, d_src, bytes, hipMemcpyDeviceToDevice, call.st);
  return e ? c->hip_fail(e, "stream_import") : SDCAS_OK;
}

int sdcas_dev_stream_update(sdcas_ctx* c, size_t nseg, const uint64_t* h_file, const uint64_t* h_msg_off,
                            const uint64_t* h_len, const uint64_t* h_dev_addr, void* stream) {
  if (!c || (nseg && (!h_file || !h_msg_off || !h_len || !h_dev_addr))) return SDCAS_E_INVALID;
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (!c->sm_active) return c->fail(SDCAS_E_INVALID, "stream_update without stream_begin");
  const uint64_t piece_bytes = 1024ull * kTile;
  uint64_t base = ~0ull;
  for (size_t k = 0; k < nseg; ++k) base = std::min(base, h_dev_addr[k]);
  // one descriptor per segment (the caller's few hundred); the device expands
  // them into the per-piece list (expand_pieces)
  std::vector<SegDesc> segs(nseg);
  uint64_t npieces = 0;
  for (size_t k = 0; k < nseg; ++k) {
    if (h_file[k] >= c->sm_files.size()) return c->fail(SDCAS_E_INVALID, "segment %zu: no such message", k);
    const FileDesc& fd = c->sm_files[h_file[k]];
    const uint64_t mlen = fd.C * 1024;  // upper bound; the last chunk may be short
    const uint64_t off = h_msg_off[k], len = h_len[k];
    if ((off % piece_bytes) || (h_dev_addr[k] & 15) || !len || off + len > mlen ||
        ((len % piece_bytes) && chunks_of(off + len) != fd.C))
      return c->fail(SDCAS_E_INVALID, "segment %zu: offset/length not on 1 MiB pieces", k);
    segs[k] = SegDesc{h_dev_addr[k] - base, off / 1024, fd.node_base, len, npieces};
    npieces += (len + piece_bytes - 1) / piece_bytes;
  }
  hipStream_t st = call.st;
  hipError_t e = stream_flush_begin(c, st);
  if (e) return c->hip_fail(e, "stream descs");
  if (!npieces) return SDCAS_OK;
  if (npieces > SDCAS_MAX_BATCH) return c->fail(SDCAS_E_CAPACITY, "stream_update: %llu pieces",
                                                (unsigned long long)npieces);
  // stream-ordered: a previous update's kernels on any stream are behind the
  // fence, so the descriptor buffers are free once this call's work starts
  if ((e = grow(c, c->sm_pieces, npieces, st)) || (e = grow(c, c->sm_segs, nseg, st)) ||
      (e = grow(c, c->piece_l4, kPieceL4Words * npieces, st)))
    return c->hip_fail(e, "piece descs");
  if ((e = c->sm_stage.put(segs.data(), sizeof(SegDesc) * nseg, c->sm_segs.p, st)) ||
      (e = expand_pieces(c->sm_segs.p, (uint32_t)nseg, c->sm_pieces.p, (uint32_t)npieces, st)))
    return c->hip_fail(e, "piece descs");
  hipEvent_t a = nullptr, b = nullptr;
  if (c->profile) {
    a = c->event();
    b = c->event();
    (void)hipEventRecord(a, st);
  }
  e = piece_hash(reinterpret_cast<const uint8_t*>(base), c->sm_pieces.p, (uint32_t)npieces, c->sm_nodes.p,
                 c->piece_ctr.p, c->piece_l4.p, c->piece_variant, st);
  if (c->profile) {
    (void)hipEventRecord(b, st);
    c->ev_leaf.push_back({a, b});
    c->ev_all.push_back({c->event(), c->event()});
    (void)hipEventRecord(c->ev_all.back().first, st);
    (void)hipEventRecord(c->ev_all.back().second, st);
  }
  return e ? c->hip_fail(e, "piece_hash") : SDCAS_OK;
}

int sdcas_dev_stream_finish(sdcas_ctx* c, uint8_t* d_out32, void* stream) {
  if (!c || !d_out32) return SDCAS_E_INVALID;
  if ((uintptr_t)d_out32 & 15) return c->fail(SDCAS_E_INVALID, "stream_finish: digests not 16-byte aligned");
  DevCall call(c, stream);
  if (call.rc) return call.rc;
  if (!c->sm_active) return c->fail(SDCAS_E_INVALID, "stream_finish without stream_begin");
  hipStream_t st = call.st;
  hipError_t e = stream_flush_begin(c, st);
  if (e) return c->hip_fail(e, "stream descs");
  c->sm_active = false;
  e = bigfile_finish(c->sm_d_files.p, (uint32_t)c->sm_files.size(), c->sm_nodes.p, d_out32, st);
  return e ? c->hip_fail(e, "bigfile_finish") : SDCAS_OK;
}

}  // extern "C"
