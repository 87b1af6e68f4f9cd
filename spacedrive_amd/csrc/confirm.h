// confirm.h — the (cas key, checksum) group-by (confirm.hip): which files of a
// batch are really duplicates, and which cas_ids collide (files that share a
// cas key while their full-content digests differ).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

constexpr uint64_t kConfirmMaxFiles = 1ull << 30;  // file indices and table capacity are 32-bit
constexpr uint32_t kConfirmCounts = 6;             // sdcas_confirm_counts' words

// table capacity for n files: a power of two >= 2n (at least 64)
inline uint64_t confirm_table_cap(uint64_t n) {
  uint64_t cap = 64;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}
// u32 words of workspace for n files: the class table and the key table
// (confirm_table_cap(n) each), every file's slot in either, and the per-key
// class counters
inline uint64_t confirm_ws_words(uint64_t n) { return 2 * confirm_table_cap(n) + 3 * n; }

// keys[n], digests[32 * n] (16-byte aligned), valid[n] (null: all valid):
// device inputs. rep / key_rep (i64[n]), flags (u8[n]) and counts
// (u64[kConfirmCounts], overwritten) may each be null. ws: confirm_ws_words(n)
// words. Enqueues on st; n in [1, kConfirmMaxFiles].
hipError_t confirm_duplicates(uint32_t* ws, const uint64_t* keys, const uint8_t* digests, const uint8_t* valid,
                              uint32_t n, int64_t* rep, int64_t* key_rep, uint8_t* flags,
                              unsigned long long* counts, hipStream_t st);

}  // namespace sdcas
