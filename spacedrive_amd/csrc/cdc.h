// cdc.h — content-defined chunking of resident file contents and the sharing
// pass over the chunks (cdc.hip; definitions in include/sdcas.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

constexpr uint64_t kCdcMaxChunks = 1ull << 30;  // chunk indices are 32-bit
constexpr uint32_t kCdcCounts = 6;              // sdcas_chunk_counts' / sdcas_sharing_counts' words
constexpr uint32_t kCdcSlot = 1024;             // positions per bitmap slot (sdcas_chunk_plan's out_max_slots)
// the gear kernel: each lane runs a strip of kCdcStrip consecutive bytes, a
// workgroup of kCdcTB lanes a tile of kCdcTile bytes of ONE file
constexpr uint32_t kCdcStrip = 128;
constexpr uint32_t kCdcTB = 256;
constexpr uint32_t kCdcTile = kCdcStrip * kCdcTB;
constexpr uint64_t kCdcGearSeed = 0x3130304344434453ull;  // "SDCDC001" little-endian

struct CdcParams {
  uint32_t min_len, avg_bits, max_len;
};
inline bool cdc_params_valid(const CdcParams& p) {
  if (p.avg_bits < 6 || p.avg_bits > 24) return false;
  const uint64_t avg = 1ull << p.avg_bits;
  return p.min_len >= 32 && p.min_len < avg && avg < p.max_len && p.max_len <= (1u << 28);
}

// ---- the plan, from host lengths (GPU-free) --------------------------------------
enum CdcPlanError { kCdcOk = 0, kCdcInvalid = 1, kCdcCapacity = 2 };
// max_chunks = sum of ceil(len / min_len); max_slots = sum of ceil(len / 1024) + max_chunks
CdcPlanError cdc_plan(const uint64_t* lens, size_t n, const CdcParams& p, uint64_t* max_chunks, uint64_t* max_slots);

// ---- the device workspace of one chunk call --------------------------------------
// byte offsets from its start, each 16-byte aligned
struct CdcLayout {
  uint64_t sb, tb, mcb, fcnt;  // u32[n + 1] each: slot, tile, chunk-bound and chunk bases (exclusive scans)
  uint64_t counts;             // u64[8]: the six counts, [6] spare (a windows call: the windows not final), [7] a bound was hit (never, with a true plan)
  uint64_t ends;               // u64[max_chunks]: the cut pass's ends, file i's at mcb[i]
  uint64_t woff, wlen, po;     // u64[max_chunks] each: the chunks' blob offsets, lengths, packed offsets
  uint64_t bitmap;             // 256 B per slot: per 128 positions LOOSE (16 B) then STRICT (16 B)
  uint64_t bytes;
};
CdcLayout cdc_layout(uint64_t n, uint64_t max_chunks, uint64_t file_slots);

struct CdcArgs {
  uint8_t* ws;
  const uint8_t* blob;
  const uint64_t* offs;
  const uint64_t* lens;
  uint32_t n;
  CdcParams p;
  uint64_t max_chunks, file_slots;  // file_slots = max_slots - max_chunks
  uint64_t* file_chunks;            // outputs, any may be null
  uint64_t* chunk_off;
  uint64_t* chunk_len;
  uint32_t* chunk_file;
};
// Enqueues the gear pass, the cut pass and the ordered write of the chunk
// arrays. Afterwards ws + l.counts holds the counts, ws + l.woff / l.wlen the
// chunks' offsets and lengths.
hipError_t cdc_chunk(const CdcLayout& l, const CdcArgs& a, hipStream_t st);
// Chunks [c0, c0 + nb) copied to scratch + po[c] (po: ws + l.po, multiples of
// 16 from 0 within the batch, total_bytes their padded sum).
hipError_t cdc_pack(const CdcLayout& l, const CdcArgs& a, uint64_t c0, uint32_t nb, uint64_t total_bytes,
                    uint8_t* scratch, hipStream_t st);

// ---- windows: chains that start at any cut and stop where they cannot decide ---------
// (include/sdcas.h "chunk windows")
constexpr uint64_t kCdcSegDefault = 1ull << 20;
// the segment length of the cut pass: what was asked for (0: the default), not
// below 2 * max_len, rounded up to a multiple of 64
inline uint64_t cdc_seg_bytes(const CdcParams& p, uint64_t asked) {
  uint64_t x = asked ? asked : kCdcSegDefault;
  if (x > (1ull << 62)) x = 1ull << 62;
  if (x < 2ull * p.max_len) x = 2ull * p.max_len;
  return (x + 63) & ~63ull;
}
// A window of 2 * seg bytes or more is cut segment by segment. Its segments
// number ceil(len / seg) <= len / seg + 1 <= 1.5 * len / seg, so that all the
// segments of a call number at most 1.5 * (1024 * file_slots) / seg; a
// segment's list holds at most ceil(seg / min_len) cuts (the cuts below the
// segment's end lie min_len apart from seg_start + min_len on, and one more
// reaches the end).
struct CdcWinLayout {
  CdcLayout l;
  uint64_t gb;        // u32[n + 1]: the files' first segments (exclusive scan of their segment counts)
  uint64_t scnt;      // u32[max_segs]: the cuts in a segment's speculative list
  uint64_t srec;      // uint4[max_segs]: the stitch's record of a segment (k_cdc_stitch)
  uint64_t spec;      // u64[max_segs * spl]: the lists, a cut's kind in its bits 62..63
  uint64_t max_segs;  // 0: no window of this call can be segmented
  uint64_t spl;       // entries per list
  uint64_t bytes;
};
CdcWinLayout cdc_win_layout(uint64_t n, uint64_t max_chunks, uint64_t file_slots, const CdcParams& p, uint64_t seg);

struct CdcWinArgs {
  const uint8_t* final;  // u8[n], null: every window is final
  uint64_t* consumed;    // u64[n] or null
  uint64_t seg;
};
// cdc_chunk for windows: the same launches but for the cut pass, which is
// k_cdc_cut_seg, k_cdc_stitch and k_cdc_gather. ws + w.l.counts etc. as there.
hipError_t cdc_chunk_windows(const CdcWinLayout& w, const CdcArgs& a, const CdcWinArgs& wa, hipStream_t st);

// ---- sharing -------------------------------------------------------------------------
inline uint64_t cdc_share_cap(uint64_t m) {
  uint64_t cap = 16;
  while (cap < 2 * m) cap <<= 1;
  return cap;
}
// bytes: the table (16 B per slot), 36 B per file, the counts
inline uint64_t cdc_share_ws_bytes(uint64_t m, uint64_t n_files) {
  return 16 * cdc_share_cap(m) + 40 * ((n_files + 1) & ~1ull) + 64;
}
// chunk_file / chunk_len / rep device arrays of m chunks; every output may be
// null; counts u64[kCdcCounts], overwritten
hipError_t cdc_sharing(uint8_t* ws, const uint32_t* chunk_file, const uint64_t* chunk_len, const int64_t* rep,
                       uint32_t m, uint32_t n_files, uint64_t* new_bytes, uint64_t* self_bytes,
                       uint64_t* other_bytes, int64_t* peer, uint64_t* peer_bytes, unsigned long long* counts,
                       hipStream_t st);

}  // namespace sdcas
