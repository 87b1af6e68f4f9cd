/*
 * sdcas.h — C ABI of the MI355X content-identification engine (libsdcas.so).
 *
 * Drop-in boundary for sd-core's content identification. The
 * Rust host keeps its signatures and binds these entry points (cgo-style
 * `extern "C"`, plain pointers and sizes, no ownership transfer; binding shown
 * in INTEGRATION.md):
 *
 *   sdcas_cas_ids        replaces per-file generate_cas_id(path, size)
 *                        core/src/object/cas.rs:23-62, called from
 *                        core/src/object/file_identifier/mod.rs:78-82 (the
 *                        join_all of FileMetadata::new at mod.rs:105-147
 *                        becomes one call per chunk), non_indexed.rs:181,
 *                        location/manager/watcher/utils.rs:236-240
 *   sdcas_checksums      replaces file_checksum(path)
 *                        core/src/object/validation/hash.rs:11-25, called from
 *                        validation/validator_job.rs:154 and watcher/utils.rs:496
 *   sdcas_identify_checksums
 *                        both of the above for a scan that also fills
 *                        integrity_checksum: one open and one read per file
 *   sdcas_dedup          replaces the cas_id -> Object group-by/link of
 *                        file_identifier/mod.rs:149-254 (HashSet at :149-154,
 *                        existing-object lookup :181-188, linear find :214-224,
 *                        new Objects :246-254)
 *   sdcas_*_from_messages / sdcas_hash_messages / sdcas_dev_*
 *                        the same engine on pre-assembled messages (host or
 *                        device memory) for tests and benchmarks
 *
 * Conventions
 *   - Return value: SDCAS_OK (0) or a negative SDCAS_E_* library failure (no
 *     device, invalid arguments, out of memory, HIP error). On failure the
 *     caller falls back to its CPU path for the whole batch.
 *   - Per-item status (out_status): 0, a positive errno from the file I/O, or
 *     SDCAS_STATUS_UNEXPECTED_EOF when read_exact() ran out of file
 *     (cas.rs:36,43,56). The Rust side maps errno with
 *     io::Error::from_raw_os_error, reproducing the per-file skip of
 *     file_identifier/mod.rs:125-141.
 *   - cas keys: u64 whose big-endian bytes are digest bytes 0..7, so
 *     format!("{:016x}", key) == hasher.finalize().to_hex()[..16] (cas.rs:61).
 *     Digests: 32 bytes in BLAKE3 output order; lowercase hex of them is
 *     hash.rs:22-24's to_hex().
 *   - Ownership: the caller owns every input and output array; the library
 *     owns device memory, pinned staging and streams inside the context and
 *     retains no caller pointer after a call returns.
 *   - Threading: calls on one context serialise internally (a mutex on the
 *     host; on the device, a call's stream waits for the previous call's work
 *     whatever stream either names, because they share the context's device
 *     scratch). Use one context per concurrent job for parallelism; the path
 *     calls block, so wrap them in spawn_blocking.
 *   - Progress and cancellation (job/worker.rs:35-36,458-480 kill a job that
 *     reports no progress for 10 minutes; job/mod.rs:862-960 pause/cancel):
 *     the path calls (sdcas_cas_ids, sdcas_checksums, sdcas_hash_messages,
 *     sdcas_cas_ids_from_messages) call the context's progress function after
 *     every staging slot / 1 MiB-piece window completes, with bytes of input
 *     whose results are final, and stop at the next such point once the
 *     cancel flag reads nonzero, returning SDCAS_E_CANCELLED. sdcas_cas_ids
 *     and sdcas_checksums report per item: items already complete keep their
 *     results and status, every other item gets SDCAS_STATUS_CANCELLED. The
 *     two message calls have no per-item status: after SDCAS_E_CANCELLED
 *     their outputs are undefined. The progress function runs on the calling
 *     thread with the context's lock held: it must not call into the same
 *     context.
 *   - Limits: a batch holds at most SDCAS_MAX_BATCH (2^31 - 1) items.
 */
#ifndef SDCAS_H
#define SDCAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDCAS_OK 0
#define SDCAS_E_NO_DEVICE (-1)
#define SDCAS_E_INVALID (-2)
#define SDCAS_E_OOM (-3)
#define SDCAS_E_HIP (-4)
#define SDCAS_E_CAPACITY (-5)
#define SDCAS_E_CANCELLED (-6)

#define SDCAS_STATUS_UNEXPECTED_EOF 100001
/* per-item status of an item the call did not complete because it was
 * cancelled (ECANCELED) */
#define SDCAS_STATUS_CANCELLED 125

#define SDCAS_MAX_BATCH 0x7FFFFFFF

/* constants of core/src/object/cas.rs:10-15 and validation/hash.rs:9 */
#define SDCAS_SAMPLE_COUNT 4
#define SDCAS_SAMPLE_SIZE 10240
#define SDCAS_HEADER_OR_FOOTER_SIZE 8192
#define SDCAS_MINIMUM_FILE_SIZE 102400
#define SDCAS_SAMPLED_MESSAGE_LEN 57352
#define SDCAS_CHECKSUM_BLOCK_LEN 1048576
/* file_identifier/mod.rs:34 */
#define SDCAS_IDENTIFIER_CHUNK_SIZE 100

typedef struct sdcas_ctx sdcas_ctx;

/* Progress report: `done` of `total` bytes of input have final results. Called
 * on the thread that made the path call. */
typedef void (*sdcas_progress_fn)(void *user, uint64_t done, uint64_t total);

/* sdcas_options.flags */
#define SDCAS_OPT_DIRECT_IO 1u /* the path calls (sdcas_cas_ids, sdcas_checksums) read files with
                                   O_DIRECT (cold storage: no page-cache copy; small and unaligned
                                   reads go through an aligned per-thread buffer); a file whose
                                   filesystem refuses O_DIRECT is read through the page cache.
                                   Same bytes, same statuses. */

typedef struct sdcas_options {
  uint32_t struct_size;    /* sizeof(sdcas_options) as the caller compiled it (SDCAS_OPTIONS_INIT sets it):
                              sdcas_init refuses any other size with SDCAS_E_INVALID, so a caller built
                              against another revision of this struct fails loudly instead of passing
                              garbage for the fields it lacks */
  int32_t device;          /* HIP device ordinal (-1: current device) */
  uint32_t io_threads;     /* reader threads of the path calls (0: 16, or the CPU count if lower; at most 256), started by the first one */
  uint32_t flags;          /* SDCAS_OPT_* */
  uint64_t staging_bytes;  /* pinned host staging per batch (0: 256 MiB) */
  sdcas_progress_fn progress;      /* may be NULL; runs on the calling thread and must not call back into
                                      the same context (its lock is held) */
  void *progress_user;             /* passed to progress */
  const volatile int32_t *cancel;  /* may be NULL; caller-owned, read atomically: nonzero cancels */
} sdcas_options;
#define SDCAS_OPTIONS_INIT {(uint32_t)sizeof(sdcas_options), -1, 0, 0, 0, NULL, NULL, NULL}

/* "sdcas-mi355x <major>.<minor>.<patch> (gfx950)"; the C ABI of this header is
 * SDCAS_ABI_VERSION (changes: 2 added sdcas_options.progress/cancel; 3 the
 * struct_size field, sdcas_dedup_window and the dedup step plan; 4
 * sdcas_dev_bind_stream; 5 the combine's output contract: one record per
 * distinct key, any order within an owner's range — same signatures, but a
 * caller that relied on ABI 4's documented key order must change; 6
 * sdcas_file_metadata, and resolve_buckets may overwrite the received
 * records' value words; 7 sdcas_dev_identify and sdcas_identify_checksums) */
#define SDCAS_ABI_VERSION 7
int sdcas_abi_version(void);
const char *sdcas_version(void);

/* Create / destroy a context bound to one GPU. opts may be NULL. */
int sdcas_init(const sdcas_options *opts, sdcas_ctx **out_ctx);
void sdcas_destroy(sdcas_ctx *ctx);
/* Text of the last library failure on this context ("" if none). */
const char *sdcas_last_error(const sdcas_ctx *ctx);
/* Re-bind the progress function and cancel flag (e.g. to the job now using
 * the context); any of them may be NULL. */
int sdcas_set_progress(sdcas_ctx *ctx, sdcas_progress_fn progress, void *user, const volatile int32_t *cancel);

/* ---- the reference functions, batched --------------------------------- */

/* cas_id of n files: generate_cas_id(paths[i], sizes[i]) (cas.rs:23-62).
 * sizes[i] is fs::metadata().len() as the identifier passes it (mod.rs:78-79);
 * it feeds the size prefix and the sample spacing, while file bytes come from
 * the file as it is now. out_keys[i] is valid iff out_status[i] == 0.
 * A small file (size <= 100 KiB) that has grown past its staging room when
 * read is read again with room for its new length, up to 4 times; one that
 * keeps growing through all of them gets out_status EAGAIN (the reference's
 * fs::read would hash whatever it read at that moment — a race with the
 * writer either way; the caller may retry the file later). */
int sdcas_cas_ids(sdcas_ctx *ctx, const char *const *paths, const uint64_t *sizes, size_t n,
                  uint64_t *out_keys, int32_t *out_status);

/* FileMetadata::new (file_identifier/mod.rs:48-96) of n files: fs::metadata,
 * then generate_cas_id(path, len) when the file is not empty (mod.rs:78-86) —
 * the metadata being fstat of the descriptor the cas_id reads use (one path
 * lookup per file; the same statuses). size_hints (may be NULL: one stat
 * pass first) only plan the staging — the indexer's sizes (file_path
 * size_in_bytes); a file of another size now is read again with room for
 * it. Per file: out_sizes[i] the metadata's len, out_flags[i]
 * SDCAS_META_HAS_CAS_ID when out_keys[i] holds the cas key (a non-empty
 * file read without error), SDCAS_META_DIR for a directory (the reference
 * refuses those, mod.rs:67-70; no cas_id), out_status[i] 0 or the errno of
 * the metadata or of the reads (SDCAS_STATUS_UNEXPECTED_EOF as
 * sdcas_cas_ids). ABI 6. */
#define SDCAS_META_HAS_CAS_ID 1u
#define SDCAS_META_DIR 2u
int sdcas_file_metadata(sdcas_ctx *ctx, const char *const *paths, const uint64_t *size_hints, size_t n,
                        uint64_t *out_sizes, uint64_t *out_keys, int32_t *out_status, uint8_t *out_flags);

/* file_checksum of n files (hash.rs:11-25): BLAKE3 of the whole content.
 * out32 receives 32*n bytes. The content hashed is the file's first L bytes,
 * L = its length when the call stats it (hash.rs reads to its first short
 * read, which on a regular local file is EOF): a file that grows while it is
 * read is hashed over L bytes, and one that shrinks below L before its bytes
 * are read gets SDCAS_STATUS_UNEXPECTED_EOF (the reference would hash the
 * shorter content). Neither happens to a file nobody writes meanwhile. */
int sdcas_checksums(sdcas_ctx *ctx, const char *const *paths, size_t n, uint8_t *out32,
                    int32_t *out_status);

/* FileMetadata::new followed by file_checksum of n files from ONE open and ONE
 * read of each: per file the results of sdcas_file_metadata followed by
 * sdcas_checksums on a file nobody writes meanwhile. A file of at most 1 MiB
 * is read once into the staging slot and both hashes come from that copy
 * (up to 100 KiB from one pass of the kernel over it, sdcas_dev_identify); a
 * larger one streams its checksum as sdcas_checksums does and its cas_id
 * windows are read through the same descriptor. Per file: out_sizes[i] the
 * length L from fstat of that descriptor; out_flags[i] SDCAS_META_HAS_CAS_ID
 * when out_keys[i] holds the cas key (a non-empty regular file),
 * SDCAS_META_HAS_CHECKSUM when out32[32 * i ..] holds the digest (every
 * regular file read without error; an empty one gets the empty-input digest,
 * as the validator hashes empty files), SDCAS_META_DIR for a directory
 * (status 0, no outputs); out_status[i] 0, the errno of the metadata, the
 * open or the reads, or SDCAS_STATUS_UNEXPECTED_EOF — a nonzero status means
 * neither result. Both hashes are over the file's first L bytes: a file that
 * grows while it is read is hashed over L bytes, one that shrinks below L
 * gets SDCAS_STATUS_UNEXPECTED_EOF. The path is stat'ed before it is opened
 * and only a regular file is opened: a FIFO, socket or device node gets size
 * 0, flags 0, status 0. size_hints (may be NULL: one stat pass first) only
 * plan the staging, as in sdcas_file_metadata: a file of another size now is
 * read again with room for it, up to 4 times, then gets EAGAIN. An open
 * refused for an empty file leaves status 0 and no checksum. Progress,
 * cancellation, SDCAS_MAX_BATCH and SDCAS_OPT_DIRECT_IO as in the two calls
 * it replaces. ABI 7. */
#define SDCAS_META_HAS_CHECKSUM 4u
int sdcas_identify_checksums(sdcas_ctx *ctx, const char *const *paths, const uint64_t *size_hints, size_t n,
                             uint64_t *out_sizes, uint64_t *out_keys, uint8_t *out32, int32_t *out_status,
                             uint8_t *out_flags);

/* ---- pre-assembled messages in host memory -----------------------------
 *
 * The bytes go through the context's pinned staging slots (a host copy by the
 * I/O threads, overlapped with the GPU). When `blob` is itself page-locked
 * (hipHostMalloc / hipHostRegister) and the messages lie in ascending,
 * non-overlapping ranges at 16-byte aligned offsets, each slot's byte range
 * is DMA'd straight from the caller's buffer instead (no host copy). */

/* BLAKE3 of n messages blob[offsets[i] .. offsets[i]+lens[i]) -> out32 (32*n B). */
int sdcas_hash_messages(sdcas_ctx *ctx, const uint8_t *blob, const uint64_t *offsets,
                        const uint64_t *lens, size_t n, uint8_t *out32);
/* the same, keeping only the cas key of each message */
int sdcas_cas_ids_from_messages(sdcas_ctx *ctx, const uint8_t *blob, const uint64_t *offsets,
                                const uint64_t *lens, size_t n, uint64_t *out_keys);

/* ---- device-resident batches (inputs already in HBM) ------------------- */

/* Size the device workspace for batches of up to max_msgs messages and
 * max_chunks total 1 KiB chunks (sum of max(1, ceil(len/1024))). Allocates;
 * call outside timed regions. */
int sdcas_dev_reserve(sdcas_ctx *ctx, size_t max_msgs, uint64_t max_chunks);
/* Enqueue the hash of n device-resident messages on `stream` (a hipStream_t,
 * NULL = the context's stream). Requirements: every offset 16-byte aligned,
 * and the blob readable for at least 64 bytes past the end of every message.
 * Either output may be NULL. d_blob and d_out32 must be 16-byte aligned and
 * d_out_keys 8-byte aligned (the kernels load the messages and store the
 * digests 16 bytes at a time): SDCAS_E_INVALID otherwise, before anything is
 * enqueued. Asynchronous; sdcas_dev_sync() reports a capacity overflow
 * detected on the device. */
int sdcas_dev_hash_messages(sdcas_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets,
                            const uint64_t *d_lens, size_t n, uint8_t *d_out32, uint64_t *d_out_keys,
                            void *stream);
int sdcas_dev_sync(sdcas_ctx *ctx, void *stream);
/* Content-resident files -> cas key (cas.rs:23-62 with size = d_lens[i]) and
 * BLAKE3(content) (hash.rs:11-25): file i's CONTENT lies at d_blob +
 * d_offsets[i] (16-byte aligned, d_lens[i] bytes, the blob readable 64 B past
 * every end). A file of 1..102400 bytes gets both hashes from one pass over
 * its bytes; a longer one has its cas message (size, header, four samples,
 * footer) gathered on the device and both messages hashed by the batch
 * kernels; an empty one gets no key and the empty-input digest.
 * d_out_has_key[i] = (d_lens[i] != 0). Any output may be NULL. d_blob and
 * d_out32 must be 16-byte aligned and d_out_keys 8-byte aligned
 * (SDCAS_E_INVALID otherwise, before anything is enqueued). Asynchronous,
 * with sdcas_dev_hash_messages's stream rules; sdcas_dev_sync() reports a
 * capacity overflow detected on the device. Workspace (sdcas_dev_reserve):
 * max_msgs >= n, and max_chunks >= the larger of 2 * (A + 2048) and B, where
 * A = sum over files of ceil((len + 8) / 1024) for 1 <= len <= 102400 and 1
 * for any other file (the two hashes' chunk streams each take half of the
 * workspace), and B = sum over the longer files of ceil(len / 1024). At most
 * SDCAS_IDENTIFY_MAX_SAMPLED files of one call may be longer than 102400
 * bytes (each needs 57,360 B of scratch for its gathered message; split a
 * batch holding more). The context's scratch for n files (and n's worth of
 * gathered messages up to that limit) is allocated by the first call that
 * needs it, which waits for the stream: warm up outside timed regions. ABI 7. */
#define SDCAS_IDENTIFY_MAX_SAMPLED 4096
int sdcas_dev_identify(sdcas_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, const uint64_t *d_lens,
                       size_t n, uint64_t *d_out_keys, uint8_t *d_out32, uint8_t *d_out_has_key, void *stream);
/* Name a stream's identity. The device calls of a context share its scratch
 * workspace, so each call makes its stream wait for the previous call's use
 * of it (an event wait: a barrier that idles the GPU ~15 us) unless both ran
 * on the same stream, whose order covers it. A handle alone cannot tell
 * "the same stream" (a destroyed stream's handle can come back for a new
 * one); a token can: consecutive calls on a stream bound with one nonzero
 * token skip the wait. The caller never hands the same token to another
 * stream while the context lives, and binds again (a new token, or 0 to
 * unbind) before destroying a bound stream or reusing its handle for a new
 * one. The end-of-call event a bound stream owes is recorded only when
 * another stream or a host wait needs it (a recorded event idles the GPU
 * ~6-8 us between calls). At most 64 streams per context are bound at once
 * (SDCAS_E_CAPACITY beyond). */
int sdcas_dev_bind_stream(sdcas_ctx *ctx, void *stream, uint64_t token);

/* ---- device-resident big messages, streamed in pieces ------------------
 *
 * file_checksum (hash.rs:11-25) of messages too large to be resident at once
 * (config C4: 1-4 GiB files, 256 GB): the caller delivers each message's
 * bytes in any order as segments already in HBM; every full 1 MiB piece
 * reduces to its level-10 BLAKE3 subtree node on the device, and finish
 * merges each message's nodes into its root.
 *   begin:  nfiles message lengths (host array), each > 1 MiB (smaller
 *           messages go through sdcas_dev_hash_messages).
 *   update: nseg segments (host arrays): bytes [h_msg_off[k], +h_len[k]) of
 *           message h_file[k], resident at device address h_dev_addr[k]
 *           (16-byte aligned, readable 64 B past the end). h_msg_off is a
 *           multiple of 1 MiB; h_len is too unless the segment ends the
 *           message. Every byte of every message exactly once over the
 *           session. Enqueued on `stream`; the segments must stay resident
 *           until the stream has passed this call. Use one stream per session.
 *   finish: 32-byte digests to d_out32 (device, 32*nfiles, 16-byte aligned:
 *           SDCAS_E_INVALID otherwise, and the session stays open), on
 *           `stream`. */
int sdcas_dev_stream_begin(sdcas_ctx *ctx, const uint64_t *lens, size_t nfiles);
int sdcas_dev_stream_update(sdcas_ctx *ctx, size_t nseg, const uint64_t *h_file, const uint64_t *h_msg_off,
                            const uint64_t *h_len, const uint64_t *h_dev_addr, void *stream);
int sdcas_dev_stream_finish(sdcas_ctx *ctx, uint8_t *d_out32, void *stream);
/* One message's pieces split over several GPUs (a file larger
 * than one GPU's share): every rank opens the same session (same lens),
 * updates with its own disjoint segments, exports its node list (32 B per
 * node: one per full 1 MiB piece, then the tail piece's nodes; entries it did
 * not hash are zero), the ranks sum the lists (an all-reduce over int64 words:
 * each entry is nonzero on one rank only), import the sum, and finish. Bytes
 * must equal sdcas_dev_stream_node_bytes(); device pointers; on `stream`. */
size_t sdcas_dev_stream_node_bytes(sdcas_ctx *ctx);
int sdcas_dev_stream_export(sdcas_ctx *ctx, uint8_t *d_dst, size_t bytes, void *stream);
int sdcas_dev_stream_import(sdcas_ctx *ctx, const uint8_t *d_src, size_t bytes, void *stream);

/* ---- dedup / link (file_identifier/mod.rs:149-254) --------------------- */

/* out_link codes besides the ordinals (below) */
#define SDCAS_LINK_DROPPED INT64_MIN             /* I/O error: the file is dropped (mod.rs:125-141) */
#define SDCAS_LINK_DEFERRED (INT64_MIN + 1)      /* no step the job runs reaches the file: it stays an
                                                    orphan for the next batch / job */

/* The file identifier job's step loop around one batch of its orphans
 * (file_identifier_job.rs:86-236). A step reads the next chunk_size orphans
 * with id >= cursor and the cursor becomes its LAST row (:296-319,
 * mod.rs:401-405), so a last row that stays an orphan — an I/O error, or a
 * cas_id of None, which gets an Object but keeps cas_id NULL — is read again
 * by the next step, and the job runs a fixed task_count = ceil(orphans /
 * chunk_size) steps (:146). */
typedef struct sdcas_job_window {
  uint64_t max_steps; /* in: steps the job may still run; 0 = ceil(n / chunk_size), the task_count of a
                         job whose orphans are exactly these n rows */
  uint32_t more;      /* in: nonzero when more orphans follow row n-1: a step that would reach past it is
                         not run (its rows are DEFERRED) */
  uint32_t reserved;
  uint64_t steps;     /* out: steps run over the batch */
  uint64_t rows;      /* out: 1 + the last row the steps read (0: none); the job's next cursor is the id
                         of row rows-1, which the next batch reads again if it is still an orphan */
  uint64_t rereads;   /* out: rows read by two consecutive steps */
} sdcas_job_window;

/* Canonical group-by of the identifier steps over n orphan file_paths in id
 * order, chunk_size rows per step (0 -> 100). has_key[i] == 0 marks a cas_id
 * of None (empty file, mod.rs:78-86); status[i] != 0 drops the file (may be
 * NULL). existing_keys are the cas keys of Objects already in the library,
 * in DB order (may be NULL when n_existing == 0).
 * out_link[i] = i        file i creates a new Object (its last, if two steps read it)
 *             = j < i    file i links to the Object created by file j
 *             = -(e+1)   file i links to existing Object e
 *             = SDCAS_LINK_DROPPED / SDCAS_LINK_DEFERRED
 * *out_created / *out_linked receive the counts identifier_job_step returns
 * (mod.rs:349), summed over the steps. window may be NULL: the whole job over
 * these n rows. */
int sdcas_dedup_window(sdcas_ctx *ctx, const uint64_t *keys, const uint8_t *has_key, const int32_t *status,
                       size_t n, size_t chunk_size, const uint64_t *existing_keys, size_t n_existing,
                       sdcas_job_window *window, int64_t *out_link, int64_t *out_created, int64_t *out_linked);
/* The same steps' bookkeeping on the host, no device: window->steps / rows /
 * rereads for these rows, out_step[i] = the step that first reads row i
 * (UINT64_MAX if none does) and out_reads[i] = how many steps read it (each
 * read of a row without cas_id creates an Object); both may be NULL. The job
 * calls it before writing the cas_ids of the rows its steps read
 * (mod.rs:157-178 precede the existing Object lookup of :181-188);
 * sdcas_dedup_window returns the same window. */
int sdcas_job_plan(const uint8_t *has_key, const int32_t *status, size_t n, size_t chunk_size,
                   sdcas_job_window *window, uint64_t *out_step, uint32_t *out_reads);
/* sdcas_dedup_window with window = NULL */
int sdcas_dedup(sdcas_ctx *ctx, const uint64_t *keys, const uint8_t *has_key, const int32_t *status,
                size_t n, size_t chunk_size, const uint64_t *existing_keys, size_t n_existing,
                int64_t *out_link, int64_t *out_created, int64_t *out_linked);

/* ---- duplicates confirmed by checksum ----------------------------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7: new
 * symbols alone are a compatible change).
 *
 * A cas_id above 100 KiB hashes 57,352 bytes of the file (cas.rs:23-62), so
 * files of one length that agree in those windows share it whatever else they
 * hold, and sdcas_dedup links them to one Object, as the reference does. This
 * group-by over the pair (cas key, 32-byte checksum) — what
 * sdcas_identify_checksums / sdcas_dev_identify return — says which files
 * are equal and which cas keys collide. Files i with valid[i] == 0 take no
 * part (valid may be NULL: all do). A CLASS is the valid files with one key
 * and one digest. Any output may be NULL.
 *   out_rep[i]     lowest valid j with keys[j] == keys[i] and all 32 digest
 *                  bytes equal (i's class); -1 when !valid[i]
 *   out_key_rep[i] lowest valid j with keys[j] == keys[i] (what the cas key
 *                  alone says); -1 when !valid[i]
 *   out_flags[i]   SDCAS_CONFIRM_DUPLICATE: out_rep[i] != i;
 *                  SDCAS_CONFIRM_COLLISION: another valid file has the key
 *                  with a different digest (set on EVERY valid file of such a
 *                  key, also one alone in its class);
 *                  SDCAS_CONFIRM_SKIPPED: !valid[i], no other bit
 * The results are exact and do not depend on scheduling. At most 2^30 files
 * per call (SDCAS_E_CAPACITY beyond); n == 0 is SDCAS_OK with zero counts. */
#define SDCAS_CONFIRM_DUPLICATE 1u
#define SDCAS_CONFIRM_COLLISION 2u
#define SDCAS_CONFIRM_SKIPPED   4u
typedef struct sdcas_confirm_counts {
  uint64_t files;           /* valid files */
  uint64_t classes;         /* distinct (key, digest) pairs */
  uint64_t keys;            /* distinct keys */
  uint64_t collided_keys;   /* keys with at least 2 classes */
  uint64_t collided_files;  /* valid files of collided keys */
  uint64_t duplicate_files; /* files - classes */
} sdcas_confirm_counts;
/* Host arrays: one upload, the group-by, one download. Holds the context as
 * the path calls do (sdcas_dedup's rules). */
int sdcas_confirm_duplicates(sdcas_ctx *ctx, const uint64_t *keys, const uint8_t *digests32, const uint8_t *valid,
                             size_t n, int64_t *out_rep, int64_t *out_key_rep, uint8_t *out_flags,
                             sdcas_confirm_counts *out_counts);
/* Device arrays, asynchronous on `stream` with sdcas_dev_hash_messages's
 * stream rules: takes sdcas_dev_identify's d_out_keys / d_out32 /
 * d_out_has_key as they are. d_digests32 must be 16-byte aligned
 * (SDCAS_E_INVALID otherwise, as for NULL keys or digests with n != 0).
 * d_counts: six u64 in sdcas_confirm_counts' order, overwritten. The
 * context's tables for n files (16 to 32 bytes per file, and 12 more) are
 * allocated by the first call that needs them, which waits for the stream:
 * warm up outside timed regions. */
int sdcas_dev_confirm_duplicates(sdcas_ctx *ctx, const uint64_t *d_keys, const uint8_t *d_digests32,
                                 const uint8_t *d_valid, size_t n, int64_t *d_out_rep, int64_t *d_out_key_rep,
                                 uint8_t *d_out_flags, uint64_t *d_counts, void *stream);

/* ---- duplicate sets: members, sizes and reclaimable bytes ----------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * The grouped, ordered form of sdcas_confirm_duplicates' out_rep, in
 * compressed-row layout. The group-by is over the VALUE rep[i]: files with
 * equal rep[i] carry one label. A file whose rep[i] lies outside [0, n) takes
 * no part (-1, what confirm writes for a skipped file, or anything else; such
 * a value is never used as an index). A SET is a label carried by at least
 * two participating files. sizes[i] is file i's length in bytes; sizes may be
 * NULL (every set_bytes and reclaimable_bytes are then 0), but not with
 * SDCAS_SETS_BY_RECLAIMABLE (SDCAS_E_INVALID, as for an unknown order).
 *   out_set_rep[s]      the set's lowest member
 *   out_set_bytes[s]    sizes[out_set_rep[s]]: the bytes of one copy
 *   out_set_offsets[s]  the members of set s are out_members[out_set_offsets[s]
 *                       .. out_set_offsets[s + 1]), ascending by file index;
 *                       out_set_offsets[0] == 0, out_set_offsets[sets] == members
 * Any output may be NULL. The caller provides n / 2 entries for set_rep and
 * set_bytes, n / 2 + 1 for set_offsets and n for members; entries past sets,
 * sets + 1 and members are left as they were. The results are exact and do
 * not depend on scheduling: two calls on one input give the same bytes. At
 * most 2^30 files per call (SDCAS_E_CAPACITY beyond); n == 0 is SDCAS_OK with
 * zero counts (and out_set_offsets[0] == 0). */
#define SDCAS_SETS_BY_REP          0u  /* sets ordered by their lowest member, ascending */
#define SDCAS_SETS_BY_RECLAIMABLE  1u  /* by reclaimable bytes descending, ties by lowest member ascending */
typedef struct sdcas_sets_counts {
  uint64_t files;             /* files that take part */
  uint64_t sets;              /* labels carried by >= 2 files */
  uint64_t members;           /* files in those sets */
  uint64_t duplicate_files;   /* members - sets */
  uint64_t reclaimable_bytes; /* sum over sets of (count - 1) * set_bytes, modulo 2^64 */
  uint64_t largest_set;       /* members of the largest set, 0 when there is none */
} sdcas_sets_counts;
/* Host arrays: one upload, the device call, the counts down, then exactly
 * sets / members entries down. Holds the context as the path calls do
 * (sdcas_dedup's rules). */
int sdcas_duplicate_sets(sdcas_ctx *ctx, const int64_t *rep, const uint64_t *sizes, size_t n, uint32_t order,
                         int64_t *out_set_rep, uint64_t *out_set_offsets, uint64_t *out_set_bytes,
                         int64_t *out_members, sdcas_sets_counts *out_counts);
/* Device arrays, asynchronous on `stream` with sdcas_dev_hash_messages's
 * stream rules: takes sdcas_dev_confirm_duplicates' d_out_rep as it is, and
 * never waits for the device (the numbers of sets and members stay there;
 * everything sized from them is sized from the bounds n / 2 and n). Every
 * array must be 8-byte aligned (SDCAS_E_INVALID otherwise, as for a NULL
 * d_rep with n != 0). d_counts: six u64 in sdcas_sets_counts' order,
 * overwritten. The context's workspace for n files (36 bytes per file, plus
 * 1 KiB per 4096 files) is allocated by the first call that needs it, which
 * waits for the stream: warm up outside timed regions. */
int sdcas_dev_duplicate_sets(sdcas_ctx *ctx, const int64_t *d_rep, const uint64_t *d_sizes, size_t n, uint32_t order,
                             int64_t *d_set_rep, uint64_t *d_set_offsets, uint64_t *d_set_bytes,
                             int64_t *d_members, uint64_t *d_counts, void *stream);

/* ---- duplicate directories: tree digests and top-most sets ----------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * A tree is n ENTRIES, files and directories in any order: parent[i] is the
 * index of the directory that holds entry i, or -1 for a root (several roots
 * are allowed); is_dir[i] says which kind it is; name32[i] is BLAKE3 of the
 * entry's name bytes (sdcas_hash_messages / sdcas_dev_hash_messages: these
 * calls never see strings). A file takes part with digests32[i] when
 * valid[i] != 0 (valid NULL: every file does). A directory is COMPLETE when
 * every file entry below it, at any depth, is valid; one with no file entry
 * below it is complete and EMPTY. A complete directory d with k direct
 * children has the digest T(d) = BLAKE3(M(d)):
 *   M(d) = "SDTREE01" || le64(k) || R(c_0) || ... || R(c_{k-1})   16 + 72 k bytes
 *   R(c) = name32[c] || content(c) || le64(kind(c))               kind: 0 file, 1 directory
 *   content(c) = digests32[c] for a file, T(c) for a directory
 * with the children in ascending order of name32 compared as 32 bytes
 * (memcmp), equal name32 by ascending entry index. The TREE KEY of d is the
 * u64 whose big-endian bytes are T(d)[0..8), the convention of the cas keys.
 * tree_bytes[i] is sizes[i] for a file and, for a directory, the sum of sizes
 * over every file entry below it modulo 2^64, valid or not (sizes NULL: 0
 * everywhere); tree_files[i] is 1 for a file and the number of file entries
 * below for a directory. The results are exact and do not depend on
 * scheduling: two calls on one input give the same bytes. At most 2^30
 * entries per call; n == 0 is SDCAS_OK with zero counts; any output may be
 * NULL. */
#define SDCAS_TREE_MAX_DEPTH 4096
/* GPU-free, like sdcas_job_plan: checks the shape and describes it.
 * SDCAS_E_CAPACITY for n > 2^30; SDCAS_E_INVALID for a parent outside
 * [-1, n), a parent that is not a directory or an entry that is its own
 * ancestor (a cycle); SDCAS_E_CAPACITY for more than SDCAS_TREE_MAX_DEPTH
 * levels. out_depth[i]: 0 for a root; out_children[i]: direct children;
 * *out_levels: 1 + the largest depth (0 for n == 0). */
int sdcas_tree_plan(const int64_t *parent, const uint8_t *is_dir, size_t n, uint32_t *out_depth,
                    uint64_t *out_children, uint64_t *out_levels);

#define SDCAS_TREE_DIR        1u  /* the entry is a directory */
#define SDCAS_TREE_INCOMPLETE 2u  /* a directory with an invalid file below it: no digest */
#define SDCAS_TREE_EMPTY      4u  /* a directory with no file entry below it */
typedef struct sdcas_tree_counts {
  uint64_t entries;
  uint64_t dirs;
  uint64_t complete_dirs;
  uint64_t empty_dirs;
  uint64_t levels;
  uint64_t largest_dir; /* most direct children */
} sdcas_tree_counts;
/* keys, digests32 and valid are IN for file entries and OUT for directory
 * entries, so that the three arrays go into sdcas_confirm_duplicates as they
 * are:
 *   directory, complete, not empty: digests32 = T(d), keys = tree key, valid = 1
 *   directory, complete, empty:     digests32 = T(d), keys = tree key, valid = 0
 *                                   (takes no part in a group-by)
 *   directory, incomplete:          digests32 = 32 zero bytes, keys = 0, valid = 0
 * File entries' slots are never changed. valid may be NULL (all files valid;
 * nothing is written for directories then: pass out_flags to tell them
 * apart); keys may be NULL; name32 and digests32 may not (SDCAS_E_INVALID with
 * n != 0), and shape errors are sdcas_tree_plan's. Host arrays: one upload,
 * the device call, one download. */
int sdcas_tree_digests(sdcas_ctx *ctx, const int64_t *parent, const uint8_t *is_dir, const uint8_t *name32,
                       const uint64_t *sizes, size_t n, uint64_t *keys, uint8_t *digests32, uint8_t *valid,
                       uint64_t *out_tree_bytes, uint64_t *out_tree_files, uint8_t *out_flags,
                       sdcas_tree_counts *out_counts);
/* parent / is_dir stay HOST arrays (the shape comes from the indexer or the
 * database in every caller, as sdcas_dev_stream_update's descriptors do): the
 * call reads them before it returns. Everything else is device memory.
 * Asynchronous on `stream` with sdcas_dev_hash_messages's stream rules. The
 * shape is checked, and misalignment refused (d_name32 / d_digests32 16-byte
 * aligned, the u64 arrays 8-byte aligned, SDCAS_E_INVALID otherwise), before
 * anything is enqueued. d_counts: six u64 in sdcas_tree_counts' order,
 * overwritten. One hash batch is enqueued per level of directories, deepest
 * first. The context's workspace (52 bytes per entry, 64 per directory of the
 * fullest level, that level's messages, and the batch workspace for them) is
 * grown by the first call that needs it, which waits for the stream: warm up
 * outside timed regions. After that the call waits for the device only when
 * the shape upload of its fourth-last predecessor has not finished. */
int sdcas_dev_tree_digests(sdcas_ctx *ctx, const int64_t *parent, const uint8_t *is_dir, const uint8_t *d_name32,
                           const uint64_t *d_sizes, size_t n, uint64_t *d_keys, uint8_t *d_digests32,
                           uint8_t *d_valid, uint64_t *d_out_tree_bytes, uint64_t *d_out_tree_files,
                           uint8_t *d_out_flags, uint64_t *d_counts, void *stream);

/* Top-most duplicates. rep[i] is any per-entry label, e.g. what
 * sdcas_confirm_duplicates writes when it is run once over ALL entries,
 * directories included; a label outside [0, n) takes no part.
 *   DUP(i):     rep[i] is carried by at least 2 participating entries
 *   NESTED(i):  DUP(i), parent[i] >= 0 and DUP(parent[i]): the entry lies
 *               inside a directory that is itself a duplicate
 *   out_top_rep[i]: rep[i] if DUP(i) and at least one carrier of that label
 *               is not NESTED, else -1
 *   out_flags[i]: SDCAS_TOP_DUP | SDCAS_TOP_NESTED
 * A class whose members are all nested is implied by a set above it and is
 * dropped; a class with a member outside any duplicate directory is kept
 * whole. sdcas_duplicate_sets(out_top_rep, tree_bytes, BY_RECLAIMABLE) is then
 * the report. */
#define SDCAS_TOP_DUP    1u
#define SDCAS_TOP_NESTED 2u
typedef struct sdcas_top_counts {
  uint64_t entries;         /* participating */
  uint64_t dup_entries;
  uint64_t nested_entries;
  uint64_t top_entries;     /* out_top_rep != -1 */
  uint64_t kept_classes;
  uint64_t dropped_classes;
} sdcas_top_counts;
/* Host arrays; a parent outside [-1, n) is SDCAS_E_INVALID here. */
int sdcas_tree_top(sdcas_ctx *ctx, const int64_t *parent, const int64_t *rep, size_t n, int64_t *out_top_rep,
                   uint8_t *out_flags, sdcas_top_counts *out_counts);
/* All device arrays (parent too), 8-byte aligned; a parent outside [-1, n)
 * is treated as -1 and never used as an index, as sdcas_dev_duplicate_sets
 * treats a stray rep. Never waits for the device once the workspace (12
 * bytes per entry) exists. d_counts: six u64 in sdcas_top_counts' order. */
int sdcas_dev_tree_top(sdcas_ctx *ctx, const int64_t *d_parent, const int64_t *d_rep, size_t n,
                       int64_t *d_out_top_rep, uint8_t *d_out_flags, uint64_t *d_counts, void *stream);

/* ---- content-defined chunks: files that share most of their bytes ---------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * File contents resident in memory are cut into chunks at places that depend
 * on the bytes, not on offsets, so that an insertion moves the cuts after it
 * along with the bytes: equal content after a common cut gives equal chunks.
 *   gear table   G[b] = (uint32)(sds_mix64(0x3130304344434453 + b) >> 32), b in
 *                0..255 (include/sdcas_synth.h; the constant is "SDCDC001")
 *   window hash  h(p) = sum over k in 0..min(31, p) of G[x[p - k]] << k mod 2^32:
 *                h = (h << 1) + G[x[p]] run from the file's start. It depends
 *                on at most the 32 bytes ending at p
 *   parameters   (min_len, avg_bits, max_len), avg = 2^avg_bits, valid when
 *                6 <= avg_bits <= 24 and 32 <= min_len < avg < max_len <= 2^28
 *   STRICT(p)    the top avg_bits + 1 bits of h(p) are zero
 *   LOOSE(p)     the top avg_bits - 1 bits of h(p) are zero
 *   cuts         of a file of L bytes, from s = 0 while s < L: if L - s <=
 *                min_len then e = L, else e is the smallest value in
 *                [s + min_len, min(s + max_len, L)] with (e - s < avg and
 *                STRICT(e - 1)) or (e - s >= avg and LOOSE(e - 1)), or
 *                min(s + max_len, L) when there is none; the chunk is [s, e),
 *                then s = e. An END chunk has e == L; any other is a HASH cut
 *                when a candidate was found, else a MAX cut
 * An empty file has no chunk; a file has at most ceil(L / min_len). Chunks
 * are numbered file by file, in file order. A chunk's digest is BLAKE3 of its
 * bytes and its key the digest's bytes 0..8 big-endian, the cas keys'
 * convention, so sdcas_confirm_duplicates(chunk keys, chunk digests) gives
 * rep[c], the lowest chunk with the same bytes. Results are exact and do not
 * depend on scheduling. At most 2^30 chunks (by the bound below) and fewer
 * than 2^32 files per call; the contents are resident as a whole. */
typedef struct sdcas_chunk_params {
  uint32_t min_len;
  uint32_t avg_bits;
  uint32_t max_len;
  uint32_t reserved; /* 0 */
} sdcas_chunk_params;
#define SDCAS_CHUNK_PARAMS_DEFAULT {2048u, 13u, 65536u, 0u}
#define SDCAS_CHUNK_MAX_CHUNKS (1ull << 30)
/* the gear kernel's tile (bytes of one file per workgroup) and strip (bytes
 * per lane): the sizes at which a test looks for a seam */
#define SDCAS_CHUNK_GEAR_TILE 32768u
#define SDCAS_CHUNK_GEAR_STRIP 128u
typedef struct sdcas_chunk_counts {
  uint64_t files;
  uint64_t chunks;
  uint64_t total_bytes; /* the sum of the lengths */
  uint64_t hash_cuts;
  uint64_t max_cuts;
  uint64_t end_chunks; /* the files that are not empty */
} sdcas_chunk_counts;
/* GPU-free, like sdcas_tree_plan: SDCAS_E_INVALID for parameters that are not
 * valid (params NULL: the default), *out_max_chunks = the sum of
 * ceil(len / min_len), the entries a caller provides for every per-chunk
 * array (SDCAS_E_CAPACITY above 2^30), *out_max_slots = the sum of
 * ceil(len / 1024) + max_chunks, which sizes the workspace (256 B per 1 KiB of
 * content for the candidate bitmap, 32 B per possible chunk). */
int sdcas_chunk_plan(const uint64_t *lens, size_t n, const sdcas_chunk_params *params, uint64_t *out_max_chunks,
                     uint64_t *out_max_slots);
/* Host arrays: file i is blob[offsets[i] .. offsets[i] + lens[i]), at any
 * offset. out_file_chunks: n + 1 entries, file i's chunks are
 * [out_file_chunks[i], out_file_chunks[i + 1]); the per-chunk arrays hold
 * max_chunks entries (sdcas_chunk_plan) and entries past counts.chunks are
 * left as they were: out_chunk_off (the chunk's offset in the blob),
 * out_chunk_len, out_chunk_file, out_keys, out_digests32 (32 B each). Any
 * output may be NULL. n == 0 is SDCAS_OK with zero counts and
 * out_file_chunks[0] == 0. One upload, the device call, the counts down, then
 * exactly `chunks` entries of each array. */
int sdcas_chunk_messages(sdcas_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, const uint64_t *lens, size_t n,
                         const sdcas_chunk_params *params, uint64_t *out_file_chunks, uint64_t *out_chunk_off,
                         uint64_t *out_chunk_len, uint32_t *out_chunk_file, uint64_t *out_keys,
                         uint8_t *out_digests32, sdcas_chunk_counts *out_counts);
/* The same over device arrays, enqueued on `stream` with
 * sdcas_dev_hash_messages's stream rules. sdcas_dev_identify's blob contract:
 * d_blob and every offset 16-byte aligned, the blob readable 64 B past every
 * file's end; nothing below d_blob + offsets[i] or at or past offsets[i] +
 * lens[i] + 64 is read. max_chunks / max_slots: sdcas_chunk_plan's of these
 * lengths (lengths on the device that need more are cut short at the bound;
 * nothing is written past it). d_digests32 16-byte aligned, every other array
 * 8-byte (d_chunk_file 4-byte) aligned: SDCAS_E_INVALID otherwise, before
 * anything is enqueued. d_counts: six u64 in sdcas_chunk_counts' order,
 * overwritten.
 * THE CALL WAITS FOR THE DEVICE EXACTLY ONCE when d_keys or d_digests32 is
 * given: after the cut pass it copies the counts and the chunk lengths (8 B
 * per possible chunk) down and plans the hash batches on the host. Cut points
 * fall on any byte and the batch hash takes 16-byte aligned messages, so each
 * batch's chunks are first copied to aligned places in the context's scratch;
 * the environment's SDCAS_CHUNK_PACK_BYTES (default 256 MiB, read per call)
 * caps the packed bytes of a batch, which holds at least one chunk. With
 * neither d_keys nor d_digests32 the call never waits. The workspace and the
 * scratch are grown by the first call that needs them, which waits for the
 * stream: warm up outside timed regions. */
int sdcas_dev_chunk(sdcas_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, const uint64_t *d_lens, size_t n,
                    const sdcas_chunk_params *params, uint64_t max_chunks, uint64_t max_slots,
                    uint64_t *d_file_chunks, uint64_t *d_chunk_off, uint64_t *d_chunk_len, uint32_t *d_chunk_file,
                    uint64_t *d_keys, uint8_t *d_digests32, uint64_t *d_counts, void *stream);

/* ---- chunk windows: a file chunked piece by piece ---------------------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * A window is W bytes of a file that begin at a cut of that file: at byte 0 or
 * at a `consumed` returned for the window before. Its flag `final` says that
 * the window ends where the file ends. The chain runs from s = 0 while s < W:
 *   final        exactly the cuts above with L = W
 *   not final    hi = min(s + max_len, W). If W - s >= min_len and there is a
 *                candidate e in [s + min_len, hi] (the same STRICT / LOOSE
 *                rule), cut at the smallest: a HASH cut. Else if s + max_len
 *                <= W, cut at s + max_len: a MAX cut. Else stop. A window
 *                that is not final never holds an END chunk
 *   consumed     s when the chain stops; W for a final window
 * h(p) depends on the 32 bytes ending at p and min_len >= 32: a chain that
 * starts at a cut s looks at positions >= s + min_len - 1 only, whose 32 bytes
 * lie in [s, ...). So a window gives the cuts the whole file gives from the
 * window's start on, without any byte before it, and
 *   - the caller's next window of that file starts at `consumed`: the bytes
 *     behind it (fewer than max_len) are delivered again with what follows;
 *   - a window of max_len bytes or more that is not final always advances;
 *     a shorter one may return consumed == 0 and no chunk;
 *   - the chunks of a file's windows, one after the other, are the chunks of
 *     the whole file, and the six counts summed over the windows of a
 *     sequence of files are sdcas_chunk_messages' counts over the files:
 *     `files` counts the final windows, `total_bytes` is the sum of consumed;
 *   - no byte at or past `consumed` of a window that is not final is hashed.
 * A window of 2 * seg bytes or more is cut by many waves at once: one chain
 * per segment of seg bytes, started at the segment's first byte, and one wave
 * per window that walks the true chain only until it lands on a cut of the
 * segment's own chain; from there on the two are one, since the chain from a
 * position depends on that position alone. The results do not depend on seg. */
/* GPU-free. The segment length the cut pass uses for these parameters (NULL:
 * the default): SDCAS_CHUNK_SEG_BYTES from the environment (read per call,
 * default 1 MiB), not below 2 * max_len, rounded up to a multiple of 64. 0 for
 * invalid parameters. */
uint64_t sdcas_chunk_seg_bytes(const sdcas_chunk_params *params);
/* sdcas_chunk_messages over windows: final[i] != 0 marks a final window
 * (final NULL: all are, and every output equals sdcas_chunk_messages');
 * out_consumed: n entries. */
int sdcas_chunk_windows(sdcas_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, const uint64_t *lens,
                        const uint8_t *final, size_t n, const sdcas_chunk_params *params, uint64_t *out_file_chunks,
                        uint64_t *out_chunk_off, uint64_t *out_chunk_len, uint32_t *out_chunk_file,
                        uint64_t *out_keys, uint8_t *out_digests32, uint64_t *out_consumed,
                        sdcas_chunk_counts *out_counts);
/* sdcas_dev_chunk over windows, with every contract of that call: the blob's
 * alignment and its 64 readable bytes, nothing read below offsets[i] or at or
 * past offsets[i] + lens[i] + 64, max_chunks / max_slots sdcas_chunk_plan's of
 * the window lengths (a window has at most ceil(len / min_len) chunks too),
 * entries past `chunks` left as they were, any output NULL, n == 0 SDCAS_OK,
 * the alignments (d_consumed 8-byte, d_final any) checked before anything is
 * enqueued, ONE WAIT when d_keys or d_digests32 is given and none otherwise:
 * d_consumed is a device output and costs no wait. The workspace takes, above
 * sdcas_dev_chunk's, about 12 B per possible chunk for the segments' lists (sized
 * from max_chunks, max_slots and the parameters; every index is checked
 * against its bound on the device). With d_final NULL every output equals
 * sdcas_dev_chunk's. */
int sdcas_dev_chunk_windows(sdcas_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, const uint64_t *d_lens,
                            const uint8_t *d_final, size_t n, const sdcas_chunk_params *params, uint64_t max_chunks,
                            uint64_t max_slots, uint64_t *d_file_chunks, uint64_t *d_chunk_off,
                            uint64_t *d_chunk_len, uint32_t *d_chunk_file, uint64_t *d_keys, uint8_t *d_digests32,
                            uint64_t *d_consumed, uint64_t *d_counts, void *stream);

/* Sharing: how many of a file's bytes already occur earlier in the corpus,
 * and which earlier file holds most of them. chunk_file[c], chunk_len[c] and
 * rep[c] describe m chunks of n_files files (sdcas_chunk_messages' arrays and
 * sdcas_confirm_duplicates' out_rep over the chunks). A rep[c] outside [0, c]
 * counts as c and is never used as an index; a chunk whose chunk_file is not
 * below n_files takes no part, and a rep naming such a chunk counts as c.
 *   origin(c) = chunk_file[rep[c]]
 *   B(i, f)   = the sum of chunk_len[c] over file i's chunks with rep[c] != c
 *               and origin(c) == f
 *   out_new_bytes[i]   the sum of chunk_len[c] over i's chunks with rep[c] == c
 *   out_self_bytes[i]  B(i, i)
 *   out_other_bytes[i] the sum of B(i, f) over f != i
 *   out_peer[i]        the f != i with the largest B(i, f) > 0, ties to the
 *                      lowest f; -1 when there is none
 *   out_peer_bytes[i]  B(i, out_peer[i]), or 0
 * All sums are modulo 2^64; the results are exact and do not depend on
 * scheduling. Any output may be NULL; m == 0 and n_files == 0 are SDCAS_OK.
 * At most 2^30 chunks and fewer than 2^32 files (the pair (file, origin) is
 * one 64-bit key): SDCAS_E_CAPACITY beyond. */
typedef struct sdcas_sharing_counts {
  uint64_t files;
  uint64_t chunks;
  uint64_t distinct_chunks; /* rep[c] == c */
  uint64_t total_bytes;
  uint64_t stored_bytes;    /* the sum of chunk_len over first occurrences: what a chunk store keeps */
  uint64_t files_with_peer;
} sdcas_sharing_counts;
/* Host arrays: one upload, the device call, one download. */
int sdcas_chunk_sharing(sdcas_ctx *ctx, const uint32_t *chunk_file, const uint64_t *chunk_len, const int64_t *rep,
                        size_t m, size_t n_files, uint64_t *out_new_bytes, uint64_t *out_self_bytes,
                        uint64_t *out_other_bytes, int64_t *out_peer, uint64_t *out_peer_bytes,
                        sdcas_sharing_counts *out_counts);
/* Device arrays, 8-byte aligned (d_chunk_file 4-byte): SDCAS_E_INVALID
 * otherwise. Never waits for the device once the workspace (32 B per chunk
 * rounded up to a power of two, 40 B per file) exists. d_counts: six u64 in
 * sdcas_sharing_counts' order, overwritten. */
int sdcas_dev_chunk_sharing(sdcas_ctx *ctx, const uint32_t *d_chunk_file, const uint64_t *d_chunk_len,
                            const int64_t *d_rep, size_t m, size_t n_files, uint64_t *d_new_bytes,
                            uint64_t *d_self_bytes, uint64_t *d_other_bytes, int64_t *d_peer, uint64_t *d_peer_bytes,
                            uint64_t *d_counts, void *stream);

/* ---- chunk index: a batch's chunks against the chunks stored before ----------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * The "existing" side of the chunk group-by: what sdcas_dedup's existing_keys
 * are to the cas keys. An INDEX of n entries with directory width `bits`
 * (0 <= bits <= 28, n <= 2^30) is four caller-owned arrays:
 *   keys[n] u64, digests32[n] (32 B each; 16-byte aligned on the device),
 *   values[n] u64 (opaque here; the upper layers store the owning file's id),
 *   with the entries STRICTLY ASCENDING in the pair (key as u64, digest as 32
 *   bytes in memcmp order), so that pairs are distinct. For real chunks the
 *   key is the digest's bytes 0..8 big-endian and this is digest order; any
 *   keys are taken, forged ones too, as sdcas_confirm_duplicates takes them.
 *   dir[2^bits + 1] u32: dir[j] = the number of entries with
 *   keys[i] >> (64 - bits) < j; for bits == 0 the directory is {0, n}. The
 *   last slot is always n.
 * The device calls clamp every directory value to n before use: a directory
 * that does not belong to its arrays gives wrong answers, never an index past
 * them. Results are exact and do not depend on scheduling: two calls on one
 * input give the same bytes. */
#define SDCAS_INDEX_MAX_ENTRIES (1ull << 30)
#define SDCAS_INDEX_MAX_BITS 28u
/* GPU-free. The recommended directory width for n entries: 0 for n < 8, else
 * min(28, ceil_log2(n) - 2): about 4 entries per bucket. */
uint32_t sdcas_chunk_index_dir_bits(uint64_t n);
/* GPU-free, host arrays (used on load from disk): SDCAS_OK when the arrays are
 * an index as defined above. SDCAS_E_CAPACITY for n > 2^30 or bits > 28, before
 * any array is touched. SDCAS_E_INVALID for a NULL array that is needed, or
 * with *out_first_bad (may be NULL) = the first entry i >= 1 that does not
 * order after entry i - 1 or, when the entries are in order, the first
 * directory slot that does not hold its count. */
int sdcas_chunk_index_check(const uint64_t *keys, const uint8_t *digests32, const uint32_t *dir, uint64_t n,
                            uint32_t bits, uint64_t *out_first_bad);

typedef struct sdcas_index_match_counts {
  uint64_t queries; /* valid queries */
  uint64_t hits;
  uint64_t misses;
  uint64_t skipped; /* !valid */
} sdcas_index_match_counts;
/* Read-only match of m queries (keys, digests32, valid: sdcas_confirm_duplicates'
 * inputs; valid NULL: all are valid) against the index; its cost follows m, not n:
 *   out_pos[c]    the entry i with idx_keys[i] == keys[c] and all 32 digest
 *                 bytes equal; -1 when there is none or !valid[c]
 *   out_value[c]  idx_values[i], or 0
 * Any output may be NULL; m == 0 and n == 0 are SDCAS_OK. Host arrays: one
 * upload of the index and the batch, the device call, one download (a caller
 * that keeps an index should keep it on the device and use the call below). */
int sdcas_chunk_index_match(sdcas_ctx *ctx, const uint64_t *idx_keys, const uint8_t *idx_digests32,
                            const uint64_t *idx_values, const uint32_t *idx_dir, uint64_t n, uint32_t bits,
                            const uint64_t *keys, const uint8_t *digests32, const uint8_t *valid, size_t m,
                            int64_t *out_pos, uint64_t *out_value, sdcas_index_match_counts *out_counts);
/* Device arrays, asynchronous on `stream` with sdcas_dev_hash_messages's
 * stream rules. Both digest arrays 16-byte aligned, the u64 arrays and the
 * outputs 8-byte, d_idx_dir 4-byte (SDCAS_E_INVALID otherwise, as for a NULL
 * array that is needed); n > 2^30, m > 2^30 or bits > 28 is SDCAS_E_CAPACITY;
 * both are reported before anything is enqueued. d_counts: four u64 in
 * sdcas_index_match_counts' order, overwritten. The call never waits for the
 * device and uses no workspace. */
int sdcas_dev_chunk_index_match(sdcas_ctx *ctx, const uint64_t *d_idx_keys, const uint8_t *d_idx_digests32,
                                const uint64_t *d_idx_values, const uint32_t *d_idx_dir, uint64_t n, uint32_t bits,
                                const uint64_t *d_keys, const uint8_t *d_digests32, const uint8_t *d_valid, size_t m,
                                int64_t *d_out_pos, uint64_t *d_out_value, uint64_t *d_counts, void *stream);

/* Add: the NEW index is the sorted distinct union of the old entries and the
 * valid pairs of the batch, with its directory at bits_new (the widths may
 * differ: growing re-buckets). A pair the old index holds keeps the old
 * value; a new pair takes values[c] of the LOWEST batch position c that holds
 * it. The new keys / digests32 / values arrays hold n_old + m entries, of
 * which the first entries_new are written and the rest left as they were;
 * new_dir holds 2^bits_new + 1.
 *   out_pos[c]    the pair's entry in the new index; -1 when !valid[c]
 *   out_flags[c]  SDCAS_INDEX_HIT: the pair was in the old index;
 *                 SDCAS_INDEX_ADDED: the pair is new and values[c] was stored;
 *                 SDCAS_INDEX_SKIPPED: !valid[c];
 *                 0: a later copy, within the batch, of an added pair
 * queries == hits + added + batch_duplicates. Old and new arrays must not
 * overlap (checked from pointers and sizes: SDCAS_E_INVALID); n_old + m <=
 * 2^30 (SDCAS_E_CAPACITY). values NULL: every stored value is 0. out_pos,
 * out_flags and the counts may be NULL. */
#define SDCAS_INDEX_HIT     1u
#define SDCAS_INDEX_ADDED   2u
#define SDCAS_INDEX_SKIPPED 4u
typedef struct sdcas_index_add_counts {
  uint64_t queries; /* valid batch entries */
  uint64_t hits;
  uint64_t added;
  uint64_t batch_duplicates;
  uint64_t entries_old;
  uint64_t entries_new; /* entries_old + added */
} sdcas_index_add_counts;
/* Host arrays: one upload, the device call, the counts down, then exactly
 * entries_new entries of the new arrays and the new directory. */
int sdcas_chunk_index_add(sdcas_ctx *ctx, const uint64_t *old_keys, const uint8_t *old_digests32,
                          const uint64_t *old_values, const uint32_t *old_dir, uint64_t n_old, uint32_t bits_old,
                          const uint64_t *keys, const uint8_t *digests32, const uint64_t *values,
                          const uint8_t *valid, size_t m, uint64_t *new_keys, uint8_t *new_digests32,
                          uint64_t *new_values, uint32_t *new_dir, uint32_t bits_new, int64_t *out_pos,
                          uint8_t *out_flags, sdcas_index_add_counts *out_counts);
/* Device arrays, asynchronous on `stream`, alignments as for the match
 * (d_out_flags any). d_counts: six u64 in sdcas_index_add_counts' order,
 * overwritten: entries_new stays on the device, and every grid is sized from
 * the bounds m and n_old. The context's workspace for a batch of m (about 100
 * bytes per batch entry with the group-by's tables; nothing that grows with
 * n_old) is allocated by the first call that needs it, which waits for the
 * stream: warm up outside timed regions. After that the call never waits. */
int sdcas_dev_chunk_index_add(sdcas_ctx *ctx, const uint64_t *d_old_keys, const uint8_t *d_old_digests32,
                              const uint64_t *d_old_values, const uint32_t *d_old_dir, uint64_t n_old,
                              uint32_t bits_old, const uint64_t *d_keys, const uint8_t *d_digests32,
                              const uint64_t *d_values, const uint8_t *d_valid, size_t m, uint64_t *d_new_keys,
                              uint8_t *d_new_digests32, uint64_t *d_new_values, uint32_t *d_new_dir,
                              uint32_t bits_new, int64_t *d_out_pos, uint8_t *d_out_flags, uint64_t *d_counts,
                              void *stream);

/* ---- holders index: a chunk index that can forget files ----------------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * The chunk index above keeps, per pair, the value that came first and so can
 * only grow. A HOLDERS INDEX keeps every holder: the same four caller-owned
 * arrays (keys[n], digests32[n], values[n], dir[2^bits + 1]; the directory
 * rule, the limits n <= 2^30 and bits <= 28 and the alignments are the chunk
 * index's), with the entries STRICTLY ASCENDING in the TRIPLE (key as u64,
 * digest as 32 bytes in memcmp order, value as unsigned 64-bit). A pair may
 * repeat, once per distinct value; the upper layers store file ids, so the
 * first entry of a pair's run is its lowest holder and the run's length is the
 * number of files that hold the pair. Every valid chunk index is a valid
 * holders index (strict in the pair implies strict in the triple); values
 * NULL stands for all 0, which allows each pair once.
 * A run is not bounded by anything (every sparse file holds the all-zero
 * chunk): no call's cost per thread follows a run's length, and forged keys
 * (one key, many digests) are taken as before. Directory values are clamped
 * to n; results are exact and do not depend on scheduling.
 * sdcas_chunk_index_dir_bits serves both kinds. */
/* GPU-free, host arrays: as sdcas_chunk_index_check, in the triple order.
 * *out_first_bad (may be NULL) = the first entry i >= 1 whose triple does not
 * order after entry i - 1's or, when the entries are in order, the first
 * directory slot that does not hold its count. */
int sdcas_chunk_holders_check(const uint64_t *keys, const uint8_t *digests32, const uint64_t *values,
                              const uint32_t *dir, uint64_t n, uint32_t bits, uint64_t *out_first_bad);

/* Read-only match; the inputs and the counts are sdcas_chunk_index_match's:
 *   out_pos[c]      the FIRST entry with c's pair; -1 when there is none or !valid[c]
 *   out_value[c]    that entry's value: the lowest holder; or 0
 *   out_holders[c]  the number of entries with the pair, or 0
 * Both ends of the run are found by halving inside the key's bucket: the cost
 * follows m, not n and not the run. Any output may be NULL. */
int sdcas_chunk_holders_match(sdcas_ctx *ctx, const uint64_t *idx_keys, const uint8_t *idx_digests32,
                              const uint64_t *idx_values, const uint32_t *idx_dir, uint64_t n, uint32_t bits,
                              const uint64_t *keys, const uint8_t *digests32, const uint8_t *valid, size_t m,
                              int64_t *out_pos, uint64_t *out_value, uint32_t *out_holders,
                              sdcas_index_match_counts *out_counts);
/* Device arrays: sdcas_dev_chunk_index_match's rules (d_out_holders 4-byte
 * aligned). Never waits for the device and uses no workspace. */
int sdcas_dev_chunk_holders_match(sdcas_ctx *ctx, const uint64_t *d_idx_keys, const uint8_t *d_idx_digests32,
                                  const uint64_t *d_idx_values, const uint32_t *d_idx_dir, uint64_t n, uint32_t bits,
                                  const uint64_t *d_keys, const uint8_t *d_digests32, const uint8_t *d_valid,
                                  size_t m, int64_t *d_out_pos, uint64_t *d_out_value, uint32_t *d_out_holders,
                                  uint64_t *d_counts, void *stream);

/* Add: the NEW index is the sorted distinct union of the old triples and the
 * batch's valid triples (keys[c], digests32[c], values[c]; values NULL: 0),
 * in arrays of n_old + m entries with the directory at bits_new, as
 * sdcas_chunk_index_add. Read per TRIPLE:
 *   out_pos[c]    the triple's entry in the new index; -1 when !valid[c]
 *   out_flags[c]  SDCAS_INDEX_HIT: the old index held the triple (this file
 *                 already held this chunk); SDCAS_INDEX_ADDED: the triple is
 *                 new and c is the lowest batch position with it;
 *                 SDCAS_INDEX_SKIPPED: !valid[c]; 0: a later batch position
 *                 with the same new triple
 * queries == hits + added + batch_duplicates. The overlap and capacity rules
 * are sdcas_chunk_index_add's. */
int sdcas_chunk_holders_add(sdcas_ctx *ctx, const uint64_t *old_keys, const uint8_t *old_digests32,
                            const uint64_t *old_values, const uint32_t *old_dir, uint64_t n_old, uint32_t bits_old,
                            const uint64_t *keys, const uint8_t *digests32, const uint64_t *values,
                            const uint8_t *valid, size_t m, uint64_t *new_keys, uint8_t *new_digests32,
                            uint64_t *new_values, uint32_t *new_dir, uint32_t bits_new, int64_t *out_pos,
                            uint8_t *out_flags, sdcas_index_add_counts *out_counts);
/* Device arrays, as sdcas_dev_chunk_index_add. The context's workspace for a
 * batch of m is 16 bytes per batch entry (two orders of the batch positions,
 * the lower bounds and their compaction) and 1/64 word of counts; nothing
 * grows with n_old. The batch is ordered by ceil_log2(m) merge passes. The
 * first call that needs the workspace allocates it and waits for the stream;
 * after that the call never waits. */
int sdcas_dev_chunk_holders_add(sdcas_ctx *ctx, const uint64_t *d_old_keys, const uint8_t *d_old_digests32,
                                const uint64_t *d_old_values, const uint32_t *d_old_dir, uint64_t n_old,
                                uint32_t bits_old, const uint64_t *d_keys, const uint8_t *d_digests32,
                                const uint64_t *d_values, const uint8_t *d_valid, size_t m, uint64_t *d_new_keys,
                                uint8_t *d_new_digests32, uint64_t *d_new_values, uint32_t *d_new_dir,
                                uint32_t bits_new, int64_t *d_out_pos, uint8_t *d_out_flags, uint64_t *d_counts,
                                void *stream);

/* Remove: the NEW index is the old entries whose value is not in removed[r]
 * (u64, STRICTLY ASCENDING, r <= 2^30), in their old order: byte for byte the
 * index built from the holders that remain. The new keys / digests32 / values
 * arrays hold n_old entries, of which the first entries_new are written and
 * the rest left as they were; new_dir holds 2^bits_new + 1 and is rebuilt, so
 * the widths may differ. The old index streams through once (48 bytes in per
 * entry, at most 48 out), `removed` is the only thing searched, by halving.
 * Old and new arrays must not overlap, nor `removed` and the new arrays
 * (checked from pointers and sizes: SDCAS_E_INVALID). r == 0 copies the old
 * entries and re-buckets; n_old == 0 is SDCAS_OK. */
typedef struct sdcas_holders_remove_counts {
  uint64_t entries_old;
  uint64_t removed;     /* entries taken out */
  uint64_t entries_new; /* entries_old - removed */
  uint64_t values;      /* r */
} sdcas_holders_remove_counts;
/* Host arrays: also SDCAS_E_INVALID, before the device is touched, for a
 * `removed` that is not strictly ascending. One upload, the device call, the
 * counts down, then exactly entries_new entries and the new directory. */
int sdcas_chunk_holders_remove(sdcas_ctx *ctx, const uint64_t *old_keys, const uint8_t *old_digests32,
                               const uint64_t *old_values, const uint32_t *old_dir, uint64_t n_old,
                               uint32_t bits_old, const uint64_t *removed, size_t r, uint64_t *new_keys,
                               uint8_t *new_digests32, uint64_t *new_values, uint32_t *new_dir, uint32_t bits_new,
                               sdcas_holders_remove_counts *out_counts);
/* Device arrays, asynchronous on `stream`, alignments as for the match
 * (d_removed 8-byte). d_counts: four u64 in sdcas_holders_remove_counts'
 * order, overwritten: entries_new stays on the device. `removed` cannot be
 * checked without reading it: one that is not ascending gives a wrong
 * selection of entries, never a store outside the arrays (every place is a
 * rank among at most n_old kept entries, checked against n_old). The
 * workspace is the keep masks and the kept counts, 36 bytes and a little per
 * 256 entries, allocated by the first call that needs it (which waits for the
 * stream); after that the call never waits. */
int sdcas_dev_chunk_holders_remove(sdcas_ctx *ctx, const uint64_t *d_old_keys, const uint8_t *d_old_digests32,
                                   const uint64_t *d_old_values, const uint32_t *d_old_dir, uint64_t n_old,
                                   uint32_t bits_old, const uint64_t *d_removed, size_t r, uint64_t *d_new_keys,
                                   uint8_t *d_new_digests32, uint64_t *d_new_values, uint32_t *d_new_dir,
                                   uint32_t bits_new, uint64_t *d_counts, void *stream);

/* ---- chunk peers: the files that hold most of a file's bytes --------------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * sdcas_chunk_sharing credits each shared chunk to ONE file, its origin (the
 * lowest holder), which was all a chunk index could say. A holders index keeps
 * every holder, and this call reads them: for a batch's chunks it computes,
 * per batch file, the bytes it shares with EVERY file that holds any of them,
 * and returns the top k files per file. Of three versions of a log with ids
 * 1 < 2 < 3, v1 = A, v2 = A B, v3 = A B C, sharing reports v1 (|A| bytes) for
 * v3; here v3's first peer is v2 with |A| + |B|. The call sits beside
 * sdcas_chunk_sharing (the new / self / other byte split is still that call's)
 * and changes no index.
 *   inputs   a holders index (idx_keys, idx_digests32, idx_values, idx_dir, n,
 *            bits: its limits, alignments and directory clamping); a batch of m
 *            chunks (keys, digests32, valid: NULL means all valid,
 *            chunk_file[m] u32, chunk_len[m] u64); file_ids[n_files] u64, the id
 *            each batch file has in the index; k in [1, 64]; max_holders H in
 *            [1, 2^20]; mode; max_pairs. A chunk takes no part when it is not
 *            valid or chunk_file[c] >= n_files.
 *   modes    SDCAS_PEERS_EARLIER: the COUNTED holders of chunk c of file i are
 *            the entries of c's pair whose value is BELOW file_ids[i];
 *            SDCAS_PEERS_ALL: the entries whose value is NOT EQUAL to it. Both
 *            are contiguous pieces of the pair's run: its two ends and the
 *            place of (key, digest, file_ids[i]) in it are found by halving, so
 *            cnt(c), their number, costs three halvings and no thread walks a
 *            run.
 *   common   a chunk with cnt(c) > H is COMMON (the zero chunk of sparse files,
 *            a template header): it scores for nobody and its length goes to
 *            out_common_bytes[i]. A definition, not a fallback: it bounds the
 *            expansion and keeps ubiquitous content from deciding the nearest
 *            file. In EARLIER mode cnt looks only at ids below the file's own,
 *            so a file's result does not depend on which later files the index
 *            already holds.
 *   score    S(i, f) = the sum, modulo 2^64, of chunk_len[c] over i's
 *            participating chunks that are not common and of which f is a
 *            counted holder; a chunk that occurs twice in i counts twice. The
 *            PEERS of i are the f with at least one such chunk, ordered by (S
 *            descending, f ascending as u64); the first k are returned.
 *   outputs  out_peer_count[n_files] u32: min(k, the number of peers);
 *            out_peers[n_files * k] and out_peer_bytes[n_files * k] u64: row i
 *            in peer order, slots past the count 0; out_shared_bytes[i]: the
 *            bytes of i's chunks with 1 <= cnt <= H, out_unique_bytes[i]: of
 *            those with cnt == 0, out_common_bytes[i]: of the common ones.
 *            shared + unique + common is the sum of i's participating chunk
 *            lengths modulo 2^64. Any output may be NULL; every slot of a given
 *            array is written, so two calls give the same bytes.
 *   capacity the expansion holds max_pairs (chunk, holder) pairs. With P, the
 *            sum of cnt over the chunks that are not common, above max_pairs
 *            the device form sets overflow, writes every peer_count as 0 and
 *            zeroes the peer rows; the three byte arrays and the counts other
 *            than edges and files_with_peer are still exact. The host form then
 *            returns SDCAS_E_CAPACITY (its outputs written as the device
 *            form's).
 * SDCAS_E_INVALID for k, H or mode out of range, a needed NULL array or a
 * misalignment; SDCAS_E_CAPACITY for m > 2^30, n > 2^30, bits > 28, n_files >
 * 2^32 - 2 or max_pairs > 2^30: all before anything is enqueued. Results are
 * exact and do not depend on scheduling. */
#define SDCAS_PEERS_EARLIER 0u
#define SDCAS_PEERS_ALL 1u
#define SDCAS_PEERS_MAX_K 64u
#define SDCAS_PEERS_MAX_HOLDERS (1u << 20)
#define SDCAS_PEERS_MAX_PAIRS (1ull << 30)
typedef struct sdcas_peers_counts {
  uint64_t files;           /* n_files */
  uint64_t chunks;          /* participating chunks */
  uint64_t common_chunks;
  uint64_t pairs;           /* P */
  uint64_t edges;           /* distinct (i, f) with a scoring chunk; 0 on overflow */
  uint64_t files_with_peer; /* 0 on overflow */
  uint64_t overflow;        /* 1: P > max_pairs */
} sdcas_peers_counts;
/* GPU-free, like sdcas_chunk_plan: the range checks above (k, H; m, n_files),
 * *out_max_pairs = min(m * H, 2^30), the bound that can never overflow, and
 * *out_workspace_bytes = what the device call takes for that many pairs (16
 * bytes per chunk, 57 per pair). Either output may be NULL. */
int sdcas_chunk_peers_plan(uint64_t m, uint64_t n_files, uint32_t k, uint32_t max_holders, uint64_t *out_max_pairs,
                           uint64_t *out_workspace_bytes);
/* Host arrays; max_pairs == 0 means the plan's bound. One upload of the index
 * and the batch, the device call, one download. */
int sdcas_chunk_peers(sdcas_ctx *ctx, const uint64_t *idx_keys, const uint8_t *idx_digests32,
                      const uint64_t *idx_values, const uint32_t *idx_dir, uint64_t n, uint32_t bits,
                      const uint64_t *keys, const uint8_t *digests32, const uint8_t *valid,
                      const uint32_t *chunk_file, const uint64_t *chunk_len, size_t m, const uint64_t *file_ids,
                      size_t n_files, uint32_t k, uint32_t max_holders, uint32_t mode, uint64_t max_pairs,
                      uint32_t *out_peer_count, uint64_t *out_peers, uint64_t *out_peer_bytes,
                      uint64_t *out_shared_bytes, uint64_t *out_unique_bytes, uint64_t *out_common_bytes,
                      sdcas_peers_counts *out_counts);
/* Device arrays under sdcas_dev_chunk_holders_match's stream and alignment
 * rules; d_chunk_file and d_out_peer_count 4-byte aligned, d_file_ids,
 * d_chunk_len and the u64 outputs 8-byte. max_pairs is taken as given (0 holds
 * no pair). d_counts: seven u64 in sdcas_peers_counts' order, overwritten. The
 * workspace for (m, max_pairs) is allocated by the first call that needs it,
 * which waits for the stream; after that the call never waits for the device.
 * Every grid is sized from m, n_files and max_pairs: P and the edges stay on
 * the device, the two orders take ceil_log2(max_pairs) merge passes each. */
int sdcas_dev_chunk_peers(sdcas_ctx *ctx, const uint64_t *d_idx_keys, const uint8_t *d_idx_digests32,
                          const uint64_t *d_idx_values, const uint32_t *d_idx_dir, uint64_t n, uint32_t bits,
                          const uint64_t *d_keys, const uint8_t *d_digests32, const uint8_t *d_valid,
                          const uint32_t *d_chunk_file, const uint64_t *d_chunk_len, size_t m,
                          const uint64_t *d_file_ids, size_t n_files, uint32_t k, uint32_t max_holders,
                          uint32_t mode, uint64_t max_pairs, uint32_t *d_out_peer_count, uint64_t *d_out_peers,
                          uint64_t *d_out_peer_bytes, uint64_t *d_out_shared_bytes, uint64_t *d_out_unique_bytes,
                          uint64_t *d_out_common_bytes, uint64_t *d_counts, void *stream);

/* ---- file families: the files that are versions of one another -----------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * sdcas_chunk_peers answers, once per file, "which k files hold most of this
 * file's bytes". Twelve versions of a log come back as twelve rows that point
 * at each other. This call is the group-by over those rows: the FAMILY of a
 * file is its connected component in the graph whose edges are the peer slots
 * that pass a shared-bytes threshold. It changes no index.
 *   inputs   n rows, one per file: ids[n] u64, the file id of row i, STRICTLY
 *            ASCENDING (the law of ids in scan order; it makes id -> row one
 *            lower bound by halving, with no sort); sizes[n] u64;
 *            peer_count[n] u32, peers[n * k] and peer_bytes[n * k] u64: exactly
 *            sdcas_dev_chunk_peers' out_peer_count, out_peers and
 *            out_peer_bytes; k in [1, SDCAS_PEERS_MAX_K]; a threshold num / den,
 *            both u32, den >= 1 and num <= den.
 *   slots    row i has min(peer_count[i], k) slots; slots past that count are
 *            never read. Slot (i, s) names f = peers[i * k + s] with b =
 *            peer_bytes[i * k + s] and is exactly one of
 *              missing  f is not in ids (a removed file, a file outside the rows)
 *              self     f == ids[i]
 *              weak     f is row j, and b == 0 or
 *                       b * den < num * max(sizes[i], sizes[j])
 *              link     f is row j, b > 0 and
 *                       b * den >= num * max(sizes[i], sizes[j])
 *            The comparison is exact: the products reach 2^96 and are compared
 *            in 128 bits. The size is the LARGER of the two: a small file
 *            embedded in a large archive does not join the archive's family,
 *            which is the "versions of one file" meaning. num = 0 links every
 *            slot with b > 0.
 *   family   the links, taken as undirected edges, partition the rows into
 *            components. out_family[i] (int64) is the LOWEST ROW INDEX of i's
 *            component; a file with no link has out_family[i] == i. The array
 *            is a valid rep for sdcas_dev_duplicate_sets, and a family is a
 *            set there. out_family_size[i] (u32) is the number of rows of i's
 *            component.
 *   unsorted the device form checks the order of ids on the device; where it
 *            is broken it sets unsorted = 1, writes out_family[i] = i and
 *            out_family_size[i] = 1, and every count but files and unsorted is
 *            0: no garbage and no host wait. The host form checks on the host
 *            before anything is uploaded and returns SDCAS_E_INVALID.
 * SDCAS_E_INVALID for k, num or den out of range, a needed NULL array or a
 * misalignment (8 bytes for u64 and int64, 4 for u32); SDCAS_E_CAPACITY for n >
 * 2^30: all before anything is enqueued. n == 0 is SDCAS_OK with zero counts.
 * Any output may be NULL; every slot of a given output is written. Results are
 * exact and do not depend on scheduling: the lowest index of a component is a
 * property of the graph, the sizes and counts are sums and a maximum. */
typedef struct sdcas_families_counts {
  uint64_t files;      /* n */
  uint64_t slots;      /* slots read */
  uint64_t missing;    /* slots classed missing */
  uint64_t self_slots; /* slots classed self */
  uint64_t weak;       /* slots classed weak */
  uint64_t links;      /* directed slots that link; a pair that lists each other counts twice */
  uint64_t families;   /* components with at least 2 rows */
  uint64_t members;    /* rows in those components */
  uint64_t largest;    /* rows in the largest family, 0 when there is none */
  uint64_t unsorted;   /* 1: ids is not strictly ascending */
} sdcas_families_counts;
/* GPU-free: the range checks above (k, n) and *out_workspace_bytes = what the
 * device call takes (8 bytes per row and a little). The output may be NULL. */
int sdcas_file_families_plan(uint64_t n, uint32_t k, uint64_t *out_workspace_bytes);
/* Host arrays: one upload, the device call, one download. */
int sdcas_file_families(sdcas_ctx *ctx, const uint64_t *ids, const uint64_t *sizes, const uint32_t *peer_count,
                        const uint64_t *peers, const uint64_t *peer_bytes, size_t n, uint32_t k, uint32_t num,
                        uint32_t den, int64_t *out_family, uint32_t *out_family_size,
                        sdcas_families_counts *out_counts);
/* Device arrays under sdcas_dev_chunk_peers' stream rules. d_counts: ten u64 in
 * sdcas_families_counts' order, overwritten. The workspace for n is allocated
 * by the first call that needs it, which waits for the stream; after that the
 * call never waits for the device. Every grid is sized from n and the labels
 * are flattened by ceil_log2(n) launches, whatever the data; inside the union
 * kernel a thread's search for a root follows the depth of the forest at that
 * moment. */
int sdcas_dev_file_families(sdcas_ctx *ctx, const uint64_t *d_ids, const uint64_t *d_sizes,
                            const uint32_t *d_peer_count, const uint64_t *d_peers, const uint64_t *d_peer_bytes,
                            size_t n, uint32_t k, uint32_t num, uint32_t den, int64_t *d_out_family,
                            uint32_t *d_out_family_size, uint64_t *d_counts, void *stream);

/* ---- family bytes: what a family's versions store and give back -----------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * sdcas_file_families says that twelve versions of a log are one family. This
 * call says what the twelve cost, what keeping each chunk once gives back, and
 * which family to look at first: sdcas_chunk_sharing's accounting INSIDE every
 * family, and the families that have two rows or more ranked by the bytes they
 * give back, in the shape of sdcas_duplicate_sets. A chunk that two unrelated
 * files happen to share is reclaimed for neither family.
 *   inputs   sdcas_chunk_sharing's and a label per file: chunk_file[m] u32, the
 *            file of chunk c; chunk_len[m] u64; rep[m] int64,
 *            sdcas_confirm_duplicates' out_rep over the chunks; family[n_files]
 *            int64, a label per file. The group-by is over the label's VALUE, as
 *            in sdcas_duplicate_sets: sdcas_file_families' out_family is a valid
 *            input as it is, and so is any other per-file label (confirm's rep
 *            over files, top_rep).
 *   row      row i takes part when 0 <= family[i] < n_files; its label is that
 *            value. It is never used as an index into the chunk arrays.
 *   chunk    chunk c takes part when chunk_file[c] < n_files and that row
 *            takes part. Its class number is r(c) = rep[c] when 0 <= rep[c] <= c,
 *            else c: a number only, never an index. Its CLASS is the pair
 *            (label of its row, r(c)); the FIRST OCCURRENCE of a class is its
 *            lowest participating chunk position.
 *   per row  the sums of chunk_len over the row's participating chunks, modulo
 *            2^64; rows that take no part get 0:
 *              out_file_bytes[i]       all of them
 *              out_delta_bytes[i]      those that are their class's first
 *                                      occurrence: what row i adds to its family
 *              out_self_bytes[i]       those whose class's first occurrence is
 *                                      an earlier chunk of row i itself
 *              out_inherited_bytes[i]  those whose class's first occurrence lies
 *                                      in another row of the family
 *            file = delta + self + inherited holds for every row.
 *   per label  total: the sum of file_bytes over its rows; stored: the sum of
 *            delta_bytes over its rows; reclaimable = total - stored, modulo 2^64.
 *   sets     a SET is a label carried by at least two participating rows. The
 *            sets are written in order of (reclaimable descending, lowest member
 *            row ascending): out_set_rep[s] int64, the set's lowest member row
 *            (as in sdcas_duplicate_sets); out_set_files[s] u32, its rows;
 *            out_set_total[s] and out_set_stored[s] u64. The caller provides
 *            n_files / 2 entries for each set array; entries past `sets` are
 *            left as they were.
 * Example: n_files = 4, family = [0, 0, 2, 0], seven chunks
 *     chunk  file  len  rep
 *     c0     0     10   0    first of class (0, 0): delta
 *     c1     0     10   0    first occurrence in its own row: self
 *     c2     1     10   0    first occurrence in row 0: inherited
 *     c3     1      5   3    first of class (0, 3): delta
 *     c4     2     10   0    label 2, first of class (2, 0): delta
 *     c5     3      5   3    first occurrence in row 1: inherited
 *     c6     3      7   6    first of class (0, 6): delta
 *   rows (file, delta, self, inherited): (20, 10, 10, 0), (15, 5, 0, 10),
 *   (10, 10, 0, 0), (12, 7, 0, 5). Row 2 is alone in label 2: the chunk it
 *   shares with label 0 is reclaimed by nobody. One set: rep 0, files 3, total
 *   47, stored 22. Counts: files 4, chunks 7, classes 4, total_bytes 57,
 *   stored_bytes 32, sets 1, members 3, set_reclaimable_bytes 25,
 *   largest_reclaimable 25.
 * Laws: (1) with rep[rep[c]] == rep[c] <= c, all rows under one label and every
 * chunk taking part, delta / self / inherited equal sdcas_chunk_sharing's new /
 * self / other and stored_bytes its stored_bytes; (2) with family[i] = i,
 * inherited is 0 everywhere and there are no sets; (3) the sum of delta over a
 * label's rows is its stored.
 * SDCAS_E_INVALID for a needed NULL array (chunk_file, chunk_len, rep with m !=
 * 0; family with n_files != 0) or a misalignment (8 bytes for u64 and int64, 4
 * for u32); SDCAS_E_CAPACITY for m > 2^30 or n_files > 2^30: all before anything
 * is enqueued. m == 0 and n_files == 0 are SDCAS_OK; with m == 0 the rows still
 * form sets, with zero bytes, ordered by rep. Any output may be NULL. Results
 * are exact and do not depend on scheduling: the first occurrence of a class is
 * a property of the input, everything else is sums modulo 2^64, a minimum and
 * a maximum; two calls on one input give the same bytes. */
typedef struct sdcas_family_bytes_counts {
  uint64_t files;                 /* participating rows */
  uint64_t chunks;                /* participating chunks */
  uint64_t classes;               /* distinct (label, class number) pairs */
  uint64_t total_bytes;           /* over all participating rows */
  uint64_t stored_bytes;          /* over all participating rows */
  uint64_t sets;                  /* labels carried by at least two rows */
  uint64_t members;               /* rows in those sets */
  uint64_t set_reclaimable_bytes; /* the sum over the sets only */
  uint64_t largest_reclaimable;   /* the largest set's reclaimable bytes, 0 when there is none */
} sdcas_family_bytes_counts;
/* GPU-free: the range checks above (m, n_files) and *out_workspace_bytes = what
 * the device call takes (a table of at least 2 m u32 slots, 4 bytes per chunk,
 * 65 bytes per row and a little). The output may be NULL. */
int sdcas_family_bytes_plan(uint64_t m, uint64_t n_files, uint64_t *out_workspace_bytes);
/* Host arrays: one upload, the device call, the counts down, then exactly
 * `sets` entries of each set array. */
int sdcas_family_bytes(sdcas_ctx *ctx, const uint32_t *chunk_file, const uint64_t *chunk_len, const int64_t *rep,
                       size_t m, const int64_t *family, size_t n_files, uint64_t *out_file_bytes,
                       uint64_t *out_delta_bytes, uint64_t *out_self_bytes, uint64_t *out_inherited_bytes,
                       int64_t *out_set_rep, uint32_t *out_set_files, uint64_t *out_set_total,
                       uint64_t *out_set_stored, sdcas_family_bytes_counts *out_counts);
/* Device arrays under sdcas_dev_chunk_peers' stream rules. d_counts: nine u64 in
 * sdcas_family_bytes_counts' order, overwritten. The workspace for (m, n_files)
 * is allocated by the first call that needs it, which waits for the stream;
 * after that the call never waits for the device. Every grid is sized from m or
 * n_files, the numbers of classes and sets stay on the device, and the sets are
 * ordered by ceil_log2(n_files) merge launches, whatever the data. */
int sdcas_dev_family_bytes(sdcas_ctx *ctx, const uint32_t *d_chunk_file, const uint64_t *d_chunk_len,
                           const int64_t *d_rep, size_t m, const int64_t *d_family, size_t n_files,
                           uint64_t *d_file_bytes, uint64_t *d_delta_bytes, uint64_t *d_self_bytes,
                           uint64_t *d_inherited_bytes, int64_t *d_set_rep, uint32_t *d_set_files,
                           uint64_t *d_set_total, uint64_t *d_set_stored, uint64_t *d_counts, void *stream);

/* ---- family recipes: rebuild every file from its family's stored bytes ----------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * sdcas_family_bytes says that a family stores 22 of its 47 bytes. This call
 * says which: per row the list of byte ranges (OPS) that rebuilds the row from
 * what its family keeps. A literal op names bytes the row keeps itself; a copy
 * op names a range of another row (or an earlier range of the same row) that is
 * kept there. Neighbouring chunks that come from neighbouring bytes of one
 * source are one op. The library returns the plan; it reads and writes no file
 * bytes.
 *   inputs   sdcas_family_bytes' and one array: chunk_file[m] u32;
 *            chunk_off[m] u64, the chunk's offset IN ITS FILE (as the chunkers
 *            here report it); chunk_len[m] u64; rep[m] int64; family[n_files]
 *            int64. Which rows and chunks take part, the class (label, r(c)) and
 *            its first occurrence f(c) are sdcas_family_bytes', word for word.
 *            All arithmetic is modulo 2^64.
 *   source   for a participating chunk c, src(c) = (chunk_file[f(c)],
 *            chunk_off[f(c)]). c is a LITERAL when f(c) == c: the row keeps
 *            these bytes. Otherwise it is a COPY.
 *   continuation  a participating chunk c CONTINUES c - 1 when all of these hold:
 *              c >= 1 and c - 1 takes part;
 *              chunk_file[c - 1] == chunk_file[c];
 *              both are literals or both are copies;
 *              chunk_off[c] == chunk_off[c - 1] + chunk_len[c - 1];
 *              chunk_file[f(c)] == chunk_file[f(c - 1)];
 *              chunk_off[f(c)] == chunk_off[f(c - 1)] + chunk_len[c - 1].
 *            Any other participating chunk starts an op (is its HEAD). Only c - 1
 *            is looked at.
 *   ops      numbered in the order of their head chunks' positions:
 *              out_op_chunk[o]      u32  the head chunk
 *              out_op_src_chunk[o]  u32  f(head); the op is a literal if and only
 *                                        if this equals out_op_chunk[o]
 *              out_op_row[o]        u32  chunk_file[head]
 *              out_op_src_row[o]    u32  chunk_file[f(head)]
 *              out_op_dst_off[o]    u64  chunk_off[head]
 *              out_op_src_off[o]    u64  chunk_off[f(head)]
 *              out_op_len[o]        u64  the sum of its chunks' lengths
 *            The caller provides m entries for each op array; entries past `ops`
 *            are left as they were.
 *   per chunk  out_chunk_op[c] u32: the op of chunk c, 0xFFFFFFFF for a chunk that
 *            takes no part.
 *   per row  out_row_ops[i] u32: the number of the row's ops; out_row_first_op[i]
 *            u32: its lowest op, 0xFFFFFFFF when it has none. When a row's chunks
 *            are adjacent in the arrays, as every producer here writes them, its
 *            ops are [row_first_op, row_first_op + row_ops). When the chunks of
 *            two rows are interleaved the ops are still exact, but a row's ops
 *            are not adjacent: find them through out_op_row.
 * Example: two rows under one label, v1 = A B C and v2 = A B X C with lengths
 * 10, 20, 30 and X = 5:
 *     chunk_file [0,0,0,1,1,1,1]   chunk_off [0,10,30,0,10,30,35]
 *     chunk_len  [10,20,30,10,20,5,30]   rep [0,1,2,0,1,5,2]   family [0,0]
 *   Seven chunks give four ops:
 *     op 0  literal  row 0  dst 0   len 60
 *     op 1  copy     row 1  dst 0   from row 0 offset 0, len 30 (A and B merged)
 *     op 2  literal  row 1  dst 30  len 5
 *     op 3  copy     row 1  dst 35  from row 0 offset 30, len 30
 *   chunk_op [0,0,0,1,1,2,3]; row_ops [1,3]; row_first_op [0,1]. Counts: files 2,
 *   chunks 7, ops 4, literal_ops 2, copy_ops 2, literal_bytes 65, copy_bytes 60,
 *   longest_op 60.
 * Laws: (1) per row the sum of the literal ops' len is sdcas_family_bytes'
 * delta_bytes and the sum of the copy ops' is self_bytes + inherited_bytes;
 * literal_bytes is its stored_bytes. (2) For inputs whose chunk_off are the
 * running sums of chunk_len per file, every copy op's source range is covered
 * by literal ops of op_src_row: no copy reads from a copy, recipes have depth
 * one. (3) With such offsets, and rep equal only where the bytes are equal,
 * writing every op's source bytes at its dst_off rebuilds every participating
 * file, the source bytes taken from a store that holds the literal ops' bytes
 * and nothing else. (4) With family[i] = i every op's source lies in its own
 * row: op_src_row == op_row everywhere.
 * Errors and limits are sdcas_family_bytes', all before anything is enqueued:
 * SDCAS_E_INVALID for a needed NULL array (chunk_file, chunk_off, chunk_len, rep
 * with m != 0; family with n_files != 0) or a misalignment (8 bytes for u64 and
 * int64, 4 for u32); SDCAS_E_CAPACITY for m > 2^30 or n_files > 2^30. m == 0
 * and n_files == 0 are SDCAS_OK. Any output may be NULL, also all but the
 * counts. Results are exact and do not depend on scheduling; two calls on one
 * input give the same bytes. */
typedef struct sdcas_family_recipes_counts {
  uint64_t files;         /* participating rows */
  uint64_t chunks;        /* participating chunks */
  uint64_t ops;           /* literal_ops + copy_ops */
  uint64_t literal_ops;
  uint64_t copy_ops;
  uint64_t literal_bytes; /* the sum of the literal ops' len: what the families store */
  uint64_t copy_bytes;    /* the sum of the copy ops' len */
  uint64_t longest_op;    /* the largest op_len, 0 when there is no op */
} sdcas_family_recipes_counts;
/* GPU-free: the range checks above (m, n_files) and *out_workspace_bytes = what
 * the device call takes (a table of at least 2 m u32 slots, 17 bytes per chunk,
 * 8 bytes per row, 8 KiB of counters and a little). The output may be NULL. */
int sdcas_family_recipes_plan(uint64_t m, uint64_t n_files, uint64_t *out_workspace_bytes);
/* Host arrays: one upload, the device call, the counts down, then exactly `ops`
 * entries of each op array, with the m entries of chunk_op and the n_files of
 * the per-row arrays. */
int sdcas_family_recipes(sdcas_ctx *ctx, const uint32_t *chunk_file, const uint64_t *chunk_off,
                         const uint64_t *chunk_len, const int64_t *rep, size_t m, const int64_t *family,
                         size_t n_files, uint32_t *out_op_chunk, uint32_t *out_op_src_chunk, uint32_t *out_op_row,
                         uint32_t *out_op_src_row, uint64_t *out_op_dst_off, uint64_t *out_op_src_off,
                         uint64_t *out_op_len, uint32_t *out_chunk_op, uint32_t *out_row_ops,
                         uint32_t *out_row_first_op, sdcas_family_recipes_counts *out_counts);
/* Device arrays under sdcas_dev_chunk_peers' stream rules. d_counts: eight u64
 * in sdcas_family_recipes_counts' order, overwritten. The workspace for (m,
 * n_files) is allocated by the first call that needs it, which waits for the
 * stream; after that the call never waits for the device. Every grid is sized
 * from m or n_files and the number of ops stays on the device. */
int sdcas_dev_family_recipes(sdcas_ctx *ctx, const uint32_t *d_chunk_file, const uint64_t *d_chunk_off,
                             const uint64_t *d_chunk_len, const int64_t *d_rep, size_t m, const int64_t *d_family,
                             size_t n_files, uint32_t *d_op_chunk, uint32_t *d_op_src_chunk, uint32_t *d_op_row,
                             uint32_t *d_op_src_row, uint64_t *d_op_dst_off, uint64_t *d_op_src_off,
                             uint64_t *d_op_len, uint32_t *d_chunk_op, uint32_t *d_row_ops,
                             uint32_t *d_row_first_op, uint64_t *d_counts, void *stream);

/* ---- family store: pack the literal bytes and restore files from them ------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * The family recipes say which byte ranges rebuild every row. These calls move
 * the bytes: the literal ranges gathered into one dense STORE, every op pointed
 * at its place there, and any window of any row given back from the store alone.
 *
 * LAYOUT. Over the op arrays of sdcas_family_recipes, as they are, with its
 * chunk_op[m] and the number of ops (d_ops on the device: the recipes' d_counts
 * + 2; the calls use min(ops, max_ops)). All arithmetic is modulo 2^64.
 *   literal op o (op_chunk[o] == op_src_chunk[o]):
 *     store_off[o] = the sum of op_len over the literal ops below o. The store
 *     is dense; store_bytes is the sum over all literal ops (the recipes'
 *     literal_bytes).
 *   copy op o, with s = op_src_chunk[o] and L = chunk_op[s], is COVERED when
 *     s < m and L < ops; L is a literal op; op_row[L] == op_src_row[o];
 *     op_src_off[o] >= op_dst_off[L]; and with d = op_src_off[o] -
 *     op_dst_off[L]: d <= op_len[L] and op_len[o] <= op_len[L] - d.
 *     Then store_off[o] = store_off[L] + d. Otherwise store_off[o] is
 *     SDCAS_STORE_NONE and the op is counted in uncovered_ops and
 *     uncovered_bytes (so is a covered op whose offset comes out as 2^64 - 1).
 *   Entries of out_op_store_off at or past `ops` are left as they were.
 * Example, the recipes' v1 = A B C and v2 = A B X C: store_off [0, 0, 60, 30],
 * store_bytes 65, no op uncovered. For recipes whose chunk_off are the running
 * sums of chunk_len per file no op is uncovered: a copy's source chunk f is a
 * literal chunk, the op L = chunk_op[f] is the maximal run of literal chunks
 * around f, and the copy's chunks continue only while their sources continue
 * each other as literals of one row, which is the rule that keeps them in L.
 *
 * THE MOVER. Rows are described by three arrays over n_files:
 *   row_at[i]   u64  where the row's window starts in the blob
 *   row_base[i] u64  the file offset of the window's first byte (NULL: zeros)
 *   row_len[i]  u64  the bytes of the row present in the blob; 0: the row is absent
 * An op's range [dst_off, dst_off + len) is clipped to its row's window [base,
 * base + row_len), giving [lo, hi); only hi - lo bytes move. A corpus larger
 * than memory goes window by window against one layout, a file larger than a
 * window piece by piece; no state is carried between calls.
 *   pack     every literal op with a store offset: blob[row_at + (lo - base) ..]
 *            to store[store_off + (lo - dst_off) ..]
 *   restore  every op with a store offset: the other way. Window bytes that no
 *            op covers are left as they were.
 * An op that the call acts on is BAD, skipped whole and counted, when its row is
 * >= n_files; dst_off + len wraps; its store range [store_off, store_off + len)
 * is not inside the store (off <= cap && len <= cap - off, cap the call's
 * store_capacity or store_bytes); or its row is present and its window is not
 * inside the blob (row_at <= blob_bytes && row_len <= blob_bytes - row_at) or
 * base + row_len wraps. Arbitrary op arrays are therefore safe.
 * Memory contract:
 *   writes   exactly the destination bytes of the clipped ops, and no other byte
 *            of the store, the blob or the gaps between windows;
 *   reads    of blob and store only 16-byte aligned granules that hold at least
 *            one source byte;
 *   d_blob and d_store are 16-byte aligned and readable up to the next multiple
 *            of 16 past their byte counts;
 *   the windows of two rows that overlap in the blob, or two ops with a common
 *            destination byte, are the caller's: the result is unspecified in
 *            those bytes and never outside them.
 * Counts: ops_moved (ops with at least one byte in a window), bytes_moved,
 * bad_ops, tiles (the clipped ops cut into sdcas_family_store_tile_bytes()
 * destination bytes at 16-byte aligned destination addresses: a clipped op of n
 * bytes to address a has ceil((a % 16 + n) / tile) tiles).
 * Errors, all before anything is enqueued: SDCAS_E_INVALID for a needed NULL
 * pointer (the op arrays, the store offsets and d_ops with max_ops != 0;
 * chunk_op with m != 0; row_at and row_len with n_files != 0; the blob or the
 * store with a non-zero byte count) or a misalignment (16 bytes for blob and
 * store, 8 for u64, 4 for u32); SDCAS_E_CAPACITY for max_ops, m or n_files above
 * 2^30. Any count output may be NULL. Results are exact and do not depend on
 * scheduling. */
#define SDCAS_STORE_NONE UINT64_MAX
typedef struct sdcas_family_store_counts {
  uint64_t ops;             /* min(ops, max_ops) */
  uint64_t literal_ops;
  uint64_t copy_ops;
  uint64_t uncovered_ops;   /* copy ops without a store offset */
  uint64_t store_bytes;     /* the sum of the literal ops' len */
  uint64_t uncovered_bytes; /* the sum of the uncovered ops' len */
} sdcas_family_store_counts;
typedef struct sdcas_family_move_counts {
  uint64_t ops_moved;
  uint64_t bytes_moved;
  uint64_t bad_ops;
  uint64_t tiles;
} sdcas_family_move_counts;
/* GPU-free: the mover's tile in destination bytes, a positive multiple of 16. */
uint64_t sdcas_family_store_tile_bytes(void);
/* GPU-free: the range checks (max_ops, n_files) and *out_workspace_bytes = what
 * the three device calls share (32 bytes per op, 8 KiB of counters and a
 * little). The output may be NULL. */
int sdcas_family_store_plan(uint64_t max_ops, uint64_t n_files, uint64_t *out_workspace_bytes);
/* Device arrays under sdcas_dev_chunk_peers' stream rules. d_counts: six u64 in
 * sdcas_family_store_counts' order, overwritten; d_op_store_off may be NULL.
 * The workspace for max_ops is allocated by the first of the three calls that
 * needs it, which waits for the stream; after that no call waits for the
 * device. Every grid is sized from max_ops or a constant. */
int sdcas_dev_family_store_layout(sdcas_ctx *ctx, const uint32_t *d_op_chunk, const uint32_t *d_op_src_chunk,
                                  const uint32_t *d_op_row, const uint32_t *d_op_src_row,
                                  const uint64_t *d_op_dst_off, const uint64_t *d_op_src_off,
                                  const uint64_t *d_op_len, const uint32_t *d_chunk_op, size_t m,
                                  const uint64_t *d_ops, size_t max_ops, uint64_t *d_op_store_off,
                                  uint64_t *d_counts, void *stream);
/* d_counts: four u64 in sdcas_family_move_counts' order, overwritten. */
int sdcas_dev_family_pack(sdcas_ctx *ctx, const uint32_t *d_op_chunk, const uint32_t *d_op_src_chunk,
                          const uint32_t *d_op_row, const uint64_t *d_op_dst_off, const uint64_t *d_op_len,
                          const uint64_t *d_op_store_off, const uint64_t *d_ops, size_t max_ops,
                          const uint64_t *d_row_at, const uint64_t *d_row_base, const uint64_t *d_row_len,
                          size_t n_files, const uint8_t *d_blob, uint64_t blob_bytes, uint8_t *d_store,
                          uint64_t store_capacity, uint64_t *d_counts, void *stream);
int sdcas_dev_family_restore(sdcas_ctx *ctx, const uint32_t *d_op_row, const uint64_t *d_op_dst_off,
                             const uint64_t *d_op_len, const uint64_t *d_op_store_off, const uint64_t *d_ops,
                             size_t max_ops, const uint64_t *d_row_at, const uint64_t *d_row_base,
                             const uint64_t *d_row_len, size_t n_files, const uint8_t *d_store,
                             uint64_t store_bytes, uint8_t *d_blob, uint64_t blob_bytes, uint64_t *d_counts,
                             void *stream);
/* Host arrays: one upload, the device call, one download. `ops` entries of
 * every op array. pack's store and restore's blob go up and come down again, so
 * the bytes the call does not write stay as the caller had them. */
int sdcas_family_store_layout(sdcas_ctx *ctx, const uint32_t *op_chunk, const uint32_t *op_src_chunk,
                              const uint32_t *op_row, const uint32_t *op_src_row, const uint64_t *op_dst_off,
                              const uint64_t *op_src_off, const uint64_t *op_len, size_t ops,
                              const uint32_t *chunk_op, size_t m, uint64_t *out_op_store_off,
                              sdcas_family_store_counts *out_counts);
int sdcas_family_pack(sdcas_ctx *ctx, const uint32_t *op_chunk, const uint32_t *op_src_chunk,
                      const uint32_t *op_row, const uint64_t *op_dst_off, const uint64_t *op_len,
                      const uint64_t *op_store_off, size_t ops, const uint64_t *row_at, const uint64_t *row_base,
                      const uint64_t *row_len, size_t n_files, const uint8_t *blob, uint64_t blob_bytes,
                      uint8_t *store, uint64_t store_capacity, sdcas_family_move_counts *out_counts);
int sdcas_family_restore(sdcas_ctx *ctx, const uint32_t *op_row, const uint64_t *op_dst_off,
                         const uint64_t *op_len, const uint64_t *op_store_off, size_t ops, const uint64_t *row_at,
                         const uint64_t *row_base, const uint64_t *row_len, size_t n_files, const uint8_t *store,
                         uint64_t store_bytes, uint8_t *blob, uint64_t blob_bytes,
                         sdcas_family_move_counts *out_counts);

/* ---- family store: forget rows ------------------------------------------------------
 *
 * Added after ABI 7; probe for the symbol (SDCAS_ABI_VERSION stays 7).
 *
 * A packed store is frozen: once a stored file is deleted, the only way to a
 * store without it was to read every original again. These two calls take rows
 * out of a store with no file read. Recipes are defined per chunk, so removal is
 * done on the chunk arrays: KEEP drops the chunks of the removed rows and
 * elects classes and labels again among the survivors; sdcas_dev_family_recipes
 * and sdcas_dev_family_store_layout run over what it leaves, unchanged; MOVES
 * says where every literal byte of the new store lies in the old one, and the
 * mover above (sdcas_dev_family_restore, one row, one window over the new store,
 * the moves as its ops) carries the bytes. The result equals the store built
 * from the surviving files alone. All arithmetic is modulo 2^64.
 *
 * KEEP. Inputs: chunk_file[m] u32, chunk_off[m] u64, chunk_len[m] u64, rep[m]
 * int64; family[n_files] int64; keep[n_files] u8, nonzero means the row stays.
 *   rows     row i is kept when keep[i] != 0. out_row_new[i] (u32, n_files
 *            entries) is the number of kept rows below i, or 0xFFFFFFFF for a
 *            removed row. out_row_from[j] (u32, n' entries, ascending) is the
 *            inverse.
 *   labels   a kept row takes part when 0 <= family[i] < n_files, which is
 *            sdcas_family_bytes' rule. out_family[j] (int64) is the new number
 *            of the lowest kept row that takes part with the same label value;
 *            -1 for a kept row that takes no part.
 *   chunks   chunk c survives when chunk_file[c] < n_files and that row is kept.
 *            Its new position is the number of surviving chunks below it.
 *            out_chunk_from[c'] (u32) is the old position; out_chunk_file[c'] =
 *            row_new[chunk_file[c]]; out_chunk_off and out_chunk_len are copied.
 *   classes  r(c) = rep[c] when 0 <= rep[c] <= c, else c: sdcas_family_bytes'
 *            class number. out_rep[c'] (int64) is the new position of the lowest
 *            surviving chunk with the same r.
 *   counts   on the device as the others are: rows_kept (n'), rows_removed,
 *            chunks_kept (m'), chunks_removed, bytes_kept, bytes_removed (the sums
 *            of chunk_len over the surviving and the other chunks).
 * The caller provides n_files entries for each row array and m for each chunk
 * array; entries of the outputs past n' or m' are left as they were. Any output
 * may be NULL.
 * Laws: (1) out_rep[out_rep[c']] == out_rep[c'] <= c'. (2) Two surviving chunks
 * have equal out_rep if and only if they have equal r. (3) Two kept
 * participating rows have equal out_family if and only if they had equal
 * labels. (4) keep(A) followed by keep(B) over its outputs equals one keep of
 * the rows that both keep. (5) For a rep that was sdcas_confirm_duplicates' over
 * all chunks, out_rep is what confirm gives over the surviving chunks alone.
 *
 * MOVES. Old side: chunk_off[m], chunk_op[m], op_dst_off[k], op_store_off[k] and
 * the number of ops (d_ops, max_ops as in the layout). New side: chunk_from[m'],
 * chunk_off'[m'], chunk_len'[m'], chunk_op'[m'] and the new ops' op_chunk',
 * op_src_chunk', op_dst_off', op_store_off' with d_ops', max_ops'. d_chunks':
 * m' as a device u64, which is keep's d_counts + 2; the call uses min(m',
 * max_chunks). For a new chunk c':
 *   old_at   let c = chunk_from[c'] and o = chunk_op[c]. old_at(c') =
 *            op_store_off[o] + (chunk_off[c] - op_dst_off[o]). This holds for a
 *            literal and for a covered copy alike, since a copy op's store
 *            offset is its source's place. old_at(c') is NONE when c >= m; o is
 *            0xFFFFFFFF or o >= ops; op_store_off[o] is SDCAS_STORE_NONE; or
 *            chunk_off[c] < op_dst_off[o] (so is a place that comes out as
 *            2^64 - 1).
 *   literal  let o' = chunk_op'[c']. c' is a literal chunk when o' < ops' and
 *            op_chunk'[o'] == op_src_chunk'[o']. Then new_at(c') =
 *            op_store_off'[o'] + (chunk_off'[c'] - op_dst_off'[o']).
 *   heads    a literal chunk with an old_at CONTINUES c' - 1 when both are
 *            literal chunks of one new op, c' - 1 has an old_at, and old_at(c')
 *            == old_at(c' - 1) + chunk_len'[c' - 1]. Only c' - 1 is looked at.
 *            Any other such chunk is a HEAD.
 *   moves    numbered in the order of their heads: out_move_dst[j] =
 *            new_at(head), out_move_src[j] = old_at(head), out_move_len[j] the
 *            sum of its chunks' lengths (u64 each). The caller gives m' entries
 *            (max_chunks on the device); those past `moves` are left as they were.
 *   lost     a literal chunk whose old_at is NONE gets no move and is counted.
 * Example, the recipes' v1 = A B C and v2 = A B X C with v1 removed: the old
 * store is A B C X with offsets [0, 0, 60, 30]; the new recipes are one literal
 * op of 65 bytes; old_at of A, B, X, C is 0, 10, 60, 30. Three moves (dst, src,
 * len): (0, 0, 30), (30, 60, 5), (35, 30, 30). Counts: moves 3, literal_chunks
 * 4, moved_bytes 65, lost 0, longest_move 30.
 * Laws: for stores of recipes under the recipes' law 2 (running-sum offsets)
 * nothing is lost: a literal chunk of the new recipes took part before, so its
 * old op has a place, and a copy's place is its source's. The moves'
 * destinations are disjoint and cover [0, store_bytes'). store_bytes' <=
 * store_bytes, so a new store never needs more room than the old one.
 * The bytes: sdcas_dev_family_restore with op_row all 0, op_dst_off =
 * move_dst, op_len = move_len, op_store_off = move_src, d_ops = moves' d_counts,
 * n_files = 1, row_at [0], row_len [store_bytes'], the old store as d_store and
 * the new one as d_blob, out of place. The mover's memory contract and its
 * bad-op rule hold for moves as they are.
 * Errors, all before anything is enqueued: SDCAS_E_INVALID for a needed NULL
 * (keep: chunk_file, chunk_off, chunk_len, rep with m != 0; family, keep with
 * n_files != 0. moves: chunk_off, chunk_op with m != 0; op_dst_off,
 * op_store_off, d_ops with max_ops != 0; the new chunk arrays and d_chunks' with
 * max_chunks != 0; the new op arrays and d_ops' with max_ops' != 0) or a
 * misalignment (8 bytes for u64 and int64, 4 for u32); SDCAS_E_CAPACITY for m,
 * n_files, max_ops, max_ops' or max_chunks above 2^30. m == 0 and n_files == 0
 * are SDCAS_OK. Results are exact and do not depend on scheduling; two calls on
 * one input give the same bytes. */
typedef struct sdcas_family_keep_counts {
  uint64_t rows_kept;
  uint64_t rows_removed;
  uint64_t chunks_kept;
  uint64_t chunks_removed;
  uint64_t bytes_kept;
  uint64_t bytes_removed;
} sdcas_family_keep_counts;
typedef struct sdcas_family_moves_counts {
  uint64_t moves;
  uint64_t literal_chunks; /* literal chunks of the new recipes, the lost among them */
  uint64_t moved_bytes;    /* the sum of the moves' len */
  uint64_t lost_chunks;
  uint64_t lost_bytes;
  uint64_t longest_move;   /* the largest move_len, 0 when there is no move */
} sdcas_family_moves_counts;
/* GPU-free: the range checks (m, n_files) and *out_workspace_bytes = what the two
 * device calls share for m chunks of n_files rows (17 bytes per chunk, 8 per
 * row, 8 KiB of counters and a little). The output may be NULL. */
int sdcas_family_forget_plan(uint64_t m, uint64_t n_files, uint64_t *out_workspace_bytes);
/* Host arrays: one upload, the device call, the counts down, then exactly n'
 * entries of row_from and family, m' of the chunk arrays and n_files of row_new. */
int sdcas_family_chunks_keep(sdcas_ctx *ctx, const uint32_t *chunk_file, const uint64_t *chunk_off,
                             const uint64_t *chunk_len, const int64_t *rep, size_t m, const int64_t *family,
                             const uint8_t *keep, size_t n_files, uint32_t *out_row_new, uint32_t *out_row_from,
                             int64_t *out_family, uint32_t *out_chunk_from, uint32_t *out_chunk_file,
                             uint64_t *out_chunk_off, uint64_t *out_chunk_len, int64_t *out_rep,
                             sdcas_family_keep_counts *out_counts);
/* Device arrays under sdcas_dev_chunk_peers' stream rules. d_counts: six u64 in
 * sdcas_family_keep_counts' order, overwritten. The workspace is allocated by
 * the first of the two calls that needs it, which waits for the stream; after
 * that no call waits for the device. Every grid is sized from m or n_files. */
int sdcas_dev_family_chunks_keep(sdcas_ctx *ctx, const uint32_t *d_chunk_file, const uint64_t *d_chunk_off,
                                 const uint64_t *d_chunk_len, const int64_t *d_rep, size_t m,
                                 const int64_t *d_family, const uint8_t *d_keep, size_t n_files,
                                 uint32_t *d_row_new, uint32_t *d_row_from, int64_t *d_family_out,
                                 uint32_t *d_chunk_from, uint32_t *d_chunk_file_out, uint64_t *d_chunk_off_out,
                                 uint64_t *d_chunk_len_out, int64_t *d_rep_out, uint64_t *d_counts, void *stream);
/* Host arrays: one upload, the device call, the counts down, then exactly
 * `moves` entries of each move array. */
int sdcas_family_store_moves(sdcas_ctx *ctx, const uint64_t *chunk_off, const uint32_t *chunk_op, size_t m,
                             const uint64_t *op_dst_off, const uint64_t *op_store_off, size_t ops,
                             const uint32_t *new_chunk_from, const uint64_t *new_chunk_off,
                             const uint64_t *new_chunk_len, const uint32_t *new_chunk_op, size_t new_chunks,
                             const uint32_t *new_op_chunk, const uint32_t *new_op_src_chunk,
                             const uint64_t *new_op_dst_off, const uint64_t *new_op_store_off, size_t new_ops,
                             uint64_t *out_move_dst, uint64_t *out_move_src, uint64_t *out_move_len,
                             sdcas_family_moves_counts *out_counts);
/* d_counts: six u64 in sdcas_family_moves_counts' order, overwritten. Every grid
 * is sized from max_chunks; the number of moves stays on the device. */
int sdcas_dev_family_store_moves(sdcas_ctx *ctx, const uint64_t *d_chunk_off, const uint32_t *d_chunk_op, size_t m,
                                 const uint64_t *d_op_dst_off, const uint64_t *d_op_store_off,
                                 const uint64_t *d_ops, size_t max_ops, const uint32_t *d_new_chunk_from,
                                 const uint64_t *d_new_chunk_off, const uint64_t *d_new_chunk_len,
                                 const uint32_t *d_new_chunk_op, const uint64_t *d_new_chunks, size_t max_chunks,
                                 const uint32_t *d_new_op_chunk, const uint32_t *d_new_op_src_chunk,
                                 const uint64_t *d_new_op_dst_off, const uint64_t *d_new_op_store_off,
                                 const uint64_t *d_new_ops, size_t max_new_ops, uint64_t *d_move_dst,
                                 uint64_t *d_move_src, uint64_t *d_move_len, uint64_t *d_counts, void *stream);

/* ---- multi-GPU dedup stages (one process per GPU) -------
 *
 * sdcas_dedup's group-by split at its one exchange step, for a node whose
 * orphan file_paths (and existing Objects) are sharded over ranks. The host
 * runs, on every rank, with its own communicator (RCCL all-to-all over xGMI;
 * spacedrive_amd/dist_dedup.py is the reference driver):
 *   0. stays(files)      -> this rank's stays ordinals; all-gather them and
 *      plan                 build the job's step plan (the same on every rank)
 *   1. combine(files)    -> records grouped by owner rank + per-file slot
 *      combine(existing) -> records grouped by owner rank (ids = DB order)
 *   2. all-to-all both record sets (counts from out_starts)
 *   3. resolve on the received records -> one int64 answer per file record
 *   4. all-to-all the answers back (the reverse of step 2's file exchange)
 *   5. apply -> out_link / counts with sdcas_dedup's encoding, except that
 *      every file index is the GLOBAL orphan ordinal d_ids[i].
 * All pointers except out_starts are device pointers; calls are enqueued on
 * `stream` (NULL = the context's); combine synchronises once to return
 * out_starts. The owner of a key is its top 12 bits (the 3-hex thumbnail
 * shard prefix) split into `world` equal ranges.
 *
 * stays: the ordinals of this rank's files that stay orphans after their
 *   step (d_status != 0 or d_has_key == 0; both may be NULL) -> d_stays[cap],
 *   ascending, padded with UINT64_MAX; *d_count (device int64) = all of them,
 *   also when more than cap (then gather them again with a larger cap).
 * plan: d_stays = every rank's stays lists (n_stays entries in any order,
 *   UINT64_MAX entries ignored); the job's orphans are ordinals [0, n_total);
 *   max_steps / more as in sdcas_job_window -> d_plan (device u64,
 *   SDCAS_PLAN_WORDS(n_stays)): word 2 the steps run, 3 rows and 8 rereads
 *   (as in sdcas_job_window); the rest is the plan's own (dist_dedup.h).
 *   Word 9 stamps the building context's coarse index of the plan's re-read
 *   list (64 or more re-reads; 0: none): an apply on that context uses it
 *   until the context builds another plan, any other apply searches the
 *   whole list — the links are the same either way.
 * combine: d_ids[n] ascending; d_has_key / d_status may be NULL (all
 *   present / all ok). Writes exactly one record d_rec[2*u], d_rec[2*u+1] =
 *   (cas key, min id over the files carrying it) per distinct key (capacity
 *   2*n u64), grouped by owner: owner r's records are d_rec's records
 *   [out_starts[r], out_starts[r+1]), in NO particular order inside that
 *   range (ABI 5; ABI 4 and earlier documented ascending top-32-bit order and
 *   possibly several records per key — do not binary-search or merge the
 *   ranges); d_slot[i] = record of file i (0xFFFFFFFF no cas_id, 0xFFFFFFFE
 *   dropped; may be NULL), and out_starts[0..world] (host) = first record of
 *   each owner; out_starts[world] is the record count.
 * resolve: d_result[p] for received file record p = -(db+1) if existing
 *   Object db carries the key (the first in DB order), else the lowest orphan
 *   ordinal carrying it on any rank.
 * apply: d_result indexed by this rank's records (in send order); d_plan from
 *   plan (NULL: no file of the job stays an orphan and its steps read every
 *   row); d_counts (2 x u64, zeroed by the caller) += (created, linked). */
#define SDCAS_PLAN_HEADER_WORDS 12
#define SDCAS_PLAN_WORDS(n_stays) (SDCAS_PLAN_HEADER_WORDS + (n_stays))
int sdcas_dev_dedup_stays(sdcas_ctx *ctx, const uint8_t *d_has_key, const int32_t *d_status, const uint64_t *d_ids,
                          size_t n, size_t cap, uint64_t *d_stays, int64_t *d_count, void *stream);
int sdcas_dev_dedup_plan(sdcas_ctx *ctx, const uint64_t *d_stays, size_t n_stays, uint64_t n_total,
                         size_t chunk_size, uint64_t max_steps, uint32_t more, uint64_t *d_plan, void *stream);
int sdcas_dev_dedup_combine(sdcas_ctx *ctx, const uint64_t *d_keys, const uint8_t *d_has_key,
                            const int32_t *d_status, const uint64_t *d_ids, size_t n, uint32_t world,
                            uint64_t *d_rec, uint32_t *d_slot, uint64_t *out_starts, void *stream);
/* combine without the host synchronisation: the owner ranges go to
 * d_starts[0..world] (device u32) instead of out_starts, so that a caller
 * driving several GPUs enqueues every GPU's combine before it reads any
 * (sdcas_node_dedup_window) */
int sdcas_dev_dedup_combine_async(sdcas_ctx *ctx, const uint64_t *d_keys, const uint8_t *d_has_key,
                                  const int32_t *d_status, const uint64_t *d_ids, size_t n, uint32_t world,
                                  uint64_t *d_rec, uint32_t *d_slot, uint32_t *d_starts, void *stream);
int sdcas_dev_dedup_resolve(sdcas_ctx *ctx, const uint64_t *d_frec, size_t nf, const uint64_t *d_erec,
                            size_t ne, int64_t *d_result, void *stream);
int sdcas_dev_dedup_apply(sdcas_ctx *ctx, const uint64_t *d_ids, const uint32_t *d_slot, size_t n,
                          const int64_t *d_result, size_t chunk_size, const uint64_t *d_plan, int64_t *d_link,
                          uint64_t *d_counts, void *stream);
/* The same two stages without any host synchronisation, for RCCL's
 * all-to-all with equal splits (spacedrive_amd/dist_dedup.py): the combine
 * writes owner r's records to bucket r of d_send (world x cap records of 16 B,
 * record p of bucket r at d_send[2 * (r * cap + p)]), d_counts[r] (device
 * int64) = its valid records, d_slot[i] = the bucket position r * cap + p of
 * file i, and sets *d_overflow (device u32) to 1 when some owner has
 * more than cap records (the buckets are then unusable: rerun the exact
 * stages). The bucket combine may send several records of one key (one per
 * key per 2048-file tile of the rank, each with the tile's lowest ordinal);
 * the owner's minimum covers them. resolve_buckets answers the received
 * buckets (world x fcap file records, world x ecap existing records, the
 * first d_fcounts[r] / d_ecounts[r] of bucket r valid) into
 * d_result[world * fcap], bucket layout, and uses the received buckets as
 * scratch: the value word of valid records may be overwritten (each key's
 * claiming record takes the key's minimum). apply then reads the answers
 * returned in the same layout. */
int sdcas_dev_dedup_combine_buckets(sdcas_ctx *ctx, const uint64_t *d_keys, const uint8_t *d_has_key,
                                    const int32_t *d_status, const uint64_t *d_ids, size_t n, uint32_t world,
                                    size_t cap, uint64_t *d_send, uint32_t *d_slot, int64_t *d_counts,
                                    uint32_t *d_overflow, void *stream);
int sdcas_dev_dedup_resolve_buckets(sdcas_ctx *ctx, const uint64_t *d_frec, size_t fcap, const int64_t *d_fcounts,
                                    const uint64_t *d_erec, size_t ecap, const int64_t *d_ecounts, uint32_t world,
                                    int64_t *d_result, void *stream);
/* A world of one: the stages without the combine (nothing is exchanged, so
 * files and existing Objects go straight into resolve's table, and the plan
 * comes from this call's own stays rows): the same d_link / d_counts as
 * stays -> plan -> combine -> resolve -> apply. d_ekeys/d_eids [ne]: existing
 * Objects' cas keys and DB indices (may be NULL when ne == 0). d_ids lie in
 * [0, n_total) (n_total 0: n); max_steps / more as in sdcas_job_window.
 * d_plan_header (may be NULL) receives the plan's SDCAS_PLAN_HEADER_WORDS. */
int sdcas_dev_dedup_local(sdcas_ctx *ctx, const uint64_t *d_keys, const uint8_t *d_has_key,
                          const int32_t *d_status, const uint64_t *d_ids, size_t n, const uint64_t *d_ekeys,
                          const uint64_t *d_eids, size_t ne, size_t chunk_size, uint64_t n_total,
                          uint64_t max_steps, uint32_t more, int64_t *d_link, uint64_t *d_counts,
                          uint64_t *d_plan_header, void *stream);

/* ---- one process, several GPUs (a node) ----------------------------------
 *
 * sd-core is one process (Node::new, apps/server/src/main.rs:40; jobs run
 * in-process, job/manager.rs:32). A node is one context per entry of
 * `devices` (a device may repeat: two contexts on one GPU), with the batch
 * calls sharded over them and the dedup's exchange run in this process as
 * device-to-device copies (hipMemcpyPeerAsync; over xGMI between distinct
 * GPUs), or over RCCL (ncclCommInitAll, grouped ncclSend / ncclRecv) when every
 * device is distinct and the environment sets SDCAS_NODE_EXCHANGE=rccl (opt-in
 * until measured on a multi-GPU box). Results are those of the single-context
 * calls. opts (may be NULL) applies to every context; its progress function
 * receives the node's sums and may run on any of the node's threads (one at a
 * time). Calls on one node serialise. */
typedef struct sdcas_node sdcas_node;
int sdcas_node_init(const int32_t *devices, size_t n_devices, const sdcas_options *opts, sdcas_node **out_node);
void sdcas_node_destroy(sdcas_node *node);
const char *sdcas_node_last_error(const sdcas_node *node);
size_t sdcas_node_size(const sdcas_node *node);
/* 1 when the dedup exchange runs over RCCL, 0 over device copies */
int sdcas_node_uses_rccl(const sdcas_node *node);
int sdcas_node_set_progress(sdcas_node *node, sdcas_progress_fn progress, void *user, const volatile int32_t *cancel);
/* sdcas_cas_ids with the files cut into contiguous ranges of about equal
 * cas-message bytes, one per context */
int sdcas_node_cas_ids(sdcas_node *node, const char *const *paths, const uint64_t *sizes, size_t n,
                       uint64_t *out_keys, int32_t *out_status);
/* sdcas_checksums with the files assigned largest first to the least loaded context */
int sdcas_node_checksums(sdcas_node *node, const char *const *paths, size_t n, uint8_t *out32, int32_t *out_status);
/* sdcas_dedup_window over the node: contiguous ordinal ranges per context,
 * stays all-gathered and planned on every context, records exchanged to the
 * key's owner context (top 12 key bits), resolved there, answers returned */
int sdcas_node_dedup_window(sdcas_node *node, const uint64_t *keys, const uint8_t *has_key, const int32_t *status,
                            size_t n, size_t chunk_size, const uint64_t *existing_keys, size_t n_existing,
                            sdcas_job_window *window, int64_t *out_link, int64_t *out_created, int64_t *out_linked);

/* ---- helpers ------------------------------------------------------------ */

void sdcas_key_to_hex(uint64_t key, char out[17]);
void sdcas_digest_to_hex(const uint8_t digest[32], char out[65]);
uint64_t sdcas_cas_message_len(uint64_t size);

#ifdef __cplusplus
}
#endif
#endif /* SDCAS_H */
