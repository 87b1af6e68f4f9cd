// sdcore.hpp — C++ host mirror of sd-core's content-identification path,
// layered on the C ABI of libsdcas.so (include/sdcas.h).
//
// The reference host is Rust (sd-core); there is no Rust toolchain in this
// image, so the host side above the C ABI is written in C++ with the
// reference's names, argument meaning and error behaviour:
//
//   generate_cas_id / generate_cas_ids   core/src/object/cas.rs:23-62
//   file_checksum / file_checksums       core/src/object/validation/hash.rs:9-25
//   FileMetadata::new (batched)          core/src/object/file_identifier/mod.rs:48-96
//   identifier_job_step                  core/src/object/file_identifier/mod.rs:98-350
//   run_file_identifier_job              core/src/object/file_identifier/file_identifier_job.rs:33-319
//   run_object_validator_job             core/src/object/validation/validator_job.rs:38-200
//
// The database side (prisma in sd-core) is the abstract `Library`; a
// `MemoryLibrary` implements it over in-memory tables with the reference's
// query semantics (filters, DB order, cursor) for tests and examples.
//
// Hashing runs on the GPU through libsdcas. There is no CPU fallback in this
// layer: when the engine cannot open (no device) `Engine::open` throws
// `LibraryError`, which is the point where the Rust host keeps its own CPU
// path (include/sdcas.h, "Conventions").
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sdcas.h"

namespace sdcore {

// std::io::Error as the Rust host sees it (crates/utils/src/error.rs:5-22
// FileIOError = path + io::Error): an errno, or UnexpectedEof from read_exact
// (cas.rs:36,43,56), which has no errno.
struct IoError {
  int code = 0;
  std::string path;
  bool unexpected_eof() const { return code == SDCAS_STATUS_UNEXPECTED_EOF; }
  std::string message() const;
};

// io::Result<T>
template <class T>
class Result {
 public:
  Result(T v) : v_(std::move(v)) {}
  Result(IoError e) : e_(std::move(e)) {}
  bool ok() const { return v_.has_value(); }
  const T& value() const {
    if (!v_) throw std::logic_error("Result::value on an error: " + e_.message());
    return *v_;
  }
  const IoError& error() const { return e_; }

 private:
  std::optional<T> v_;
  IoError e_;
};

// A library failure (negative SDCAS_E_* return): the whole batch must take the
// host's CPU path.
class LibraryError : public std::runtime_error {
 public:
  LibraryError(int code, const std::string& what) : std::runtime_error(what), code(code) {}
  int code;
};

// A chunk index on the host (include/sdcas.h "chunk index"): the entries
// strictly ascending in (key, digest as 32 bytes), digests 32 bytes per entry,
// values the file_path id of the row that held the chunk first, and the
// directory of 2^bits + 1 slots.
struct ChunkIndexData {
  std::vector<uint64_t> keys, values;
  std::vector<uint8_t> digests;
  std::vector<uint32_t> dir{0, 0};
  uint32_t bits = 0;
  size_t size() const { return keys.size(); }
};

class Engine {
 public:
  struct Options {
    int device = -1;             // HIP device ordinal, -1: current
    uint32_t io_threads = 0;     // reader threads (0: library default)
    uint64_t staging_bytes = 0;  // pinned staging per slot (0: library default)
    uint32_t flags = 0;          // SDCAS_OPT_* (SDCAS_OPT_DIRECT_IO: big-file checksums bypass the page cache)
    // progress / cancellation of the batch calls (sdcas.h "Conventions"): the
    // job's progress hook (job/worker.rs:458-480) and its cancel command
    // (job/mod.rs:862-960)
    sdcas_progress_fn progress = nullptr;
    void* progress_user = nullptr;
    const volatile int32_t* cancel = nullptr;
  };
  static std::unique_ptr<Engine> open(const Options& opts);
  static std::unique_ptr<Engine> open() { return open(Options{}); }
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  // cas.rs:23-62 over a batch: (path, size from fs::metadata) -> 16 lowercase hex
  std::vector<Result<std::string>> generate_cas_ids(const std::vector<std::pair<std::string, uint64_t>>& files);
  // hash.rs:11-25 over a batch: path -> 64 lowercase hex
  std::vector<Result<std::string>> file_checksums(const std::vector<std::string>& paths);
  // fs::metadata + generate_cas_id of FileMetadata::new (mod.rs:48-96) in one
  // call (sdcas_file_metadata: the length from fstat of the descriptor the
  // reads use)
  struct RawMetadata {
    std::vector<uint64_t> size, key;
    std::vector<int32_t> status;
    std::vector<uint8_t> flags;  // SDCAS_META_*
    std::vector<uint8_t> digest;  // identify_checksums only: 32 bytes per file
  };
  RawMetadata file_metadata(const std::vector<const char*>& paths, const uint64_t* size_hints = nullptr);
  // the same and file_checksum from one open and one read of each file
  // (sdcas_identify_checksums): digest holds 32 bytes per file, valid where
  // flags has SDCAS_META_HAS_CHECKSUM
  RawMetadata identify_checksums(const std::vector<const char*>& paths, const uint64_t* size_hints = nullptr);

  // the canonical group-by of mod.rs:149-254 over the job's steps
  // (sdcas_dedup_window; sdcas_dedup encoding of out_link). window may be
  // null: the whole job over these rows.
  struct Dedup {
    std::vector<int64_t> link;
    int64_t created = 0, linked = 0;
  };
  Dedup dedup(const std::vector<uint64_t>& keys, const std::vector<uint8_t>& has_key,
              const std::vector<int32_t>& status, size_t chunk_size, const std::vector<uint64_t>& existing_keys,
              sdcas_job_window* window = nullptr);

  // the group-by over (cas key, 32-byte checksum) (sdcas_confirm_duplicates):
  // digests holds 32 bytes per key; valid may be empty (all files take part)
  struct Confirm {
    std::vector<int64_t> rep, key_rep;
    std::vector<uint8_t> flags;  // SDCAS_CONFIRM_*
    sdcas_confirm_counts counts{};
  };
  Confirm confirm_duplicates(const std::vector<uint64_t>& keys, const std::vector<uint8_t>& digests,
                             const std::vector<uint8_t>& valid);

  // the files grouped by the value rep[i] into sets of two or more
  // (sdcas_duplicate_sets), trimmed to the counts: set s is
  // members[set_offsets[s] .. set_offsets[s + 1]), ascending. sizes may be
  // empty (set_bytes are 0; not with SDCAS_SETS_BY_RECLAIMABLE)
  struct Sets {
    std::vector<int64_t> set_rep, members;
    std::vector<uint64_t> set_offsets, set_bytes;
    sdcas_sets_counts counts{};
  };
  Sets duplicate_sets(const std::vector<int64_t>& rep, const std::vector<uint64_t>& sizes,
                      uint32_t order = SDCAS_SETS_BY_REP);

  // BLAKE3 of each string (sdcas_hash_messages): 32 bytes per string, the
  // name digests the tree calls take
  std::vector<uint8_t> hash_strings(const std::vector<std::string>& strings);

  // a digest per directory (sdcas_tree_digests): keys / digests / valid hold
  // the FILE entries' values and come back with the directory entries' slots
  // filled; sizes may be empty (every tree_bytes is 0)
  struct TreeDigests {
    std::vector<uint64_t> keys, tree_bytes, tree_files;
    std::vector<uint8_t> digests, valid, flags;  // flags: SDCAS_TREE_*
    sdcas_tree_counts counts{};
  };
  TreeDigests tree_digests(const std::vector<int64_t>& parent, const std::vector<uint8_t>& is_dir,
                           const std::vector<uint8_t>& name32, const std::vector<uint64_t>& sizes,
                           const std::vector<uint64_t>& keys, const std::vector<uint8_t>& digests,
                           const std::vector<uint8_t>& valid);
  // the top-most duplicates (sdcas_tree_top) of a label per entry
  struct TreeTop {
    std::vector<int64_t> top_rep;
    std::vector<uint8_t> flags;  // SDCAS_TOP_*
    sdcas_top_counts counts{};
  };
  TreeTop tree_top(const std::vector<int64_t>& parent, const std::vector<int64_t>& rep);

  // the files blob[offsets[i] .. offsets[i] + lens[i]) cut into content-defined
  // chunks (sdcas_chunk_messages), every per-chunk array trimmed to the
  // counts: file i's chunks are [file_chunks[i], file_chunks[i + 1]);
  // chunk_off are offsets in the blob; digests holds 32 bytes per chunk.
  // params null: SDCAS_CHUNK_PARAMS_DEFAULT
  struct Chunks {
    std::vector<uint64_t> file_chunks, chunk_off, chunk_len, keys;
    std::vector<uint32_t> chunk_file;
    std::vector<uint8_t> digests;
    sdcas_chunk_counts counts{};
  };
  Chunks chunk_messages(const std::vector<uint8_t>& blob, const std::vector<uint64_t>& offsets,
                        const std::vector<uint64_t>& lens, const sdcas_chunk_params* params = nullptr);
  // per file, the bytes of its chunks seen first in it, earlier in it and in
  // other files, and the other file that holds most of them
  // (sdcas_chunk_sharing; rep: confirm_duplicates' rep over the chunks)
  struct Sharing {
    std::vector<uint64_t> new_bytes, self_bytes, other_bytes, peer_bytes;
    std::vector<int64_t> peer;  // -1: none
    sdcas_sharing_counts counts{};
  };
  Sharing chunk_sharing(const std::vector<uint32_t>& chunk_file, const std::vector<uint64_t>& chunk_len,
                        const std::vector<int64_t>& rep, size_t n_files);
  // chunk_messages over windows (sdcas_chunk_windows): window i holds bytes of
  // a file from one of its cuts on, final[i] != 0 says that it ends where the
  // file ends (final empty: all do); consumed[i] is where the next window of
  // that file begins, relative to this one
  struct WindowChunks : Chunks {
    std::vector<uint64_t> consumed;
  };
  WindowChunks chunk_windows(const std::vector<uint8_t>& blob, const std::vector<uint64_t>& offsets,
                             const std::vector<uint64_t>& lens, const std::vector<uint8_t>& final,
                             const sdcas_chunk_params* params = nullptr);

  // a batch's (key, digest) pairs against a chunk index
  // (sdcas_chunk_index_match); valid may be empty (every query takes part)
  struct IndexMatch {
    std::vector<int64_t> pos;     // the entry with the query's key and digest, -1: none
    std::vector<uint64_t> value;  // its value, or 0
    sdcas_index_match_counts counts{};
  };
  IndexMatch chunk_index_match(const ChunkIndexData& index, const std::vector<uint64_t>& keys,
                               const std::vector<uint8_t>& digests, const std::vector<uint8_t>& valid);
  // the index with the batch's unseen pairs merged in (sdcas_chunk_index_add),
  // its directory at the recommended width for the old entries plus the batch
  struct IndexAdd {
    ChunkIndexData index;
    std::vector<int64_t> pos;    // each pair's entry in the new index
    std::vector<uint8_t> flags;  // SDCAS_INDEX_*
    sdcas_index_add_counts counts{};
  };
  IndexAdd chunk_index_add(const ChunkIndexData& index, const std::vector<uint64_t>& keys,
                           const std::vector<uint8_t>& digests, const std::vector<uint64_t>& values,
                           const std::vector<uint8_t>& valid);

  sdcas_ctx* raw() { return ctx_; }

 private:
  explicit Engine(sdcas_ctx* c, int device) : ctx_(c), device_(device) {}
  [[noreturn]] void fail(int rc, const char* what) const;
  [[noreturn]] void fail_on(sdcas_ctx* c, int rc, const char* what) const;
  sdcas_ctx* dedup_ctx();
  sdcas_ctx* ctx_;
  // the group-by's own context (created with the first dedup): a job's
  // read-ahead holds ctx_ through its path calls, which the group-by of the
  // batch being written would otherwise wait for (SDCORE_DEDUP_CTX=same: ctx_)
  int device_ = -1;
  sdcas_ctx* dedup_ctx_ = nullptr;
  std::mutex dedup_mu_;
};

// single-file forms with the reference signatures (cas.rs:23, hash.rs:11)
Result<std::string> generate_cas_id(Engine& engine, const std::string& path, uint64_t size);
Result<std::string> file_checksum(Engine& engine, const std::string& path);

// cas key <-> the 16-hex cas_id string (cas.rs:61: to_hex()[..16])
std::string key_to_hex(uint64_t key);
uint64_t hex_to_key(const std::string& cas_id);

// ---- rows (the prisma columns this path reads or writes) -------------------

using ObjectKind = int32_t;  // sd_file_ext::kind::ObjectKind discriminant; 0 = Unknown
// the discriminants of crates/file-ext/src/kind.rs:4-59
enum : ObjectKind {
  ObjectKindUnknown = 0, ObjectKindDocument = 1, ObjectKindFolder = 2, ObjectKindText = 3, ObjectKindPackage = 4,
  ObjectKindImage = 5, ObjectKindAudio = 6, ObjectKindVideo = 7, ObjectKindArchive = 8, ObjectKindExecutable = 9,
  ObjectKindAlias = 10, ObjectKindEncrypted = 11, ObjectKindKey = 12, ObjectKindLink = 13,
  ObjectKindWebPageArchive = 14, ObjectKindWidget = 15, ObjectKindAlbum = 16, ObjectKindCollection = 17,
  ObjectKindFont = 18, ObjectKindMesh = 19, ObjectKindCode = 20, ObjectKindDatabase = 21, ObjectKindBook = 22,
  ObjectKindConfig = 23, ObjectKindDotfile = 24, ObjectKindScreenshot = 25,
};
// FilePathRow::kind / file_metadata_batch: derive the kind from the path
constexpr ObjectKind kKindFromPath = -1;

// ---- kind detection (crates/file-ext, file_ext.cpp) ---------------------------

// Extension::from_str (magic.rs:63-79): the ObjectKinds of the categories
// accepting `ext` (case-insensitive), in the Extension enum's order; empty =
// None, one = Known, two = Conflicts ("ts", "mts": Video and Code)
std::vector<ObjectKind> extension_kinds(const std::string& ext);
// Extension::resolve_conflicting(path, false) (magic.rs:176-235) as an
// ObjectKind: nullopt when the path has no (UTF-8) extension, the extension
// is unknown, the file does not open, or a conflict is not "ts"/"mts" as
// written; "ts"/"mts" are Video when the file has the MPEG-TS magic bytes,
// else Code
std::optional<ObjectKind> resolve_conflicting_kind(const std::string& path);
// FileMetadata::new's kind (mod.rs:72-76): the above, or Unknown
ObjectKind object_kind_of(const std::string& path);
using PubId = std::array<uint8_t, 16>;

struct Location {  // location::Data (id, path)
  int32_t id = 0;
  std::string path;
};

// file_path, with the columns of file_path_for_file_identifier and
// file_path_for_object_validator (crates/file-path-helper/src/lib.rs:30-47)
struct FilePathRow {
  int32_t id = 0;
  PubId pub_id{};
  int32_t location_id = 0;
  std::string materialized_path = "/";  // "/" or "/a/b/" (isolated_file_path_data.rs)
  std::string name, extension;
  bool is_dir = false;
  uint64_t size_in_bytes = 0;
  std::optional<std::string> cas_id;
  std::optional<int32_t> object_id;
  std::optional<std::string> integrity_checksum;
  int64_t date_created = 0;
  uint64_t inode = 0;   // FilePathMetadata (crates/file-path-helper/src/lib.rs:125-131)
  bool hidden = false;
  // kKindFromPath: FileMetadata::new derives it (object_kind_of, mod.rs:72-76);
  // >= 0: a kind already known to the caller, used as is
  ObjectKind kind = kKindFromPath;
};

struct ObjectRow {  // object (id, pub_id, kind, date_created)
  int32_t id = 0;
  PubId pub_id{};
  ObjectKind kind = 0;
  int64_t date_created = 0;
};

// location path joined with the row's relative path (assemble_relative_path /
// join_location_relative_path, isolated_file_path_data.rs:533-560)
std::string full_path(const Location& location, const FilePathRow& row);

// The indexer's walk (core/src/location/indexer/walk.rs:432-560) without
// indexer rules: every directory and regular file under the location,
// breadth first, entries of a directory in name order; symlinks skipped
// (walk.rs: `metadata.is_symlink()`); IsolatedFilePathData::new naming
// (isolated_file_path_data.rs:49-87): materialized_path "/a/b/", a file's
// name is Rust's Path::file_stem and its extension Path::extension, a
// directory keeps its whole file name; hidden = name starts with '.'
// (lib.rs:133-147). Rows come back with id 0 (the library assigns ids);
// entries that cannot be read are skipped and reported in `errors`.
std::vector<FilePathRow> walk_location(const Location& location, std::vector<IoError>* errors = nullptr);

// Rust's Path::file_stem / Path::extension of a file name
std::pair<std::string, std::optional<std::string>> file_stem_and_extension(const std::string& file_name);

// ---- the database seam ------------------------------------------------------

class Library {
 public:
  virtual ~Library() = default;
  // orphan_path_filters (file_identifier_job.rs:251-283): (object_id IS NULL OR
  // cas_id IS NULL) AND is_dir = false AND location_id = ? AND size != 0
  // [AND materialized_path LIKE sub%] [AND id >= cursor], ORDER BY id
  virtual size_t count_orphan_file_paths(int32_t location_id, const std::string& sub_materialized_path) = 0;
  virtual std::vector<FilePathRow> get_orphan_file_paths(int32_t location_id, int32_t cursor,
                                                         const std::string& sub_materialized_path, size_t take) = 0;
  // the shallow identifier's orphan_path_filters (shallow.rs:120-142): the
  // same with materialized_path = dir (one directory level, "/" = the
  // location's root) instead of the sub-path prefix
  virtual size_t count_orphan_file_paths_in_dir(int32_t location_id, const std::string& dir) = 0;
  virtual std::vector<FilePathRow> get_orphan_file_paths_in_dir(int32_t location_id, int32_t cursor,
                                                                const std::string& dir, size_t take) = 0;
  // mod.rs:157-178: file_path.cas_id = ? per processed file
  virtual void set_cas_id(int32_t file_path_id, const std::optional<std::string>& cas_id) = 0;
  // mod.rs:181-188: Objects having a file_path whose cas_id is in `cas_ids`,
  // in DB order, each with the cas_ids of its file_paths
  virtual std::vector<std::pair<int32_t, std::vector<std::string>>> existing_objects(
      const std::vector<std::string>& cas_ids) = 0;
  // what the identifier step takes from that lookup (mod.rs:181-188 with the
  // find of :214-224): per cas_id, the first Object in DB order having a
  // file_path with it, in no particular order; cas_ids without one are left
  // out. The default derives it from existing_objects; a database can answer
  // it with one index probe per cas_id.
  virtual std::vector<std::pair<std::string, int32_t>> first_objects(const std::vector<std::string>& cas_ids);
  // set_cas_id then connect of one row as one write: the row's state after
  // mod.rs:157-178 and :352-377. The step uses it for rows without an Object,
  // whose cas_id no lookup of the step can see before the link.
  virtual void set_cas_id_and_connect(int32_t file_path_id, const std::optional<std::string>& cas_id,
                                      int32_t object_id) {
    set_cas_id(file_path_id, cas_id);
    connect(file_path_id, object_id);
  }
  // set_cas_id_and_connect of many rows, one write per row, each row at most
  // once (the default writes them one by one)
  struct CasLink {
    int32_t file_path_id;
    std::optional<std::string> cas_id;
    int32_t object_id;
  };
  virtual void set_cas_ids_and_connect(const std::vector<CasLink>& rows) {
    for (const auto& r : rows) set_cas_id_and_connect(r.file_path_id, r.cas_id, r.object_id);
  }
  // mod.rs:290-327: object::create_unchecked(kind, date_created) -> object id
  virtual int32_t create_object(ObjectKind kind, int64_t date_created) = 0;
  // object::create_many (mod.rs:314-327): Objects created in this order, ids
  // returned in the same order (the default creates them one by one)
  virtual std::vector<int32_t> create_objects(const std::vector<std::pair<ObjectKind, int64_t>>& kinds_dates) {
    std::vector<int32_t> ids;
    ids.reserve(kinds_dates.size());
    for (const auto& [k, d] : kinds_dates) ids.push_back(create_object(k, d));
    return ids;
  }
  // connect_file_path_to_object (mod.rs:352-377)
  virtual void connect(int32_t file_path_id, int32_t object_id) = 0;
  // validator_job.rs:107-123: location_id = ? AND is_dir = false AND
  // integrity_checksum IS NULL [AND materialized_path LIKE sub%]
  virtual std::vector<FilePathRow> file_paths_without_checksum(int32_t location_id,
                                                               const std::string& sub_materialized_path) = 0;
  virtual void set_integrity_checksum(int32_t file_path_id, const std::string& checksum) = 0;
  // confirm_duplicates' rows: location_id = ? AND is_dir = false AND cas_id IS
  // NOT NULL AND integrity_checksum IS NOT NULL [AND materialized_path LIKE
  // sub%], ORDER BY id. A library that does not override it cannot be
  // confirmed: the default throws LibraryError.
  virtual std::vector<FilePathRow> file_paths_with_checksum(int32_t location_id,
                                                            const std::string& sub_materialized_path);
  // the writes between these calls are one batch (sync.write_ops batches a
  // step's operations, core/crates/sync/src/manager.rs:70-93): one
  // transaction in a database; no-ops in memory
  // tree_report's rows: location_id = ? [AND materialized_path LIKE sub%],
  // files and directories, ORDER BY id (the default throws LibraryError)
  virtual std::vector<FilePathRow> file_paths_in_location(int32_t location_id,
                                                          const std::string& sub_materialized_path);
  virtual void begin_batch() {}
  virtual void end_batch() {}
  // A job about to identify `orphans` rows may let the database keep what
  // first_objects answers on the host for the job's duration instead of in
  // an index it would update row by row (SqliteLibrary: the cas_id index is
  // dropped, its content kept as a cas_id -> first Object map that every
  // write of the job updates, and the index rebuilt in one pass by
  // end_bulk_identify). Returns whether it did. Every query answers as
  // before; the job must be the library's only writer meanwhile.
  virtual bool begin_bulk_identify(size_t orphans) {
    (void)orphans;
    return false;
  }
  virtual void end_bulk_identify() {}
  // The job reads its next batch (orphans past the current batch's last row,
  // which the current batch never writes) while the current batch's writes
  // are still open. A database that can serve that read from another
  // connection without waiting for them (SQLite in WAL mode: a second,
  // read-only connection) says so here; the job then fetches on its
  // metadata thread, concurrently with the writes. The concurrent call
  // answers what get_orphan_file_paths would after the current batch commits.
  virtual bool concurrent_orphan_reads() { return false; }
  virtual std::vector<FilePathRow> get_orphan_file_paths_concurrent(int32_t location_id, int32_t cursor,
                                                                    const std::string& sub_materialized_path,
                                                                    size_t take) {
    return get_orphan_file_paths(location_id, cursor, sub_materialized_path, take);
  }
};

// In-memory tables with the reference's query semantics (ids ascending = DB order)
class MemoryLibrary : public Library {
 public:
  std::vector<FilePathRow> file_paths;  // kept sorted by id
  std::vector<ObjectRow> objects;       // ids ascending

  FilePathRow& add_file_path(FilePathRow row);  // assigns id and pub_id when 0
  const FilePathRow* file_path(int32_t id) const;

  size_t count_orphan_file_paths(int32_t location_id, const std::string& sub) override;
  std::vector<FilePathRow> get_orphan_file_paths(int32_t location_id, int32_t cursor, const std::string& sub,
                                                 size_t take) override;
  size_t count_orphan_file_paths_in_dir(int32_t location_id, const std::string& dir) override;
  std::vector<FilePathRow> get_orphan_file_paths_in_dir(int32_t location_id, int32_t cursor, const std::string& dir,
                                                        size_t take) override;
  void set_cas_id(int32_t file_path_id, const std::optional<std::string>& cas_id) override;
  std::vector<std::pair<int32_t, std::vector<std::string>>> existing_objects(
      const std::vector<std::string>& cas_ids) override;
  int32_t create_object(ObjectKind kind, int64_t date_created) override;
  void connect(int32_t file_path_id, int32_t object_id) override;
  std::vector<FilePathRow> file_paths_without_checksum(int32_t location_id, const std::string& sub) override;
  std::vector<FilePathRow> file_paths_with_checksum(int32_t location_id, const std::string& sub) override;
  std::vector<FilePathRow> file_paths_in_location(int32_t location_id, const std::string& sub) override;
  void set_integrity_checksum(int32_t file_path_id, const std::string& checksum) override;

 private:
  FilePathRow* find(int32_t id);
  bool orphan(const FilePathRow& r, int32_t location_id, const std::string& sub) const;
  int32_t next_file_path_id_ = 1, next_object_id_ = 1;
};

// SQLite tables with the columns of the reference's file_path / object
// models (core/prisma/schema.prisma) and the reference's queries as prepared
// statements (the DB side of the join). Differences, both
// deliberate: an index on file_path(cas_id), which the reference's schema
// lacks (the existing-Object lookup of mod.rs:181-188 then scans the table),
// and a `kind_hint` column carrying FilePathRow::kind (kKindFromPath unless a
// caller supplies a kind).
// Batches are transactions (begin_batch / end_batch).
class SqliteLibrary : public Library {
 public:
  // path of the database file, or ":memory:"; throws std::runtime_error.
  // cas_id_index = false keeps the reference's schema (no index on cas_id),
  // for comparison. object_id_index: an index on file_path(object_id), which
  // the reference's schema lacks too and the identifier step does not read
  // (only existing_objects' join does); off by default, since every link
  // would update it.
  static std::unique_ptr<SqliteLibrary> open(const std::string& path, bool cas_id_index = true,
                                             bool object_id_index = false);
  ~SqliteLibrary() override;

  // insert rows (ids and pub_ids assigned when 0), one transaction
  void add_file_paths(std::vector<FilePathRow>& rows);
  std::optional<FilePathRow> file_path(int32_t id);
  std::vector<ObjectRow> objects();

  size_t count_orphan_file_paths(int32_t location_id, const std::string& sub) override;
  std::vector<FilePathRow> get_orphan_file_paths(int32_t location_id, int32_t cursor, const std::string& sub,
                                                 size_t take) override;
  size_t count_orphan_file_paths_in_dir(int32_t location_id, const std::string& dir) override;
  std::vector<FilePathRow> get_orphan_file_paths_in_dir(int32_t location_id, int32_t cursor, const std::string& dir,
                                                        size_t take) override;
  void set_cas_id(int32_t file_path_id, const std::optional<std::string>& cas_id) override;
  std::vector<std::pair<int32_t, std::vector<std::string>>> existing_objects(
      const std::vector<std::string>& cas_ids) override;
  // one probe of the cas_id index per cas_id (the reference's schema, without
  // that index: the existing_objects query)
  std::vector<std::pair<std::string, int32_t>> first_objects(const std::vector<std::string>& cas_ids) override;
  void set_cas_id_and_connect(int32_t file_path_id, const std::optional<std::string>& cas_id,
                              int32_t object_id) override;
  // UPDATE ... FROM (VALUES ...) of up to 64 rows per statement (bulk
  // identify: of rows without an Object, a row found with one takes the
  // general path)
  void set_cas_ids_and_connect(const std::vector<CasLink>& rows) override;
  int32_t create_object(ObjectKind kind, int64_t date_created) override;
  // multi-row INSERTs of up to 64 Objects each
  std::vector<int32_t> create_objects(const std::vector<std::pair<ObjectKind, int64_t>>& kinds_dates) override;
  void connect(int32_t file_path_id, int32_t object_id) override;
  std::vector<FilePathRow> file_paths_without_checksum(int32_t location_id, const std::string& sub) override;
  std::vector<FilePathRow> file_paths_with_checksum(int32_t location_id, const std::string& sub) override;
  std::vector<FilePathRow> file_paths_in_location(int32_t location_id, const std::string& sub) override;
  void set_integrity_checksum(int32_t file_path_id, const std::string& checksum) override;
  void begin_batch() override;
  void end_batch() override;
  // with the cas_id index, when the library holds at most 4x `orphans` rows
  // with a cas_id (loading them costs less than indexing the job's rows one
  // by one): the index goes, a host map of its MIN(object_id) per cas_id
  // stays; a write that could make the map stale (a row with an Object and
  // a cas_id gets another of either) restores the index first — inside a
  // batch that commits the batch's writes so far and opens a new
  // transaction for the rest (CREATE INDEX runs in its own)
  bool begin_bulk_identify(size_t orphans) override;
  void end_bulk_identify() override;
  bool bulk_identify_active() const;
  // a file database (not ":memory:") opens a second, read-only connection
  // for the job's read-ahead (WAL readers do not wait for the writer)
  bool concurrent_orphan_reads() override;
  std::vector<FilePathRow> get_orphan_file_paths_concurrent(int32_t location_id, int32_t cursor,
                                                            const std::string& sub, size_t take) override;

  // The chunk index's tables (similarity_report_indexed): chunk_index(digest
  // BLOB PRIMARY KEY, file_path_id INTEGER), one row per distinct chunk with
  // the row that held it first — the key is the digest's first 8 bytes and
  // ORDER BY digest is index order, since SQLite orders BLOBs as memcmp does —
  // and chunk_indexed_file(file_path_id INTEGER PRIMARY KEY, size INTEGER), the
  // rows whose chunks are in it. Both are created by the first call below.
  // The stored index, its directory at the recommended width; checked
  // (sdcas_chunk_index_check, and every digest 32 bytes): LibraryError with
  // SDCAS_E_INVALID for a table that is no index.
  ChunkIndexData load_chunk_index();
  // (file_path id, bytes read) of the rows indexed so far, ascending by id
  std::vector<std::pair<int32_t, uint64_t>> chunk_indexed_files();
  // one transaction, and the only writes to the two tables: the added chunks
  // (32 bytes each) with their owners, and the rows now indexed. A digest
  // already stored or a row already indexed is std::runtime_error, and then
  // nothing of the call is kept.
  void append_chunk_index(const std::vector<uint8_t>& digests, const std::vector<int32_t>& owners,
                          const std::vector<std::pair<int32_t, uint64_t>>& files);

 private:
  struct Impl;
  explicit SqliteLibrary(std::unique_ptr<Impl> d);
  std::unique_ptr<Impl> d_;
};

// ---- file_identifier ----------------------------------------------------------

// FileMetadata (mod.rs:48-53)
struct FileMetadata {
  std::optional<std::string> cas_id;  // None for an empty file (mod.rs:78-86)
  ObjectKind kind = 0;
  uint64_t len = 0;  // fs_metadata.len()
  // file_checksum of the same read (hash.rs:11-25; 64 lowercase hex): set only
  // by file_metadata_batch with `checksums`, for the identifier job that also
  // fills integrity_checksum (FileIdentifierJobInit::checksums)
  std::optional<std::string> integrity_checksum;
};

// FileMetadata::new for a batch of (full path, kind): fs::metadata, the
// is_dir assertion (mod.rs:67-70, std::logic_error here), the kind from the
// path (object_kind_of) unless the pair carries one (>= 0), cas_id only for
// len != 0, one generate_cas_ids call for the batch (the join_all of
// mod.rs:105-147). Errors carry the path (FileIOError). size_hints (may be
// null; one per file): the indexer's sizes (file_path size_in_bytes), which
// only plan the reads' staging (sdcas_file_metadata: the metadata is fstat of
// each read's descriptor).
std::vector<Result<FileMetadata>> file_metadata_batch(Engine& engine,
                                                      const std::vector<std::pair<std::string, ObjectKind>>& files,
                                                      const std::vector<uint64_t>* size_hints = nullptr);
// The same with `checksums`: every file's cas_id and checksum from one open
// and one read (sdcas_identify_checksums); integrity_checksum is set for every
// file read without error, the empty ones included.
std::vector<Result<FileMetadata>> file_metadata_batch(Engine& engine,
                                                      const std::vector<std::pair<std::string, ObjectKind>>& files,
                                                      const std::vector<uint64_t>* size_hints, bool checksums);

// The DB half of the job's steps over a batch of its orphans (mod.rs:157-342
// per step): write the cas_id of every row the steps read, look up the
// existing Objects of their cas_ids, group (the GPU's sdcas_dedup_window in
// identifier_job_step; any function with its encoding here), create Objects
// and link; a row the steps read whose FileMetadata carries an
// integrity_checksum gets it written too (set_integrity_checksum, in its
// step's batch after its cas_id). md[i] is file_paths[i]'s FileMetadata. window (in: max_steps,
// more; out: steps, rows, rereads) may be null: the whole job over these rows.
// The steps' bookkeeping comes from sdcas_job_plan before any write. A batch
// must not hold a row to re-identify — an Object but no cas_id (the indexer
// nulls cas_id of a changed file) — past its first step: its cas_id, written
// in its own step, makes its Object an existing one for the steps after
// (mod.rs:157-188); the job cuts its batches there (run_file_identifier_job),
// and this function throws std::invalid_argument if one is left.
using GroupBy = std::function<Engine::Dedup(const std::vector<uint64_t>& keys, const std::vector<uint8_t>& has_key,
                                            const std::vector<int32_t>& status,
                                            const std::vector<uint64_t>& existing_keys, sdcas_job_window& window)>;
std::pair<size_t, size_t> identifier_step_db(Library& db, const std::vector<FilePathRow>& file_paths,
                                             const std::vector<Result<FileMetadata>>& md, const GroupBy& group_by,
                                             sdcas_job_window* window = nullptr,
                                             size_t chunk_size = SDCAS_IDENTIFIER_CHUNK_SIZE);

// sdcas_job_plan over the rows' FileMetadata: per row the step that first
// reads it (UINT64_MAX: none) and how many steps read it
struct StepPlan {
  std::vector<uint64_t> step;
  std::vector<uint32_t> reads;
};
StepPlan plan_steps(const std::vector<Result<FileMetadata>>& md, size_t chunk_size, sdcas_job_window& window);

// identifier_job_step (mod.rs:98-350) over `file_paths` in id order: one
// step of the reference per chunk_size rows (CHUNK_SIZE = 100), the cursor
// rule included (a step's last row that stays an orphan is read again by the
// next step). window as in identifier_step_db. Returns (total_created,
// total_linked) as mod.rs:349 does, summed over the steps.
std::pair<size_t, size_t> identifier_job_step(Engine& engine, Library& db, const Location& location,
                                              const std::vector<FilePathRow>& file_paths,
                                              size_t chunk_size = SDCAS_IDENTIFIER_CHUNK_SIZE,
                                              sdcas_job_window* window = nullptr);

// FileIdentifierJobRunMetadata (file_identifier_job.rs:54-71)
struct FileIdentifierJobRunMetadata {
  int32_t cursor = 0;
  size_t total_orphan_paths = 0;
  size_t total_objects_created = 0;
  size_t total_objects_linked = 0;
  size_t total_objects_ignored = 0;
  size_t steps = 0;           // the reference's steps
  size_t batches = 0;         // fetches of `batch` rows
  size_t rereads = 0;         // rows two consecutive steps read
  bool early_finish = false;  // JobError::EarlyFinish (file_identifier_job.rs:184-191)
  bool bulk_identify = false; // the library kept its lookups on the host (FileIdentifierJobInit::bulk_identify)
};

// FileIdentifierJobInit (file_identifier_job.rs:33-37); batch = orphans
// fetched per GPU call (the reference fetches CHUNK_SIZE = 100 per step; a
// larger batch runs several of its steps in one call with identical results)
struct FileIdentifierJobInit {
  Location location;
  std::string sub_materialized_path;  // "" or "/sub/dir/"
  size_t batch = SDCAS_IDENTIFIER_CHUNK_SIZE;
  // let the library trade its lookup index for a host map during the job
  // (Library::begin_bulk_identify); the rows and Objects the job leaves are
  // the same either way
  bool bulk_identify = false;
  // also fill integrity_checksum (what run_object_validator_job would write
  // afterwards) from the same read of each file: the FileMetadata comes from
  // sdcas_identify_checksums, and every row the steps read whose metadata
  // carries a checksum gets it in that row's step. Files the indexer saw
  // empty are no orphans, so no step reads them: run_file_identifier_job
  // checksums those after its steps, as the validator would. Clear: the job
  // writes no checksum, whatever its metadata function returns.
  bool checksums = false;
};

// init (count orphans, cursor = first orphan id, task_count = ceil(count /
// CHUNK_SIZE) steps, file_identifier_job.rs:125-176), then batches: fetch
// `batch` orphans with id >= cursor, run as many of the job's steps over them
// as fit (identifier_job_step with a window), advance the cursor to the last
// row the steps read (mod.rs:401-405). meta.steps counts the reference's
// steps, meta.batches the fetches.
FileIdentifierJobRunMetadata run_file_identifier_job(Engine& engine, Library& db, const FileIdentifierJobInit& init);

// the same loop with any group-by (tests: the CPU oracle), metadata from
// `metadata` (tests: synthetic) instead of the files
using MetadataFn = std::function<std::vector<Result<FileMetadata>>(const std::vector<FilePathRow>& rows)>;
FileIdentifierJobRunMetadata run_file_identifier_job_with(Library& db, const FileIdentifierJobInit& init,
                                                          const MetadataFn& metadata, const GroupBy& group_by);

// the shallow identifier (file_identifier/shallow.rs:24-118, run by
// light_scan_location): the same steps over the orphans of ONE directory
// level (materialized_path = dir; "" or "/" = the location's root), task_count
// = ceil(orphans / CHUNK_SIZE) with no early finish — a step that finds no
// rows leaves the cursor where it is (mod.rs:401-405). Its first cursor comes
// from an unordered find_first (shallow.rs:74-84, `.order_by` commented out):
// the canonical pick here is the lowest orphan id, which is what SQLite returns
// for that query when it scans in rowid order. `batch` as in
// FileIdentifierJobInit.
struct ShallowIdentifierReport {
  size_t orphans = 0, steps = 0, batches = 0, rereads = 0;
  size_t created = 0, linked = 0;
  int32_t cursor = 0;
};
ShallowIdentifierReport shallow_file_identifier(Engine& engine, Library& db, const Location& location,
                                                const std::string& dir, size_t batch = SDCAS_IDENTIFIER_CHUNK_SIZE);
ShallowIdentifierReport shallow_file_identifier_with(Library& db, const Location& location, const std::string& dir,
                                                     size_t batch, const MetadataFn& metadata,
                                                     const GroupBy& group_by);

// ---- object validator -----------------------------------------------------------

struct ObjectValidatorJobInit {  // validator_job.rs:38-42
  Location location;
  std::string sub_materialized_path;
  size_t batch = SDCAS_IDENTIFIER_CHUNK_SIZE;  // the reference runs one file per step
};

struct ObjectValidatorReport {
  size_t task_count = 0;   // rows selected at init
  size_t checksummed = 0;  // integrity_checksum written
  // the first file whose checksum failed: the reference's execute_step returns
  // ValidatorError::FileIO (validator_job.rs:154-156) and the job stops there
  std::optional<IoError> error;
};

ObjectValidatorReport run_object_validator_job(Engine& engine, Library& db, const ObjectValidatorJobInit& init);

// ---- duplicates confirmed by checksum ----------------------------------------------
//
// The identifier links file_paths by cas_id, which above 100 KiB hashes
// 57,352 bytes of the file (cas.rs:23-62): files of one length that agree in
// those windows end on one Object whatever else they hold. Once the rows
// carry their integrity_checksum too (FileIdentifierJobInit::checksums, or
// the validator), the pair (cas_id, checksum) says which rows are the same
// file and which cas_ids collide.
struct DuplicateReport {
  // rows with one cas_id and one checksum
  struct Class {
    std::string cas_id, checksum;
    std::vector<int32_t> file_path_ids;  // ascending
  };
  // a cas_id whose rows carry more than one checksum
  struct Collision {
    std::string cas_id;
    std::vector<std::vector<int32_t>> classes;  // file_path ids ascending, classes by their first id
    std::vector<int32_t> object_ids;  // the distinct Objects those rows are linked to, ascending
  };
  std::vector<Class> confirmed;       // the classes of two or more rows, ordered by their first id
  std::vector<Collision> collisions;  // one per collided cas_id, ordered by its first id
  sdcas_confirm_counts counts{};
};

// The report's shaping, no GPU: rows in id order and the group-by's answer
// for them (sdcas_confirm_duplicates' out_rep / out_key_rep / out_flags with
// row i as file i); rows flagged SDCAS_CONFIRM_SKIPPED are left out. The
// counts are taken from the three arrays.
DuplicateReport duplicate_report_from(const std::vector<FilePathRow>& rows, const std::vector<int64_t>& rep,
                                      const std::vector<int64_t>& key_rep, const std::vector<uint8_t>& flags);

// Read-only: reads Library::file_paths_with_checksum, turns the hex strings
// into keys and digests (a row whose cas_id is not 16 or whose checksum is not
// 64 hex characters takes no part), groups them on the GPU
// (Engine::confirm_duplicates) and shapes the report. Writes nothing.
DuplicateReport confirm_duplicates(Engine& engine, Library& db, int32_t location_id, const std::string& sub = "");

// ---- duplicate sets: what deleting the extra copies gives back ---------------------
struct ReclaimReport {
  struct Set {
    std::vector<int32_t> file_path_ids;  // ascending
    uint64_t bytes = 0;                  // one copy (the first row's size_in_bytes)
    uint64_t reclaimable_bytes = 0;      // (rows - 1) * bytes, modulo 2^64
    bool operator==(const Set& o) const {
      return file_path_ids == o.file_path_ids && bytes == o.bytes && reclaimable_bytes == o.reclaimable_bytes;
    }
  };
  std::vector<Set> sets;  // in the order of the arrays they were shaped from
  sdcas_sets_counts counts{};
};

// The report's shaping, no GPU: rows in id order and sdcas_duplicate_sets'
// answer for them with row i as file i (Engine::Sets' arrays, trimmed). Throws
// std::invalid_argument when the arrays do not describe sets of these rows.
ReclaimReport reclaim_report_from(const std::vector<FilePathRow>& rows, const std::vector<int64_t>& set_rep,
                                  const std::vector<uint64_t>& set_offsets, const std::vector<uint64_t>& set_bytes,
                                  const std::vector<int64_t>& members, const sdcas_sets_counts& counts);

// Read-only: reads Library::file_paths_with_checksum, confirms the rows'
// (cas_id, checksum) pairs (Engine::confirm_duplicates), groups the answer
// into sets with the rows' size_in_bytes, the most reclaimable bytes first
// (Engine::duplicate_sets, SDCAS_SETS_BY_RECLAIMABLE). Writes nothing.
ReclaimReport reclaim_report(Engine& engine, Library& db, int32_t location_id, const std::string& sub = "");

// ---- duplicate directories: the top-most duplicate sets of a location ---------------
// The tree of a location's rows, no GPU: parent[i] is the index of the
// directory row whose own path (materialized_path + name + "/") is row i's
// materialized_path, or -1 when that row is absent (the location's root, or
// the directory a `sub` scope starts at); of several directory rows with one
// path the first counts.
struct TreeShape {
  std::vector<int64_t> parent;
  std::vector<uint8_t> is_dir;
};
TreeShape tree_shape_from(const std::vector<FilePathRow>& rows);
// the name a row stands under in its directory: a directory's name, a file's
// name with "." and its extension when it has one
std::string entry_name(const FilePathRow& row);

struct TreeReport {
  struct Set {
    std::vector<int32_t> file_path_ids;  // ascending
    bool is_dir = false;                 // the kind of the set's first row
    uint64_t tree_bytes = 0;             // one copy: a file's size, or all file bytes below a directory
    uint64_t tree_files = 0;             // 1, or the files below a directory
    uint64_t reclaimable_bytes = 0;      // (rows - 1) * tree_bytes, modulo 2^64
    bool operator==(const Set& o) const {
      return file_path_ids == o.file_path_ids && is_dir == o.is_dir && tree_bytes == o.tree_bytes &&
             tree_files == o.tree_files && reclaimable_bytes == o.reclaimable_bytes;
    }
  };
  std::vector<Set> sets;  // in the order of the arrays they were shaped from
  sdcas_tree_counts tree{};
  sdcas_top_counts top{};
  sdcas_sets_counts counts{};
};
// The report's shaping, no GPU: rows and, with row i as entry i, the per-entry
// rollups (Engine::TreeDigests) and the sets of Engine::duplicate_sets over
// top_rep and tree_bytes. Throws std::invalid_argument when the arrays do not
// fit the rows or each other.
TreeReport tree_report_from(const std::vector<FilePathRow>& rows, const std::vector<uint64_t>& tree_bytes,
                            const std::vector<uint64_t>& tree_files, const std::vector<int64_t>& set_rep,
                            const std::vector<uint64_t>& set_offsets, const std::vector<uint64_t>& set_bytes,
                            const std::vector<int64_t>& members, const sdcas_sets_counts& counts);
// Read-only: reads Library::file_paths_in_location (files and directories),
// hashes the names, gives every directory its digest (a file without a
// 64-hex integrity_checksum is invalid and makes its ancestors INCOMPLETE; a
// file's key is its checksum's first 8 bytes), confirms all entries at once,
// keeps the top-most duplicates and lists them, directories and files mixed,
// the most reclaimable first. Writes nothing.
TreeReport tree_report(Engine& engine, Library& db, int32_t location_id, const std::string& sub = "");

// ---- files that share most of their bytes ---------------------------------------------
struct SimilarityReport {
  struct Pair {
    int32_t file_path_id = 0;
    int32_t peer_id = 0;        // the other row that holds most of this row's repeated bytes
    uint64_t shared_bytes = 0;  // the bytes of this row's chunks first seen in the peer
    uint64_t size = 0;          // the bytes read from this row's file
    bool operator==(const Pair& o) const {
      return file_path_id == o.file_path_id && peer_id == o.peer_id && shared_bytes == o.shared_bytes && size == o.size;
    }
  };
  std::vector<Pair> pairs;  // most shared bytes first, ties by file_path id ascending
  sdcas_chunk_counts chunks{};
  sdcas_sharing_counts counts{};
};
// The report's shaping, no GPU: rows and, with row i as file i, the bytes read
// from each and Engine::Sharing's peer / peer_bytes. Throws
// std::invalid_argument when the arrays do not fit the rows or name no other row.
SimilarityReport similarity_report_from(const std::vector<FilePathRow>& rows, const std::vector<uint64_t>& sizes,
                                        const std::vector<int64_t>& peer, const std::vector<uint64_t>& peer_bytes);
// Read-only: reads the file rows of Library::file_paths_in_location(location.id,
// sub) and their files' contents whole (a file that cannot be read counts as
// empty; LibraryError with SDCAS_E_CAPACITY when they hold more than max_bytes
// in all: the contents are resident at once), cuts them into content-defined
// chunks, confirms the chunks' (key, digest) pairs, runs the sharing pass and
// lists every row that has a peer. Writes nothing.
SimilarityReport similarity_report(Engine& engine, Library& db, const Location& location, const std::string& sub = "",
                                   uint64_t max_bytes = 1ull << 30);


// ---- the same for files that are not resident at once ----------------------------------
// The windows of files of these sizes, taken in order (no GPU): consecutive
// whole files while they fit in window_bytes together (streamed false); a
// file larger than window_bytes alone, over consecutive windows (streamed
// true, n_files 1). Throws std::invalid_argument for window_bytes == 0.
struct WindowPlan {
  size_t first_file = 0, n_files = 0;
  bool streamed = false;
  bool operator==(const WindowPlan& o) const {
    return first_file == o.first_file && n_files == o.n_files && streamed == o.streamed;
  }
};
std::vector<WindowPlan> plan_chunk_windows(const std::vector<uint64_t>& sizes, uint64_t window_bytes);
// One window's result: its files are first_file .. first_file + offsets.size(),
// offsets where each begins in the window's blob (Engine::chunk_windows'
// argument), file_pos where a streamed file's window begins in the file.
struct ChunkWindow {
  size_t first_file = 0;
  uint64_t file_pos = 0;
  std::vector<uint64_t> offsets;
  Engine::WindowChunks chunks;
};
// The windows' arrays as one call over the whole files would give them (no
// GPU): chunk_file are indices into the n_files files, chunk_off offsets in
// the file, file_chunks the files' first chunks, the counts summed;
// sizes[i] the bytes consumed of file i. The windows come in file order:
// throws std::invalid_argument for a window that goes back, names a file past
// n_files, or whose arrays do not fit each other.
Engine::Chunks merge_chunk_windows(const std::vector<ChunkWindow>& windows, size_t n_files,
                                   std::vector<uint64_t>* sizes = nullptr);
// similarity_report without the contents being resident at once: the files
// go through windows of at most window_bytes (plan_chunk_windows; a streamed
// file's window is grown when it consumed nothing), the chunk arrays, keys
// and digests are kept, and one confirm and one sharing pass run over all of
// them. The same report as similarity_report whenever that one can run.
SimilarityReport similarity_report_streamed(Engine& engine, Library& db, const Location& location,
                                            const std::string& sub = "", uint64_t window_bytes = 256ull << 20);

// ---- the same against the chunks stored before ------------------------------------------
// The per-file sharing of a batch against a chunk index (no device work of its
// own: Engine::chunk_sharing over the batch's chunks with one pseudo-chunk per
// matched pair in front). rep / hit_value: Engine::confirm_duplicates' rep over
// the batch's chunks and Engine::chunk_index_match's pos / value. The origin of
// a chunk is the stored value when the index holds it, else file_ids[the file of
// its lowest copy in the batch]; peer is a FILE ID (ties to the lowest), -1 none.
struct IndexedSharing {
  std::vector<uint64_t> new_bytes, self_bytes, other_bytes, indexed_bytes, peer_bytes;
  std::vector<int64_t> peer;
};
IndexedSharing indexed_sharing(Engine& engine, const Engine::Chunks& chunks, const std::vector<int64_t>& rep,
                               const Engine::IndexMatch& match, const std::vector<uint64_t>& file_ids);
// similarity_report_streamed for the rows that came since the last call: the
// location's file rows that chunk_indexed_file does not hold yet go through
// the windows, their chunks are confirmed, matched against the stored index
// (SqliteLibrary::load_chunk_index) and added to it with their row's id, and
// the added chunks and the rows are recorded (append_chunk_index, the only
// writes). Reports a Pair for each of those rows that has a peer; a peer may
// be a row indexed by an earlier call. Called after each of several batches
// of files is created, the union of its reports is similarity_report_streamed's
// over all of them. With no new row it reports nothing and writes nothing.
SimilarityReport similarity_report_indexed(Engine& engine, SqliteLibrary& db, const Location& location,
                                           const std::string& sub = "", uint64_t window_bytes = 256ull << 20);

}  // namespace sdcore
