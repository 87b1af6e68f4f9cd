// sdcore.cpp — C++ host mirror of sd-core's content-identification path over
// libsdcas (see include/sdcore.hpp for the reference file:line of each entry).
#include "sdcore.hpp"

#include <dirent.h>
#include <fcntl.h>
#include <unistd.h>
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <exception>
#include <future>
#include <mutex>
#include <set>
#include <thread>
#include <unordered_map>
#include <unordered_set>

namespace sdcore {

std::string IoError::message() const {
  std::string m = unexpected_eof() ? "failed to fill whole buffer" : std::strerror(code);
  return path.empty() ? m : m + " <path='" + path + "'>";
}

// ---- Engine -------------------------------------------------------------------

void Engine::fail(int rc, const char* what) const { fail_on(ctx_, rc, what); }

void Engine::fail_on(sdcas_ctx* c, int rc, const char* what) const {
  throw LibraryError(rc, std::string(what) + ": " + sdcas_last_error(c));
}

sdcas_ctx* Engine::dedup_ctx() {
  static const bool same = [] {
    const char* v = getenv("SDCORE_DEDUP_CTX");
    return v && strcmp(v, "same") == 0;
  }();
  if (same) return ctx_;
  std::lock_guard<std::mutex> g(dedup_mu_);
  if (!dedup_ctx_) {
    sdcas_options opts = SDCAS_OPTIONS_INIT;
    opts.device = device_;
    sdcas_ctx* c = nullptr;
    if (sdcas_init(&opts, &c) != SDCAS_OK) {  // no second context: share the first
      if (c) sdcas_destroy(c);
      return ctx_;
    }
    dedup_ctx_ = c;
  }
  return dedup_ctx_;
}

std::unique_ptr<Engine> Engine::open(const Options& o) {
  sdcas_options opts = SDCAS_OPTIONS_INIT;
  opts.device = o.device;
  opts.io_threads = o.io_threads;
  opts.flags = o.flags;
  opts.staging_bytes = o.staging_bytes;
  opts.progress = o.progress;
  opts.progress_user = o.progress_user;
  opts.cancel = o.cancel;
  sdcas_ctx* c = nullptr;
  const int rc = sdcas_init(&opts, &c);
  if (rc != SDCAS_OK) {
    std::string msg = c ? sdcas_last_error(c) : "sdcas_init failed";
    if (c) sdcas_destroy(c);
    throw LibraryError(rc, msg);
  }
  return std::unique_ptr<Engine>(new Engine(c, o.device));
}

Engine::~Engine() {
  if (dedup_ctx_) sdcas_destroy(dedup_ctx_);
  sdcas_destroy(ctx_);
}

std::string key_to_hex(uint64_t key) {
  char b[17];
  sdcas_key_to_hex(key, b);
  return std::string(b, 16);
}

uint64_t hex_to_key(const std::string& cas_id) {
  if (cas_id.size() != 16) throw std::invalid_argument("cas_id must be 16 hex chars: " + cas_id);
  return std::stoull(cas_id, nullptr, 16);
}

Engine::RawMetadata Engine::file_metadata(const std::vector<const char*>& paths, const uint64_t* size_hints) {
  const size_t n = paths.size();
  RawMetadata m;
  m.size.resize(n);
  m.key.resize(n);
  m.status.resize(n);
  m.flags.resize(n);
  if (n) {
    const int rc = sdcas_file_metadata(ctx_, paths.data(), size_hints, n, m.size.data(), m.key.data(),
                                       m.status.data(), m.flags.data());
    if (rc != SDCAS_OK) fail(rc, "sdcas_file_metadata");
  }
  return m;
}

Engine::RawMetadata Engine::identify_checksums(const std::vector<const char*>& paths, const uint64_t* size_hints) {
  const size_t n = paths.size();
  RawMetadata m;
  m.size.resize(n);
  m.key.resize(n);
  m.status.resize(n);
  m.flags.resize(n);
  m.digest.resize(32 * n);
  if (n) {
    const int rc = sdcas_identify_checksums(ctx_, paths.data(), size_hints, n, m.size.data(), m.key.data(),
                                            m.digest.data(), m.status.data(), m.flags.data());
    if (rc != SDCAS_OK) fail(rc, "sdcas_identify_checksums");
  }
  return m;
}

std::vector<Result<std::string>> Engine::generate_cas_ids(
    const std::vector<std::pair<std::string, uint64_t>>& files) {
  const size_t n = files.size();
  std::vector<const char*> paths(n);
  std::vector<uint64_t> sizes(n), keys(n);
  std::vector<int32_t> st(n);
  for (size_t i = 0; i < n; ++i) {
    paths[i] = files[i].first.c_str();
    sizes[i] = files[i].second;
  }
  if (n) {
    const int rc = sdcas_cas_ids(ctx_, paths.data(), sizes.data(), n, keys.data(), st.data());
    if (rc != SDCAS_OK) fail(rc, "sdcas_cas_ids");
  }
  std::vector<Result<std::string>> out;
  out.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    if (st[i]) out.emplace_back(IoError{st[i], files[i].first});
    else out.emplace_back(key_to_hex(keys[i]));
  }
  return out;
}

std::vector<Result<std::string>> Engine::file_checksums(const std::vector<std::string>& files) {
  const size_t n = files.size();
  std::vector<const char*> paths(n);
  std::vector<uint8_t> d(32 * n);
  std::vector<int32_t> st(n);
  for (size_t i = 0; i < n; ++i) paths[i] = files[i].c_str();
  if (n) {
    const int rc = sdcas_checksums(ctx_, paths.data(), n, d.data(), st.data());
    if (rc != SDCAS_OK) fail(rc, "sdcas_checksums");
  }
  std::vector<Result<std::string>> out;
  out.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    if (st[i]) {
      out.emplace_back(IoError{st[i], files[i]});
    } else {
      char h[65];
      sdcas_digest_to_hex(&d[32 * i], h);
      out.emplace_back(std::string(h, 64));
    }
  }
  return out;
}

Engine::Dedup Engine::dedup(const std::vector<uint64_t>& keys, const std::vector<uint8_t>& has_key,
                            const std::vector<int32_t>& status, size_t chunk_size,
                            const std::vector<uint64_t>& existing_keys, sdcas_job_window* window) {
  const size_t n = keys.size();
  if (has_key.size() != n || (!status.empty() && status.size() != n))
    throw std::invalid_argument("dedup: keys / has_key / status lengths differ");
  Dedup r;
  r.link.assign(n, 0);
  if (!n) {
    if (window) window->steps = window->rows = window->rereads = 0;
    return r;
  }
  sdcas_ctx* dc = dedup_ctx();
  const int rc = sdcas_dedup_window(dc, keys.data(), has_key.data(), status.empty() ? nullptr : status.data(), n,
                                    chunk_size, existing_keys.empty() ? nullptr : existing_keys.data(),
                                    existing_keys.size(), window, r.link.data(), &r.created, &r.linked);
  if (rc != SDCAS_OK) fail_on(dc, rc, "sdcas_dedup_window");
  return r;
}

Result<std::string> generate_cas_id(Engine& engine, const std::string& path, uint64_t size) {
  return std::move(engine.generate_cas_ids({{path, size}})[0]);
}

Result<std::string> file_checksum(Engine& engine, const std::string& path) {
  return std::move(engine.file_checksums({path})[0]);
}

// ---- paths --------------------------------------------------------------------

std::string full_path(const Location& location, const FilePathRow& row) {
  // assemble_relative_path: materialized_path without its leading '/', then
  // name, then ".extension" for a file with a non-empty extension
  std::string rel = row.materialized_path.size() > 1 ? row.materialized_path.substr(1) : std::string();
  rel += row.name;
  if (!row.is_dir && !row.extension.empty()) rel += "." + row.extension;
  std::string base = location.path;
  if (!base.empty() && base.back() != '/') base += '/';
  return base + rel;
}

// ---- indexer walk ------------------------------------------------------------------

std::pair<std::string, std::optional<std::string>> file_stem_and_extension(const std::string& name) {
  // std::path's rsplit_file_at_dot: "..": no extension; the text before the
  // last dot empty (".bashrc"): no extension; else (before, after)
  if (name == "..") return {name, std::nullopt};
  const size_t dot = name.rfind('.');
  if (dot == std::string::npos) return {name, std::nullopt};
  if (dot == 0) return {name, std::nullopt};
  return {name.substr(0, dot), name.substr(dot + 1)};
}

std::vector<FilePathRow> walk_location(const Location& location, std::vector<IoError>* errors) {
  std::vector<FilePathRow> out;
  std::string root = location.path;
  while (root.size() > 1 && root.back() == '/') root.pop_back();
  std::vector<std::string> queue{""};  // relative directory paths, "" = the location itself
  for (size_t qi = 0; qi < queue.size(); ++qi) {
    const std::string rel = queue[qi];
    const std::string dir = rel.empty() ? root : root + "/" + rel;
    DIR* d = opendir(dir.c_str());
    if (!d) {
      if (errors) errors->push_back(IoError{errno, dir});
      continue;
    }
    std::vector<std::string> names;
    while (dirent* e = readdir(d)) {
      if (!std::strcmp(e->d_name, ".") || !std::strcmp(e->d_name, "..")) continue;
      names.emplace_back(e->d_name);
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    for (const auto& name : names) {
      const std::string full = dir + "/" + name;
      struct stat sb;
      if (lstat(full.c_str(), &sb) != 0) {
        if (errors) errors->push_back(IoError{errno, full});
        continue;
      }
      if (S_ISLNK(sb.st_mode)) continue;
      const bool is_dir = S_ISDIR(sb.st_mode);
      if (!is_dir && !S_ISREG(sb.st_mode)) continue;  // sockets, fifos, devices
      FilePathRow r;
      r.location_id = location.id;
      r.is_dir = is_dir;
      r.materialized_path = rel.empty() ? "/" : "/" + rel + "/";
      if (is_dir) {
        r.name = name;
      } else {
        auto [stem, ext] = file_stem_and_extension(name);
        r.name = stem;
        r.extension = ext.value_or("");
      }
      r.size_in_bytes = (uint64_t)sb.st_size;
      r.inode = (uint64_t)sb.st_ino;
      r.hidden = !name.empty() && name[0] == '.';
      r.date_created = (int64_t)sb.st_mtime;  // created_or_now(): birth time is not in struct stat
      out.push_back(std::move(r));
      if (is_dir) queue.push_back(rel.empty() ? name : rel + "/" + name);
    }
  }
  return out;
}

// ---- MemoryLibrary ------------------------------------------------------------------

// pub_ids in creation order: a tag, then the id big-endian in the last 8
// bytes, so that consecutive rows sort together (memcmp order) — the
// reference draws them at random (Uuid::new_v4, mod.rs:273), which is why it
// cannot be matched byte for byte, and an ordered id keeps the UNIQUE index
// on pub_id appending instead of inserting at random (as UUIDv7 does)
static PubId pub_id_of(uint32_t tag, int64_t id) {
  PubId p{};
  std::memcpy(p.data(), &tag, 4);
  for (int i = 0; i < 8; ++i) p[8 + i] = (uint8_t)((uint64_t)id >> (56 - 8 * i));
  return p;
}

FilePathRow& MemoryLibrary::add_file_path(FilePathRow row) {
  if (row.id == 0) row.id = next_file_path_id_;
  next_file_path_id_ = std::max(next_file_path_id_, row.id + 1);
  if (row.pub_id == PubId{}) row.pub_id = pub_id_of(0x46504154u, row.id);
  auto it = std::lower_bound(file_paths.begin(), file_paths.end(), row.id,
                             [](const FilePathRow& a, int32_t id) { return a.id < id; });
  if (it != file_paths.end() && it->id == row.id) throw std::invalid_argument("duplicate file_path id");
  return *file_paths.insert(it, std::move(row));
}

FilePathRow* MemoryLibrary::find(int32_t id) {
  auto it = std::lower_bound(file_paths.begin(), file_paths.end(), id,
                             [](const FilePathRow& a, int32_t v) { return a.id < v; });
  return it != file_paths.end() && it->id == id ? &*it : nullptr;
}

const FilePathRow* MemoryLibrary::file_path(int32_t id) const {
  return const_cast<MemoryLibrary*>(this)->find(id);
}

static bool under(const FilePathRow& r, const std::string& sub) {
  return sub.empty() || r.materialized_path.compare(0, sub.size(), sub) == 0;
}

bool MemoryLibrary::orphan(const FilePathRow& r, int32_t location_id, const std::string& sub) const {
  return (!r.object_id || !r.cas_id) && !r.is_dir && r.location_id == location_id && r.size_in_bytes != 0 &&
         under(r, sub);
}

size_t MemoryLibrary::count_orphan_file_paths(int32_t location_id, const std::string& sub) {
  return (size_t)std::count_if(file_paths.begin(), file_paths.end(),
                               [&](const FilePathRow& r) { return orphan(r, location_id, sub); });
}

std::vector<FilePathRow> MemoryLibrary::get_orphan_file_paths(int32_t location_id, int32_t cursor,
                                                              const std::string& sub, size_t take) {
  std::vector<FilePathRow> out;
  for (const auto& r : file_paths) {
    if (out.size() >= take) break;
    if (r.id >= cursor && orphan(r, location_id, sub)) out.push_back(r);
  }
  return out;
}

static bool orphan_in_dir(const FilePathRow& r, int32_t location_id, const std::string& dir) {
  return (!r.object_id || !r.cas_id) && !r.is_dir && r.location_id == location_id && r.size_in_bytes != 0 &&
         r.materialized_path == dir;
}

size_t MemoryLibrary::count_orphan_file_paths_in_dir(int32_t location_id, const std::string& dir) {
  return (size_t)std::count_if(file_paths.begin(), file_paths.end(),
                               [&](const FilePathRow& r) { return orphan_in_dir(r, location_id, dir); });
}

std::vector<FilePathRow> MemoryLibrary::get_orphan_file_paths_in_dir(int32_t location_id, int32_t cursor,
                                                                     const std::string& dir, size_t take) {
  std::vector<FilePathRow> out;
  for (const auto& r : file_paths) {
    if (out.size() >= take) break;
    if (r.id >= cursor && orphan_in_dir(r, location_id, dir)) out.push_back(r);
  }
  return out;
}

void MemoryLibrary::set_cas_id(int32_t id, const std::optional<std::string>& cas_id) {
  if (auto* r = find(id)) r->cas_id = cas_id;
}

std::vector<std::pair<int32_t, std::vector<std::string>>> MemoryLibrary::existing_objects(
    const std::vector<std::string>& cas_ids) {
  const std::set<std::string> want(cas_ids.begin(), cas_ids.end());
  std::map<int32_t, std::vector<std::string>> by_object;  // object id order = DB order
  std::set<int32_t> hit;
  for (const auto& r : file_paths) {
    if (!r.object_id) continue;
    if (r.cas_id && want.count(*r.cas_id)) hit.insert(*r.object_id);
  }
  for (const auto& r : file_paths)
    if (r.object_id && hit.count(*r.object_id) && r.cas_id) by_object[*r.object_id].push_back(*r.cas_id);
  return {by_object.begin(), by_object.end()};
}

std::vector<std::pair<std::string, int32_t>> Library::first_objects(const std::vector<std::string>& cas_ids) {
  const std::set<std::string> want(cas_ids.begin(), cas_ids.end());
  std::set<std::string> got;
  std::vector<std::pair<std::string, int32_t>> out;
  for (const auto& [oid, cs] : existing_objects(cas_ids))  // objects in DB order
    for (const auto& c : cs)
      if (want.count(c) && got.insert(c).second) out.emplace_back(c, oid);
  return out;
}

int32_t MemoryLibrary::create_object(ObjectKind kind, int64_t date_created) {
  ObjectRow o;
  o.id = next_object_id_++;
  o.pub_id = pub_id_of(0x4F424A54u, o.id);
  o.kind = kind;
  o.date_created = date_created;
  objects.push_back(o);
  return o.id;
}

void MemoryLibrary::connect(int32_t file_path_id, int32_t object_id) {
  if (auto* r = find(file_path_id)) r->object_id = object_id;
}

std::vector<FilePathRow> MemoryLibrary::file_paths_without_checksum(int32_t location_id, const std::string& sub) {
  std::vector<FilePathRow> out;
  for (const auto& r : file_paths)
    if (r.location_id == location_id && !r.is_dir && !r.integrity_checksum && under(r, sub)) out.push_back(r);
  return out;
}

void MemoryLibrary::set_integrity_checksum(int32_t id, const std::string& checksum) {
  if (auto* r = find(id)) r->integrity_checksum = checksum;
}

// ---- file_identifier ----------------------------------------------------------------

// SDCORE_DIRFD=0: the stat pass by full path (A/B)
static bool stat_dirfd() {
  static const bool on = [] {
    const char* v = getenv("SDCORE_DIRFD");
    return !(v && strcmp(v, "0") == 0);
  }();
  return on;
}

// SDCORE_FOLD_STAT=0: fs::metadata as its own fstatat pass before the cas_id
// reads (round 5) instead of inside them (sdcas_file_metadata) (A/B)
static bool fold_stat() {
  static const bool on = [] {
    const char* v = getenv("SDCORE_FOLD_STAT");
    return !(v && strcmp(v, "0") == 0);
  }();
  return on;
}

std::vector<Result<FileMetadata>> file_metadata_batch(Engine& engine,
                                                      const std::vector<std::pair<std::string, ObjectKind>>& files,
                                                      const std::vector<uint64_t>* size_hints) {
  return file_metadata_batch(engine, files, size_hints, false);
}

std::vector<Result<FileMetadata>> file_metadata_batch(Engine& engine,
                                                      const std::vector<std::pair<std::string, ObjectKind>>& files,
                                                      const std::vector<uint64_t>* size_hints, bool checksums) {
  const size_t n = files.size();
  if (size_hints && size_hints->size() != n) throw std::invalid_argument("file_metadata_batch: one size hint per file");
  if (checksums || fold_stat()) {
    // fs::metadata, the kind and generate_cas_id (mod.rs:63-86) in one library
    // call: the metadata is the fstat of the descriptor the reads use
    std::vector<const char*> paths(n);
    for (size_t i = 0; i < n; ++i) paths[i] = files[i].first.c_str();
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t* hints = size_hints ? size_hints->data() : nullptr;
    const Engine::RawMetadata raw = checksums ? engine.identify_checksums(paths, hints) : engine.file_metadata(paths, hints);
    static const bool trace = [] {
      const char* v = getenv("SDCORE_TRACE_JOB");
      return v && *v && strcmp(v, "0") != 0;
    }();
    const auto t1 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < n; ++i)
      if (raw.flags[i] & SDCAS_META_DIR)
        throw std::logic_error("We can't generate cas_id for directories");  // mod.rs:67-70
    // the results (the kind from the extension, the hex cas_id) on a few
    // threads for a big batch: this thread's part of the job's read-ahead
    std::vector<Result<FileMetadata>> out(n, Result<FileMetadata>(IoError{}));
    auto fill = [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        if (raw.status[i]) {
          out[i] = IoError{raw.status[i], files[i].first};
          continue;
        }
        FileMetadata m;
        m.kind = files[i].second >= 0 ? files[i].second : object_kind_of(files[i].first);  // mod.rs:72-76
        m.len = raw.size[i];
        if (raw.flags[i] & SDCAS_META_HAS_CAS_ID) m.cas_id = key_to_hex(raw.key[i]);
        if (raw.flags[i] & SDCAS_META_HAS_CHECKSUM) {
          char h[65];
          sdcas_digest_to_hex(&raw.digest[32 * i], h);
          m.integrity_checksum = std::string(h, 64);
        }
        out[i] = std::move(m);
      }
    };
    const size_t parts = std::min<size_t>(4, n / 2048 + 1);
    if (parts < 2) {
      fill(0, n);
    } else {
      std::vector<std::thread> th;
      for (size_t t = 1; t < parts; ++t) th.emplace_back(fill, n * t / parts, n * (t + 1) / parts);
      fill(0, n / parts);
      for (auto& x : th) x.join();
    }
    if (trace)
      fprintf(stderr, "sdcore file_metadata_batch: %zu files, sdcas_file_metadata %.2f ms, results %.2f ms\n", n,
              std::chrono::duration<double, std::milli>(t1 - t0).count(),
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    return out;
  }
  std::vector<std::optional<IoError>> err(n);
  std::vector<FileMetadata> md(n);
  std::vector<uint8_t> is_dir(n, 0);
  // fs::metadata and the kind per file (mod.rs:63-76), on up to 16 threads for
  // a big batch (the reference's join_all runs them concurrently too)
  // each file is stat'ed relative to its directory, whose descriptor a
  // thread keeps while consecutive files share it (one path component walked
  // instead of all; the library's readers open the same way, cas_io.cpp)
  auto stat_range = [&](size_t lo, size_t hi) {
    std::string dir;
    int dfd = -1;
    for (size_t i = lo; i < hi; ++i) {
      struct stat sb;
      const std::string& p = files[i].first;
      const size_t slash = p.rfind('/');
      int at = AT_FDCWD;
      const char* name = p.c_str();
      if (stat_dirfd() && slash != std::string::npos && slash > 0 && slash + 1 < p.size()) {
        if (dfd < 0 || dir.size() != slash || p.compare(0, slash, dir) != 0) {
          if (dfd >= 0) ::close(dfd);
          dir.assign(p, 0, slash);
          dfd = ::open(dir.c_str(), O_PATH | O_DIRECTORY | O_CLOEXEC);
        }
        if (dfd >= 0) {
          at = dfd;
          name = p.c_str() + slash + 1;
        }
      }
      if (::fstatat(at, name, &sb, 0) != 0) {  // fs::metadata (mod.rs:63-65)
        err[i] = IoError{errno, files[i].first};
        continue;
      }
      if (S_ISDIR(sb.st_mode)) {
        is_dir[i] = 1;
        continue;
      }
      md[i].kind = files[i].second >= 0 ? files[i].second : object_kind_of(files[i].first);  // mod.rs:72-76
      md[i].len = (uint64_t)sb.st_size;
    }
    if (dfd >= 0) ::close(dfd);
  };
  static const bool trace = [] {
    const char* v = getenv("SDCORE_TRACE_JOB");
    return v && *v && strcmp(v, "0") != 0;
  }();
  const auto t0 = std::chrono::steady_clock::now();
  const size_t threads = std::min<size_t>(16, n / 512);
  if (threads < 2) {
    stat_range(0, n);
  } else {
    std::vector<std::thread> pool;
    for (size_t t = 0; t < threads; ++t) pool.emplace_back(stat_range, n * t / threads, n * (t + 1) / threads);
    for (auto& th : pool) th.join();
  }
  std::vector<std::pair<std::string, uint64_t>> to_hash;
  std::vector<size_t> hashed_index;
  for (size_t i = 0; i < n; ++i) {
    if (is_dir[i]) throw std::logic_error("We can't generate cas_id for directories");  // mod.rs:67-70
    if (err[i]) continue;
    if (md[i].len != 0) {  // mod.rs:78-86: empty files get no cas_id
      to_hash.emplace_back(files[i].first, md[i].len);
      hashed_index.push_back(i);
    }
  }
  const auto t1 = std::chrono::steady_clock::now();
  auto cas = engine.generate_cas_ids(to_hash);
  if (trace)
    fprintf(stderr, "sdcore file_metadata_batch: %zu files, stat+kind %.2f ms, cas_ids %.2f ms\n", n,
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  for (size_t k = 0; k < cas.size(); ++k) {
    const size_t i = hashed_index[k];
    if (cas[k].ok()) md[i].cas_id = cas[k].value();
    else err[i] = cas[k].error();
  }
  std::vector<Result<FileMetadata>> out;
  out.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    if (err[i]) out.emplace_back(*err[i]);
    else out.emplace_back(std::move(md[i]));
  }
  return out;
}

static void flags_of(const std::vector<Result<FileMetadata>>& md, std::vector<uint8_t>& has_key,
                     std::vector<int32_t>& status) {
  const size_t n = md.size();
  has_key.assign(n, 0);
  status.assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    if (!md[i].ok()) status[i] = md[i].error().code;
    else has_key[i] = md[i].value().cas_id ? 1 : 0;
  }
}

StepPlan plan_steps(const std::vector<Result<FileMetadata>>& md, size_t chunk_size, sdcas_job_window& window) {
  std::vector<uint8_t> has_key;
  std::vector<int32_t> status;
  flags_of(md, has_key, status);
  StepPlan p;
  p.step.resize(md.size());
  p.reads.resize(md.size());
  const int rc =
      sdcas_job_plan(has_key.data(), status.data(), md.size(), chunk_size, &window, p.step.data(), p.reads.data());
  if (rc != SDCAS_OK) throw LibraryError(rc, "sdcas_job_plan");
  return p;
}

// a row to re-identify: an Object but no cas_id (the indexer nulled it when
// the file changed); writing its new cas_id makes its Object "existing" for
// that cas_id from its own step on (mod.rs:157-188)
static bool reidentified(const FilePathRow& r, const Result<FileMetadata>& md) {
  return r.object_id && !r.cas_id && md.ok() && md.value().cas_id;
}

// SDCORE_TRACE_JOB=1: where the identifier job's wall time goes, per phase
// of its main thread, summed over the job and printed to stderr at its end
// (a diagnostic; the phases of the read-ahead thread overlap them)
namespace {
struct JobTrace {
  enum { kMetadata, kWaitAhead, kFetch, kPlan, kCasWrites, kLookup, kGroupBy, kObjects, kIndex, kInit, kN };
  bool on = [] {
    const char* v = getenv("SDCORE_TRACE_JOB");
    return v && *v && strcmp(v, "0") != 0;
  }();
  double t[kN] = {};
  const std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now();
  std::chrono::steady_clock::time_point m = start;
  void mark() { m = std::chrono::steady_clock::now(); }
  void lap(int k) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    t[k] += std::chrono::duration<double>(now - m).count();
    m = now;
  }
  void print() const {
    if (!on) return;
    double sum = 0;
    for (double x : t) sum += x;
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    fprintf(stderr,
            "sdcore job trace s: metadata %.3f wait_ahead %.3f fetch %.3f plan %.3f cas_writes %.3f lookup %.3f "
            "group_by %.3f objects_links %.3f index %.3f init %.3f other %.3f wall %.3f\n",
            t[kMetadata], t[kWaitAhead], t[kFetch], t[kPlan], t[kCasWrites], t[kLookup], t[kGroupBy], t[kObjects],
            t[kIndex], t[kInit], wall - sum, wall);
  }
};
thread_local JobTrace* g_trace = nullptr;
void trace_lap(int k) {
  if (g_trace) g_trace->lap(k);
}
void trace_mark() {
  if (g_trace) g_trace->mark();
}
}  // namespace

// once the batch's steps are planned, before any of its writes: the job's
// loop starts reading its next batch there (run_steps)
using OnGrouped = std::function<void(const sdcas_job_window& done)>;

static std::pair<size_t, size_t> step_db(Library& db, const std::vector<FilePathRow>& file_paths,
                                         const std::vector<Result<FileMetadata>>& md, const GroupBy& group_by,
                                         sdcas_job_window* window, size_t chunk_size, const OnGrouped* on_grouped,
                                         const OnGrouped* after_group_by = nullptr,
                                         const OnGrouped* after_lookup = nullptr);

std::pair<size_t, size_t> identifier_step_db(Library& db, const std::vector<FilePathRow>& file_paths,
                                             const std::vector<Result<FileMetadata>>& md, const GroupBy& group_by,
                                             sdcas_job_window* window, size_t chunk_size) {
  return step_db(db, file_paths, md, group_by, window, chunk_size, nullptr);
}

static std::pair<size_t, size_t> step_db(Library& db, const std::vector<FilePathRow>& file_paths,
                                         const std::vector<Result<FileMetadata>>& md, const GroupBy& group_by,
                                         sdcas_job_window* window, size_t chunk_size, const OnGrouped* on_grouped,
                                         const OnGrouped* after_group_by, const OnGrouped* after_lookup) {
  const size_t n = file_paths.size();
  if (md.size() != n) throw std::invalid_argument("identifier_step_db: one metadata per file_path");
  sdcas_job_window win{};
  if (window) {
    win.max_steps = window->max_steps;
    win.more = window->more;
  }
  // which rows the steps read: only theirs are written (mod.rs:157-178)
  trace_mark();
  const StepPlan plan = plan_steps(md, chunk_size, win);
  const auto& step = plan.step;
  // the plan fixes which rows the steps read, so the job's read-ahead of its
  // next batch (rows past the last of them) starts now, beside this batch's
  // writes, lookup and group-by
  if (on_grouped) (*on_grouped)(win);
  trace_lap(JobTrace::kFetch);
  for (size_t i = 0; i < n; ++i)
    if (step[i] != UINT64_MAX && step[i] > 0 && reidentified(file_paths[i], md[i]))
      throw std::invalid_argument("identifier_step_db: a row to re-identify past the batch's first step");
  std::vector<uint64_t> keys(n, 0);
  std::vector<uint8_t> has_key(n, 0);
  std::vector<int32_t> status(n, 0);
  std::vector<std::string> unique;
  std::unordered_set<uint64_t> seen;  // by cas key: cas_ids are canonical 16-hex (cas.rs:61)
  seen.reserve(n);
  // cas_id writes (mod.rs:157-178): a row with an Object now, since the
  // lookup below can find its Object by it; a row without one together with
  // its link (set_cas_id_and_connect), the same end state in one write
  std::vector<uint8_t> cas_pending(n, 0);
  db.begin_batch();
  for (size_t i = 0; i < n; ++i) {
    if (!md[i].ok()) {
      status[i] = md[i].error().code;
      continue;
    }
    const auto& cas = md[i].value().cas_id;
    if (cas) {
      keys[i] = hex_to_key(*cas);
      has_key[i] = 1;
    }
    if (step[i] == UINT64_MAX) continue;  // no step reads it: it stays as it is
    if (cas && seen.insert(keys[i]).second) unique.push_back(*cas);
    if (file_paths[i].object_id) db.set_cas_id(file_paths[i].id, cas);
    else cas_pending[i] = 1;
  }
  db.end_batch();
  trace_lap(JobTrace::kCasWrites);
  // the first existing Object carrying each cas_id, DB order (mod.rs:181-188
  // and the find of :214-224): one existing-key entry per cas_id
  std::vector<uint64_t> ekeys;
  std::vector<int32_t> eobj;
  for (const auto& [c, oid] : db.first_objects(unique)) {
    ekeys.push_back(hex_to_key(c));
    eobj.push_back(oid);
  }
  trace_lap(JobTrace::kLookup);
  // (or here: the chunked loop's read-ahead beside the group-by and the
  // writes, not beside the lookup's index probes)
  if (after_lookup) (*after_lookup)(win);
  sdcas_job_window gw{};
  gw.max_steps = win.max_steps;
  gw.more = win.more;
  auto d = group_by(keys, has_key, status, ekeys, gw);
  trace_lap(JobTrace::kGroupBy);
  // (the chunked loop's read-ahead starts here: its FileMetadata call would
  // otherwise hold the engine while this batch's group-by waits for it)
  if (after_group_by) (*after_group_by)(win);
  if (d.link.size() != n) throw std::logic_error("identifier_step_db: group-by returned a wrong link count");
  if (gw.steps != win.steps || gw.rows != win.rows)
    throw std::logic_error("identifier_step_db: the group-by ran other steps than the plan");
  // new Objects (mod.rs:246-342) in the order the steps create them: step by
  // step, rows in id order within a step; a row without cas_id that several
  // steps read gets an Object from each, the last one its link. They take
  // the kind and date_created of their file (mod.rs:266-291).
  std::vector<std::pair<uint64_t, size_t>> creates;
  for (size_t i = 0; i < n; ++i)
    if (d.link[i] == (int64_t)i)
      for (uint32_t r = 0; r < plan.reads[i]; ++r) creates.emplace_back(plan.step[i] + r, i);
  std::stable_sort(creates.begin(), creates.end(),
                   [](const std::pair<uint64_t, size_t>& a, const std::pair<uint64_t, size_t>& b) {
                     return a.first < b.first;
                   });
  // each row's last link: a row several steps read links to the Object of
  // the last (creates are in step order); 0 = not linked
  std::vector<int32_t> created_object(n, 0), link_to(n, 0);
  db.begin_batch();
  {
    // object::create_many (mod.rs:314-327), then the links of :331-342
    std::vector<std::pair<ObjectKind, int64_t>> kd;
    kd.reserve(creates.size());
    for (const auto& [s, i] : creates) kd.emplace_back(md[i].value().kind, file_paths[i].date_created);
    const std::vector<int32_t> oids = db.create_objects(kd);
    if (oids.size() != creates.size()) throw std::logic_error("identifier_step_db: create_objects returned a wrong count");
    for (size_t k = 0; k < creates.size(); ++k) {
      const size_t i = creates[k].second;
      created_object[i] = link_to[i] = oids[k];
    }
  }
  // links to the first Object carrying the cas_id (mod.rs:202-238)
  for (size_t i = 0; i < n; ++i) {
    const int64_t l = d.link[i];
    if (l == SDCAS_LINK_DROPPED || l == SDCAS_LINK_DEFERRED || l == (int64_t)i) continue;
    link_to[i] = l >= 0 ? created_object[(size_t)l] : eobj[(size_t)(-(l + 1))];
  }
  // one write per row, in row order: a row without an Object takes its
  // cas_id and its link together (set_cas_ids_and_connect), a row with one
  // its link (connect); a row read but not linked its cas_id (none such today)
  std::vector<Library::CasLink> writes;
  writes.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    if (link_to[i] && cas_pending[i]) writes.push_back({file_paths[i].id, md[i].value().cas_id, link_to[i]});
    else if (link_to[i]) db.connect(file_paths[i].id, link_to[i]);
    else if (cas_pending[i]) db.set_cas_id(file_paths[i].id, md[i].value().cas_id);
  }
  // SDCORE_LINKS=each: the rows one statement each (A/B)
  static const bool each = [] {
    const char* v = getenv("SDCORE_LINKS");
    return v && !strcmp(v, "each");
  }();
  if (each) db.Library::set_cas_ids_and_connect(writes);
  else db.set_cas_ids_and_connect(writes);
  // the checksum of the same read (FileIdentifierJobInit::checksums): every
  // row the steps read, after its cas_id write
  for (size_t i = 0; i < n; ++i)
    if (step[i] != UINT64_MAX && md[i].ok() && md[i].value().integrity_checksum)
      db.set_integrity_checksum(file_paths[i].id, *md[i].value().integrity_checksum);
  db.end_batch();
  trace_lap(JobTrace::kObjects);
  if (window) *window = win;
  return {(size_t)d.created, (size_t)d.linked};
}
std::pair<size_t, size_t> identifier_job_step(Engine& engine, Library& db, const Location& location,
                                              const std::vector<FilePathRow>& file_paths, size_t chunk_size,
                                              sdcas_job_window* window) {
  const size_t n = file_paths.size();
  std::vector<std::pair<std::string, ObjectKind>> files(n);
  std::vector<uint64_t> hints(n);
  for (size_t i = 0; i < n; ++i) {
    files[i] = {full_path(location, file_paths[i]), file_paths[i].kind};
    hints[i] = file_paths[i].size_in_bytes;
  }
  // FileMetadata::new for every row (mod.rs:105-147): failing files are
  // logged and left out of the rest of the step (mod.rs:125-141)
  auto md = file_metadata_batch(engine, files, &hints);
  return identifier_step_db(
      db, file_paths, md,
      [&](const std::vector<uint64_t>& k, const std::vector<uint8_t>& h, const std::vector<int32_t>& st,
          const std::vector<uint64_t>& e, sdcas_job_window& w) { return engine.dedup(k, h, st, chunk_size, e, &w); },
      window, chunk_size);
}

namespace {
// The steps of the identifier over its orphans, `batch` rows per fetch
// (file_identifier_job.rs:180-236 and shallow.rs:92-112 share it): each batch
// runs as many of the job's 100-row steps as it holds (identifier_step_db),
// and the cursor moves to the last row they read (mod.rs:401-405).
struct StepLoop {
  size_t created = 0, linked = 0, steps = 0, batches = 0, rereads = 0;
  int32_t cursor = 0;
  bool ran_dry = false;  // a fetch found no rows
};
using Fetch = std::function<std::vector<FilePathRow>(int32_t cursor, size_t take)>;

// Round 6: the orphans read ahead in chunks on the read-ahead connection by a
// thread of their own, `batch` rows past the last row read so far, up to two
// chunks ahead. Rows past the job's cursor are never written by the batch
// that fetched them (its steps write only the rows they read, all at or
// before the cursor), so a chunk fetched before a batch's writes is what a
// fetch after them would return.
class ChunkFetcher {
 public:
  struct Chunk {
    std::vector<FilePathRow> rows;
    bool full = false;  // `take` rows: more may follow
    std::exception_ptr err;
  };
  ChunkFetcher(const Fetch& fetch, int32_t after, size_t take) : fetch_(fetch), after_(after), take_(take) {
    th_ = std::thread([this] { loop(); });
  }
  ~ChunkFetcher() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  // the next chunk (empty rows: none left), in id order
  Chunk next() {
    std::unique_lock<std::mutex> g(m_);
    cv_.wait(g, [this] { return !q_.empty(); });
    Chunk c = std::move(q_.front());
    q_.pop_front();
    cv_.notify_all();
    return c;
  }

 private:
  static constexpr size_t kDepth = 2;
  void loop() {
    for (;;) {
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return stop_ || q_.size() < kDepth; });
        if (stop_) return;
      }
      Chunk c;
      try {
        c.rows = fetch_(after_ + 1, take_);  // id >= after + 1 ORDER BY id
        c.full = c.rows.size() == take_;
        if (!c.rows.empty()) after_ = c.rows.back().id;
      } catch (...) {
        c.err = std::current_exception();
      }
      const bool last = c.err || !c.full;
      {
        std::lock_guard<std::mutex> g(m_);
        q_.push_back(std::move(c));
      }
      cv_.notify_all();
      if (last) return;
    }
  }
  const Fetch& fetch_;
  int32_t after_;
  const size_t take_;
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<Chunk> q_;
  bool stop_ = false;
  std::thread th_;
};

// SDCORE_PIPELINE=0: round 5's loop (the next batch fetched after the plan,
// on the same thread as its FileMetadata) (A/B)
static bool pipeline_enabled() {
  static const bool on = [] {
    const char* v = getenv("SDCORE_PIPELINE");
    return !(v && strcmp(v, "0") == 0);
  }();
  return on;
}

// Where the chunked loop's read-ahead FileMetadata starts in a batch
// (SDCORE_AHEAD_AT): "lookup" (the default) after the existing-Object
// lookup — beside the group-by (its own context, Engine::dedup_ctx, so the
// read-ahead's path call does not hold it up) and the writes, but not beside
// the lookup's index probes, which it slowed (10 000-row batches without bulk
// identify 316 -> 240-280 K orphans/s at "plan"); "plan" at the plan; "groupby"
// after the group-by (A/B)
enum AheadAt { kAheadPlan, kAheadLookup, kAheadGroupBy };
static AheadAt ahead_at() {
  static const AheadAt at = [] {
    const char* v = getenv("SDCORE_AHEAD_AT");
    if (v && strcmp(v, "plan") == 0) return kAheadPlan;
    if (v && strcmp(v, "groupby") == 0) return kAheadGroupBy;
    return kAheadLookup;
  }();
  return at;
}

// The step loop with the chunk fetcher: each batch is the cursor row when it
// stays an orphan (fetched again after the writes: its Object may be new),
// then the rows the batch fetched but its steps did not read, then the next
// chunk, whose FileMetadata runs beside this batch's writes (as round 5's
// read-ahead) but no longer waits for its own fetch.
StepLoop run_steps_chunked(Library& db, uint64_t task_count, int32_t cursor, size_t batch_rows, const Fetch& fetch,
                           const MetadataFn& metadata, const GroupBy& group_by, const Fetch& fetch_ahead) {
  StepLoop L;
  L.cursor = cursor;
  const size_t cs = SDCAS_IDENTIFIER_CHUNK_SIZE;
  const size_t batch = std::max(cs, batch_rows);
  uint64_t steps_left = task_count;
  trace_mark();
  // a short first batch: the pipeline's fill is its FileMetadata alone (the
  // next chunk's runs while it is written)
  const size_t first_take = batch >= 8 * cs ? std::max(cs, batch / 8) : batch;
  std::vector<FilePathRow> rows = fetch(L.cursor, first_take);  // id >= cursor ORDER BY id (file_identifier_job.rs:296-319)
  trace_lap(JobTrace::kFetch);
  bool more = rows.size() == first_take;
  std::unique_ptr<ChunkFetcher> fetcher;
  if (more) fetcher = std::make_unique<ChunkFetcher>(fetch_ahead, rows.back().id, batch);
  trace_mark();
  std::vector<Result<FileMetadata>> md = metadata(rows);
  trace_lap(JobTrace::kMetadata);
  struct Ahead {
    ChunkFetcher::Chunk chunk;
    std::vector<Result<FileMetadata>> md;
  };
  while (steps_left) {
    if (rows.empty()) {
      L.ran_dry = true;
      break;
    }
    if (L.batches && rows[0].id == L.cursor) ++L.rereads;  // the cursor row is still an orphan
    sdcas_job_window w{};
    w.max_steps = steps_left;
    w.more = more;
    // a row to re-identify must sit in the batch's first step (identifier_step_db)
    {
      sdcas_job_window probe = w;
      const StepPlan plan = plan_steps(md, cs, probe);
      uint64_t cut = UINT64_MAX;
      for (size_t i = 0; i < rows.size(); ++i)
        if (plan.step[i] != UINT64_MAX && plan.step[i] > 0 && reidentified(rows[i], md[i]))
          cut = std::min(cut, plan.step[i]);
      if (cut != UINT64_MAX) w.max_steps = cut;
    }
    std::future<Ahead> next_md;
    const OnGrouped start_next = [&](const sdcas_job_window& done) {
      if (done.steps == 0 || done.steps >= steps_left || !fetcher) return;
      ChunkFetcher* f = fetcher.get();
      next_md = std::async(std::launch::async, [f, &metadata] {
        Ahead a;
        a.chunk = f->next();
        if (!a.chunk.err && !a.chunk.rows.empty()) a.md = metadata(a.chunk.rows);
        return a;
      });
    };
    const AheadAt at = ahead_at();
    auto [created, linked] = step_db(db, rows, md, group_by, &w, cs, at == kAheadPlan ? &start_next : nullptr,
                                     at == kAheadGroupBy ? &start_next : nullptr,
                                     at == kAheadLookup ? &start_next : nullptr);
    if (w.steps == 0) break;  // cannot happen: a batch of >= cs rows holds a whole step
    L.created += created;
    L.linked += linked;
    L.steps += w.steps;
    L.rereads += w.rereads;
    ++L.batches;
    steps_left -= std::min<uint64_t>(steps_left, w.steps);
    const size_t last = w.rows - 1;
    L.cursor = rows[last].id;
    if (!steps_left) break;
    // the next batch: the cursor row again if it stays an orphan, the rows
    // past it, the next chunk
    std::vector<FilePathRow> nrows;
    std::vector<Result<FileMetadata>> nmd;
    trace_mark();
    if (!md[last].ok() || !md[last].value().cas_id) {
      std::vector<FilePathRow> cur = fetch(L.cursor, 1);
      if (cur.size() == 1 && cur[0].id == L.cursor) {
        nrows.push_back(std::move(cur[0]));
        nmd.push_back(md[last]);  // the same file: its FileMetadata as this batch read it
      }
    }
    trace_lap(JobTrace::kFetch);
    for (size_t i = w.rows; i < rows.size(); ++i) {
      nrows.push_back(std::move(rows[i]));
      nmd.push_back(std::move(md[i]));
    }
    if (next_md.valid()) {
      trace_mark();
      Ahead a = next_md.get();
      trace_lap(JobTrace::kWaitAhead);
      if (a.chunk.err) std::rethrow_exception(a.chunk.err);
      more = a.chunk.full;
      if (!more) fetcher.reset();  // the fetcher has ended
      for (size_t i = 0; i < a.chunk.rows.size(); ++i) {
        nrows.push_back(std::move(a.chunk.rows[i]));
        nmd.push_back(std::move(a.md[i]));
      }
    } else if (!fetcher) {
      more = false;
    }
    rows = std::move(nrows);
    md = std::move(nmd);
  }
  return L;
}

StepLoop run_steps(Library& db, uint64_t task_count, int32_t cursor, size_t batch_rows, const Fetch& fetch,
                   const MetadataFn& metadata, const GroupBy& group_by, const Fetch* fetch_ahead = nullptr) {
  if (fetch_ahead && pipeline_enabled())
    return run_steps_chunked(db, task_count, cursor, batch_rows, fetch, metadata, group_by, *fetch_ahead);
  StepLoop L;
  L.cursor = cursor;
  const size_t cs = SDCAS_IDENTIFIER_CHUNK_SIZE;
  const size_t batch = std::max(cs, batch_rows);  // a batch holds at least one whole step
  uint64_t steps_left = task_count;
  std::vector<FilePathRow> rows = fetch(L.cursor, batch);  // id >= cursor ORDER BY id (file_identifier_job.rs:296-319)
  std::vector<Result<FileMetadata>> md;
  bool have_md = false;
  while (steps_left) {
    if (rows.empty()) {
      L.ran_dry = true;
      break;
    }
    trace_mark();
    if (!have_md) md = metadata(rows);
    trace_lap(JobTrace::kMetadata);
    if (L.batches && rows[0].id == L.cursor) ++L.rereads;  // the cursor row is still an orphan
    sdcas_job_window w{};
    w.max_steps = steps_left;
    w.more = rows.size() == batch;
    // a row to re-identify must sit in the batch's first step (identifier_step_db)
    {
      sdcas_job_window probe = w;
      const StepPlan plan = plan_steps(md, cs, probe);
      uint64_t cut = UINT64_MAX;
      for (size_t i = 0; i < rows.size(); ++i)
        if (plan.step[i] != UINT64_MAX && plan.step[i] > 0 && reidentified(rows[i], md[i]))
          cut = std::min(cut, plan.step[i]);
      if (cut != UINT64_MAX) w.max_steps = cut;
    }
    // The next batch is read while this one's Objects are written: the next
    // fetch (id >= the cursor) is the cursor row if it stays an orphan (an
    // error or no cas_id: nothing makes it whole) and then orphans past the
    // cursor, which this batch does not write. Those are fetched and their
    // FileMetadata computed on another thread after the group-by; the cursor
    // row is fetched again once the writes are done.
    std::vector<FilePathRow> next;
    using Ahead = std::pair<std::vector<FilePathRow>, std::vector<Result<FileMetadata>>>;
    std::future<Ahead> next_md;
    bool stays = false;
    int32_t next_cursor = 0;
    const OnGrouped prefetch = [&](const sdcas_job_window& done) {
      if (done.steps == 0 || done.steps >= steps_left) return;
      const size_t last = done.rows - 1;
      next_cursor = rows[last].id;
      stays = !md[last].ok() || !md[last].value().cas_id;
      std::vector<FilePathRow> head;
      if (stays) head.push_back(rows[last]);  // the same file; its row is re-read below
      const size_t take = batch - (stays ? 1 : 0);
      if (fetch_ahead) {
        // the fetch too runs beside this batch's writes (a second connection)
        next_md = std::async(std::launch::async, [&metadata, fetch_ahead, head = std::move(head), next_cursor, take] {
          Ahead a;
          a.first = (*fetch_ahead)(next_cursor + 1, take);
          std::vector<FilePathRow> ahead = head;
          ahead.insert(ahead.end(), a.first.begin(), a.first.end());
          if (!ahead.empty()) a.second = metadata(ahead);
          return a;
        });
        return;
      }
      next = fetch(next_cursor + 1, take);
      std::vector<FilePathRow> ahead = std::move(head);
      ahead.insert(ahead.end(), next.begin(), next.end());
      if (ahead.empty()) return;
      next_md = std::async(std::launch::async, [&metadata, ahead = std::move(ahead)] {
        return Ahead{{}, metadata(ahead)};
      });
    };
    auto [created, linked] = step_db(db, rows, md, group_by, &w, cs, &prefetch);
    if (w.steps == 0) break;  // cannot happen: a batch of `batch` >= cs rows holds a whole step
    L.created += created;
    L.linked += linked;
    L.steps += w.steps;
    L.rereads += w.rereads;
    ++L.batches;
    steps_left -= std::min<uint64_t>(steps_left, w.steps);
    L.cursor = rows[w.rows - 1].id;
    have_md = false;
    if (next_md.valid()) {
      trace_mark();
      Ahead got = next_md.get();
      trace_lap(JobTrace::kWaitAhead);
      if (fetch_ahead) next = std::move(got.first);
      auto ahead_md = std::move(got.second);
      if (ahead_md.empty()) {  // nothing past the cursor, nor a cursor row to read again
        if (steps_left) rows = fetch(L.cursor, batch);
        continue;
      }
      std::vector<FilePathRow> cur;
      if (stays) cur = fetch(L.cursor, 1);
      if (!stays || (cur.size() == 1 && cur[0].id == L.cursor)) {
        rows = std::move(cur);
        rows.insert(rows.end(), next.begin(), next.end());
        md = std::move(ahead_md);
        have_md = true;
        continue;
      }
    }
    trace_mark();
    if (steps_left) rows = fetch(L.cursor, batch);
    trace_lap(JobTrace::kFetch);
  }
  return L;
}
}  // namespace

FileIdentifierJobRunMetadata run_file_identifier_job_with(Library& db, const FileIdentifierJobInit& init,
                                                          const MetadataFn& metadata, const GroupBy& group_by) {
  FileIdentifierJobRunMetadata meta;
  const int32_t loc = init.location.id;
  const std::string& sub = init.sub_materialized_path;
  JobTrace trace;
  // init (file_identifier_job.rs:125-176)
  meta.total_orphan_paths = db.count_orphan_file_paths(loc, sub);
  if (meta.total_orphan_paths == 0) return meta;
  auto first = db.get_orphan_file_paths(loc, 0, sub, 1);
  meta.cursor = first.empty() ? 0 : first[0].id;
  const uint64_t task_count = (meta.total_orphan_paths + SDCAS_IDENTIFIER_CHUNK_SIZE - 1) / SDCAS_IDENTIFIER_CHUNK_SIZE;
  struct TraceScope {
    JobTrace* t;
    explicit TraceScope(JobTrace* x) : t(x) { g_trace = x->on ? x : nullptr; }
    ~TraceScope() {
      t->print();
      g_trace = nullptr;
    }
  } trace_scope(&trace);
  // the lookup index traded for a host map for the job's duration, restored
  // on every way out (Library::begin_bulk_identify)
  struct Bulk {
    Library& db;
    bool on;
    ~Bulk() {
      if (!on) return;
      trace_mark();
      try {
        db.end_bulk_identify();
        trace_lap(JobTrace::kIndex);
      } catch (...) {  // unwinding already; the index is rebuilt by the next bulk job or existing_objects
      }
    }
  } bulk{db, init.bulk_identify && db.begin_bulk_identify(meta.total_orphan_paths)};
  meta.bulk_identify = bulk.on;
  const Fetch ahead = [&](int32_t cursor, size_t take) {
    return db.get_orphan_file_paths_concurrent(loc, cursor, sub, take);
  };
  const bool concurrent = db.concurrent_orphan_reads();
  trace.lap(JobTrace::kInit);
  // without `checksums` the job writes none: a metadata function's are dropped
  const MetadataFn no_checksums = [&](const std::vector<FilePathRow>& rows) {
    auto md = metadata(rows);
    for (auto& m : md)
      if (m.ok() && m.value().integrity_checksum) {
        FileMetadata v = m.value();
        v.integrity_checksum.reset();
        m = std::move(v);
      }
    return md;
  };
  const StepLoop L = run_steps(
      db, task_count, meta.cursor, init.batch,
      [&](int32_t cursor, size_t take) { return db.get_orphan_file_paths(loc, cursor, sub, take); },
      init.checksums ? metadata : no_checksums, group_by, concurrent ? &ahead : nullptr);
  meta.total_objects_created = L.created;
  meta.total_objects_linked = L.linked;
  meta.steps = L.steps;
  meta.batches = L.batches;
  meta.rereads = L.rereads;
  meta.cursor = L.cursor;
  meta.early_finish = L.ran_dry;  // EarlyFinish (:203-209)
  return meta;
}

ShallowIdentifierReport shallow_file_identifier_with(Library& db, const Location& location, const std::string& dir,
                                                     size_t batch, const MetadataFn& metadata,
                                                     const GroupBy& group_by) {
  ShallowIdentifierReport rep;
  const std::string d = dir.empty() ? "/" : dir;  // materialized_path_for_children of the root
  rep.orphans = db.count_orphan_file_paths_in_dir(location.id, d);  // shallow.rs:62-66
  if (rep.orphans == 0) return rep;
  // find_first without ordering (shallow.rs:74-84): the lowest orphan id
  auto first = db.get_orphan_file_paths_in_dir(location.id, 0, d, 1);
  if (first.empty()) return rep;  // "another Job finishing first" (shallow.rs:81-83)
  const uint64_t task_count = (rep.orphans + SDCAS_IDENTIFIER_CHUNK_SIZE - 1) / SDCAS_IDENTIFIER_CHUNK_SIZE;
  // every step runs (shallow.rs:92-112): one that finds no rows changes
  // nothing, so the loop may stop at the first empty fetch
  const StepLoop L = run_steps(
      db, task_count, first[0].id, batch,
      [&](int32_t cursor, size_t take) { return db.get_orphan_file_paths_in_dir(location.id, cursor, d, take); },
      metadata, group_by);
  rep.steps = L.steps;
  rep.batches = L.batches;
  rep.rereads = L.rereads;
  rep.created = L.created;
  rep.linked = L.linked;
  rep.cursor = L.cursor;
  return rep;
}

static std::vector<Result<FileMetadata>> metadata_of(Engine& engine, const Location& location,
                                                     const std::vector<FilePathRow>& rows, bool checksums = false) {
  std::vector<std::pair<std::string, ObjectKind>> files(rows.size());
  std::vector<uint64_t> hints(rows.size());
  for (size_t i = 0; i < rows.size(); ++i) {
    files[i] = {full_path(location, rows[i]), rows[i].kind};
    hints[i] = rows[i].size_in_bytes;
  }
  return file_metadata_batch(engine, files, &hints, checksums);
}

static GroupBy gpu_group_by(Engine& engine) {
  return [&engine](const std::vector<uint64_t>& k, const std::vector<uint8_t>& h, const std::vector<int32_t>& st,
                   const std::vector<uint64_t>& e, sdcas_job_window& w) {
    return engine.dedup(k, h, st, SDCAS_IDENTIFIER_CHUNK_SIZE, e, &w);
  };
}

ShallowIdentifierReport shallow_file_identifier(Engine& engine, Library& db, const Location& location,
                                                const std::string& dir, size_t batch) {
  return shallow_file_identifier_with(
      db, location, dir, batch, [&](const std::vector<FilePathRow>& rows) { return metadata_of(engine, location, rows); },
      gpu_group_by(engine));
}

FileIdentifierJobRunMetadata run_file_identifier_job(Engine& engine, Library& db, const FileIdentifierJobInit& init) {
  const FileIdentifierJobRunMetadata meta = run_file_identifier_job_with(
      db, init,
      [&](const std::vector<FilePathRow>& rows) { return metadata_of(engine, init.location, rows, init.checksums); },
      gpu_group_by(engine));
  if (!init.checksums) return meta;
  // Files the indexer saw empty are never orphans (size_in_bytes != 0 in the
  // filter of file_identifier_job.rs:251-278), so no step reads them, while
  // the validator hashes them like any file: they get their checksum here,
  // from the validator's own call. A file that fails keeps none.
  std::vector<FilePathRow> rest;
  for (auto& r : db.file_paths_without_checksum(init.location.id, init.sub_materialized_path))
    if (r.size_in_bytes == 0) rest.push_back(std::move(r));
  const size_t batch = std::max<size_t>(1, init.batch);
  for (size_t lo = 0; lo < rest.size(); lo += batch) {
    const size_t hi = std::min(rest.size(), lo + batch);
    std::vector<std::string> paths;
    for (size_t i = lo; i < hi; ++i) paths.push_back(full_path(init.location, rest[i]));
    const auto sums = engine.file_checksums(paths);
    db.begin_batch();
    for (size_t i = lo; i < hi; ++i)
      if (sums[i - lo].ok()) db.set_integrity_checksum(rest[i].id, sums[i - lo].value());
    db.end_batch();
  }
  return meta;
}

// ---- object validator -----------------------------------------------------------------

ObjectValidatorReport run_object_validator_job(Engine& engine, Library& db, const ObjectValidatorJobInit& init) {
  ObjectValidatorReport rep;
  auto rows = db.file_paths_without_checksum(init.location.id, init.sub_materialized_path);
  rep.task_count = rows.size();
  const size_t batch = std::max<size_t>(1, init.batch);
  for (size_t lo = 0; lo < rows.size(); lo += batch) {
    const size_t hi = std::min(rows.size(), lo + batch);
    std::vector<std::string> paths;
    for (size_t i = lo; i < hi; ++i) paths.push_back(full_path(init.location, rows[i]));
    auto sums = engine.file_checksums(paths);
    db.begin_batch();
    for (size_t i = lo; i < hi; ++i) {
      const auto& r = sums[i - lo];
      if (!r.ok()) {  // validator_job.rs:154-156: the step fails with FileIO
        rep.error = r.error();
        db.end_batch();
        return rep;
      }
      db.set_integrity_checksum(rows[i].id, r.value());  // validator_job.rs:158-172
      ++rep.checksummed;
    }
    db.end_batch();
  }
  return rep;
}

// ---- duplicates confirmed by checksum -----------------------------------------------

static int hex_nibble(char ch) {
  if (ch >= '0' && ch <= '9') return ch - '0';
  if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
  if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
  return -1;
}

// `bytes` bytes from 2 * bytes hex characters; false when s is anything else
static bool hex_to_bytes(const std::string& s, uint8_t* out, size_t bytes) {
  if (s.size() != 2 * bytes) return false;
  for (size_t i = 0; i < bytes; ++i) {
    const int hi = hex_nibble(s[2 * i]), lo = hex_nibble(s[2 * i + 1]);
    if (hi < 0 || lo < 0) return false;
    out[i] = (uint8_t)(hi << 4 | lo);
  }
  return true;
}

DuplicateReport duplicate_report_from(const std::vector<FilePathRow>& rows, const std::vector<int64_t>& rep,
                                      const std::vector<int64_t>& key_rep, const std::vector<uint8_t>& flags) {
  const size_t n = rows.size();
  if (rep.size() != n || key_rep.size() != n || flags.size() != n)
    throw std::invalid_argument("duplicate_report_from: rows / rep / key_rep / flags lengths differ");
  DuplicateReport out;
  // rows come in id order, so a class's (key's) lowest file is its first row
  // and walking the rows in order gives every list ascending
  std::vector<std::vector<int32_t>> members(n);  // at a class's first row: its rows
  std::vector<std::vector<size_t>> classes(n);   // at a collided key's first row: its classes' first rows
  for (size_t i = 0; i < n; ++i) {
    if (flags[i] & SDCAS_CONFIRM_SKIPPED) continue;
    if (rep[i] < 0 || (size_t)rep[i] > i || key_rep[i] < 0 || key_rep[i] > rep[i])
      throw std::invalid_argument("duplicate_report_from: row " + std::to_string(i) + " has no valid rep");
    const bool collided = flags[i] & SDCAS_CONFIRM_COLLISION;
    ++out.counts.files;
    out.counts.classes += (size_t)rep[i] == i;
    out.counts.keys += (size_t)key_rep[i] == i;
    out.counts.collided_keys += (size_t)key_rep[i] == i && collided;
    out.counts.collided_files += collided;
    out.counts.duplicate_files += (size_t)rep[i] != i;
    members[(size_t)rep[i]].push_back(rows[i].id);
    if (collided && (size_t)rep[i] == i) classes[(size_t)key_rep[i]].push_back(i);
  }
  for (size_t i = 0; i < n; ++i) {
    if (members[i].size() >= 2)
      out.confirmed.push_back({rows[i].cas_id.value_or(""), rows[i].integrity_checksum.value_or(""), members[i]});
    if (classes[i].empty()) continue;
    DuplicateReport::Collision c;
    c.cas_id = rows[i].cas_id.value_or("");
    for (size_t first : classes[i]) c.classes.push_back(members[first]);
    out.collisions.push_back(std::move(c));
  }
  // the Objects the cas-only link merged each collided cas_id's rows into
  std::vector<std::set<int32_t>> objects(n);
  for (size_t i = 0; i < n; ++i)
    if (!(flags[i] & SDCAS_CONFIRM_SKIPPED) && (flags[i] & SDCAS_CONFIRM_COLLISION) && rows[i].object_id)
      objects[(size_t)key_rep[i]].insert(*rows[i].object_id);
  size_t next = 0;
  for (size_t i = 0; i < n; ++i)
    if (!classes[i].empty()) out.collisions[next++].object_ids.assign(objects[i].begin(), objects[i].end());
  return out;
}

Engine::Confirm Engine::confirm_duplicates(const std::vector<uint64_t>& keys, const std::vector<uint8_t>& digests,
                                           const std::vector<uint8_t>& valid) {
  const size_t n = keys.size();
  if (digests.size() != 32 * n || (!valid.empty() && valid.size() != n))
    throw std::invalid_argument("confirm_duplicates: keys / digests / valid lengths differ");
  Confirm r;
  r.rep.assign(n, 0);
  r.key_rep.assign(n, 0);
  r.flags.assign(n, 0);
  const int rc = sdcas_confirm_duplicates(ctx_, keys.data(), digests.data(), valid.empty() ? nullptr : valid.data(), n,
                                          r.rep.data(), r.key_rep.data(), r.flags.data(), &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_confirm_duplicates");
  return r;
}

std::vector<FilePathRow> Library::file_paths_with_checksum(int32_t, const std::string&) {
  throw LibraryError(SDCAS_E_INVALID, "this Library does not implement file_paths_with_checksum");
}

std::vector<FilePathRow> MemoryLibrary::file_paths_with_checksum(int32_t location_id, const std::string& sub) {
  std::vector<FilePathRow> out;
  for (const auto& r : file_paths)
    if (r.location_id == location_id && !r.is_dir && r.cas_id && r.integrity_checksum && under(r, sub))
      out.push_back(r);
  return out;
}

DuplicateReport confirm_duplicates(Engine& engine, Library& db, int32_t location_id, const std::string& sub) {
  const std::vector<FilePathRow> rows = db.file_paths_with_checksum(location_id, sub);
  const size_t n = rows.size();
  std::vector<uint64_t> keys(n, 0);
  std::vector<uint8_t> digests(32 * n, 0), valid(n, 0);
  for (size_t i = 0; i < n; ++i) {
    uint8_t k[8];
    if (!rows[i].cas_id || !rows[i].integrity_checksum || !hex_to_bytes(*rows[i].cas_id, k, 8) ||
        !hex_to_bytes(*rows[i].integrity_checksum, &digests[32 * i], 32))
      continue;
    keys[i] = hex_to_key(*rows[i].cas_id);
    valid[i] = 1;
  }
  const Engine::Confirm c = engine.confirm_duplicates(keys, digests, valid);
  DuplicateReport out = duplicate_report_from(rows, c.rep, c.key_rep, c.flags);
  out.counts = c.counts;
  return out;
}

Engine::Sets Engine::duplicate_sets(const std::vector<int64_t>& rep, const std::vector<uint64_t>& sizes,
                                    uint32_t order) {
  const size_t n = rep.size();
  if (!sizes.empty() && sizes.size() != n) throw std::invalid_argument("duplicate_sets: rep / sizes lengths differ");
  Sets r;
  r.set_rep.assign(n / 2, 0);
  r.set_offsets.assign(n / 2 + 1, 0);
  r.set_bytes.assign(n / 2, 0);
  r.members.assign(n, 0);
  const int rc = sdcas_duplicate_sets(ctx_, rep.data(), sizes.empty() ? nullptr : sizes.data(), n, order,
                                      r.set_rep.data(), r.set_offsets.data(), r.set_bytes.data(), r.members.data(),
                                      &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_duplicate_sets");
  r.set_rep.resize(r.counts.sets);
  r.set_offsets.resize(r.counts.sets + 1);
  r.set_bytes.resize(r.counts.sets);
  r.members.resize(r.counts.members);
  return r;
}

ReclaimReport reclaim_report_from(const std::vector<FilePathRow>& rows, const std::vector<int64_t>& set_rep,
                                  const std::vector<uint64_t>& set_offsets, const std::vector<uint64_t>& set_bytes,
                                  const std::vector<int64_t>& members, const sdcas_sets_counts& counts) {
  const size_t sets = set_rep.size();
  if (sets == 0 && set_offsets.empty() && set_bytes.empty() && members.empty()) {  // nothing at all: no sets
    ReclaimReport none;
    none.counts = counts;
    return none;
  }
  if (set_bytes.size() != sets || set_offsets.size() != sets + 1 || set_offsets.front() != 0 ||
      set_offsets.back() != members.size())
    throw std::invalid_argument("reclaim_report_from: set_rep / set_offsets / set_bytes / members lengths differ");
  ReclaimReport out;
  out.counts = counts;
  out.sets.resize(sets);
  for (size_t s = 0; s < sets; ++s) {
    if (set_offsets[s] > set_offsets[s + 1] || set_offsets[s + 1] > members.size())
      throw std::invalid_argument("reclaim_report_from: set_offsets do not ascend");
    ReclaimReport::Set& set = out.sets[s];
    for (uint64_t j = set_offsets[s]; j < set_offsets[s + 1]; ++j) {
      if (members[j] < 0 || (uint64_t)members[j] >= rows.size())
        throw std::invalid_argument("reclaim_report_from: member " + std::to_string(j) + " is no row");
      set.file_path_ids.push_back(rows[(size_t)members[j]].id);
    }
    if (set.file_path_ids.empty()) throw std::invalid_argument("reclaim_report_from: an empty set");
    // rows are in id order, so ascending members are ascending ids; a caller's
    // rows in another order still get what the header promises
    std::sort(set.file_path_ids.begin(), set.file_path_ids.end());
    set.bytes = set_bytes[s];
    set.reclaimable_bytes = (uint64_t)(set.file_path_ids.size() - 1) * set.bytes;
  }
  return out;
}

ReclaimReport reclaim_report(Engine& engine, Library& db, int32_t location_id, const std::string& sub) {
  const std::vector<FilePathRow> rows = db.file_paths_with_checksum(location_id, sub);
  const size_t n = rows.size();
  std::vector<uint64_t> keys(n, 0), sizes(n, 0);
  std::vector<uint8_t> digests(32 * n, 0), valid(n, 0);
  for (size_t i = 0; i < n; ++i) {
    sizes[i] = rows[i].size_in_bytes;
    uint8_t k[8];
    if (!rows[i].cas_id || !rows[i].integrity_checksum || !hex_to_bytes(*rows[i].cas_id, k, 8) ||
        !hex_to_bytes(*rows[i].integrity_checksum, &digests[32 * i], 32))
      continue;
    keys[i] = hex_to_key(*rows[i].cas_id);
    valid[i] = 1;
  }
  if (n == 0) return ReclaimReport{};
  const Engine::Confirm c = engine.confirm_duplicates(keys, digests, valid);
  const Engine::Sets s = engine.duplicate_sets(c.rep, sizes, SDCAS_SETS_BY_RECLAIMABLE);
  return reclaim_report_from(rows, s.set_rep, s.set_offsets, s.set_bytes, s.members, s.counts);
}

// ---- duplicate directories ---------------------------------------------------------

std::vector<uint8_t> Engine::hash_strings(const std::vector<std::string>& strings) {
  const size_t n = strings.size();
  std::vector<uint64_t> offs(n, 0), lens(n, 0);
  std::string blob;
  for (size_t i = 0; i < n; ++i) {
    offs[i] = blob.size();
    lens[i] = strings[i].size();
    blob += strings[i];
  }
  blob.append(64, '\0');  // never empty, and readable past the last string
  std::vector<uint8_t> out(32 * n, 0);
  if (n == 0) return out;
  const int rc = sdcas_hash_messages(ctx_, reinterpret_cast<const uint8_t*>(blob.data()), offs.data(), lens.data(), n,
                                     out.data());
  if (rc != SDCAS_OK) fail(rc, "sdcas_hash_messages");
  return out;
}

Engine::TreeDigests Engine::tree_digests(const std::vector<int64_t>& parent, const std::vector<uint8_t>& is_dir,
                                         const std::vector<uint8_t>& name32, const std::vector<uint64_t>& sizes,
                                         const std::vector<uint64_t>& keys, const std::vector<uint8_t>& digests,
                                         const std::vector<uint8_t>& valid) {
  const size_t n = parent.size();
  if (is_dir.size() != n || name32.size() != 32 * n || digests.size() != 32 * n || keys.size() != n ||
      (!sizes.empty() && sizes.size() != n) || (!valid.empty() && valid.size() != n))
    throw std::invalid_argument("tree_digests: the arrays' lengths differ");
  TreeDigests r;
  r.keys = keys, r.digests = digests, r.valid = valid;
  r.tree_bytes.assign(n, 0);
  r.tree_files.assign(n, 0);
  r.flags.assign(n, 0);
  const int rc = sdcas_tree_digests(ctx_, parent.data(), is_dir.data(), name32.data(),
                                    sizes.empty() ? nullptr : sizes.data(), n, r.keys.data(), r.digests.data(),
                                    r.valid.empty() ? nullptr : r.valid.data(), r.tree_bytes.data(),
                                    r.tree_files.data(), r.flags.data(), &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_tree_digests");
  return r;
}

Engine::TreeTop Engine::tree_top(const std::vector<int64_t>& parent, const std::vector<int64_t>& rep) {
  const size_t n = parent.size();
  if (rep.size() != n) throw std::invalid_argument("tree_top: parent / rep lengths differ");
  TreeTop r;
  r.top_rep.assign(n, -1);
  r.flags.assign(n, 0);
  const int rc = sdcas_tree_top(ctx_, parent.data(), rep.data(), n, r.top_rep.data(), r.flags.data(), &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_tree_top");
  return r;
}

std::vector<FilePathRow> Library::file_paths_in_location(int32_t, const std::string&) {
  throw LibraryError(SDCAS_E_INVALID, "this Library does not implement file_paths_in_location");
}

std::vector<FilePathRow> MemoryLibrary::file_paths_in_location(int32_t location_id, const std::string& sub) {
  std::vector<FilePathRow> out;
  for (const auto& r : file_paths)
    if (r.location_id == location_id && under(r, sub)) out.push_back(r);
  return out;
}

std::string entry_name(const FilePathRow& row) {
  return row.is_dir || row.extension.empty() ? row.name : row.name + "." + row.extension;
}

TreeShape tree_shape_from(const std::vector<FilePathRow>& rows) {
  const size_t n = rows.size();
  TreeShape t;
  t.parent.assign(n, -1);
  t.is_dir.assign(n, 0);
  std::map<std::string, int64_t> dir_at;  // a directory row's own path -> its index
  for (size_t i = 0; i < n; ++i) {
    t.is_dir[i] = rows[i].is_dir ? 1 : 0;
    if (rows[i].is_dir) dir_at.emplace(rows[i].materialized_path + rows[i].name + "/", (int64_t)i);
  }
  for (size_t i = 0; i < n; ++i) {
    const auto it = dir_at.find(rows[i].materialized_path);
    if (it != dir_at.end() && it->second != (int64_t)i) t.parent[i] = it->second;
  }
  return t;
}

TreeReport tree_report_from(const std::vector<FilePathRow>& rows, const std::vector<uint64_t>& tree_bytes,
                            const std::vector<uint64_t>& tree_files, const std::vector<int64_t>& set_rep,
                            const std::vector<uint64_t>& set_offsets, const std::vector<uint64_t>& set_bytes,
                            const std::vector<int64_t>& members, const sdcas_sets_counts& counts) {
  if (tree_bytes.size() != rows.size() || tree_files.size() != rows.size())
    throw std::invalid_argument("tree_report_from: tree_bytes / tree_files do not fit the rows");
  // the sets' shape is reclaim_report_from's: the same checks, the same order
  const ReclaimReport base = reclaim_report_from(rows, set_rep, set_offsets, set_bytes, members, counts);
  TreeReport out;
  out.counts = counts;
  out.sets.resize(base.sets.size());
  for (size_t s = 0; s < base.sets.size(); ++s) {
    if (set_rep[s] < 0 || (uint64_t)set_rep[s] >= rows.size())
      throw std::invalid_argument("tree_report_from: set_rep " + std::to_string(s) + " is no row");
    const size_t first = (size_t)set_rep[s];
    TreeReport::Set& set = out.sets[s];
    set.file_path_ids = base.sets[s].file_path_ids;
    set.is_dir = rows[first].is_dir;
    set.tree_bytes = tree_bytes[first];
    set.tree_files = tree_files[first];
    if (set.tree_bytes != set_bytes[s])
      throw std::invalid_argument("tree_report_from: set_bytes " + std::to_string(s) + " is not its first row's tree_bytes");
    set.reclaimable_bytes = base.sets[s].reclaimable_bytes;
  }
  return out;
}

TreeReport tree_report(Engine& engine, Library& db, int32_t location_id, const std::string& sub) {
  const std::vector<FilePathRow> rows = db.file_paths_in_location(location_id, sub);
  const size_t n = rows.size();
  if (n == 0) return TreeReport{};
  const TreeShape shape = tree_shape_from(rows);
  std::vector<std::string> names(n);
  std::vector<uint64_t> keys(n, 0), sizes(n, 0);
  std::vector<uint8_t> digests(32 * n, 0), valid(n, 0);
  for (size_t i = 0; i < n; ++i) {
    names[i] = entry_name(rows[i]);
    if (rows[i].is_dir) continue;
    sizes[i] = rows[i].size_in_bytes;
    if (!rows[i].integrity_checksum || !hex_to_bytes(*rows[i].integrity_checksum, &digests[32 * i], 32)) {
      std::fill(digests.begin() + 32 * i, digests.begin() + 32 * (i + 1), 0);
      continue;
    }
    for (size_t b = 0; b < 8; ++b) keys[i] = keys[i] << 8 | digests[32 * i + b];  // one key rule for both kinds
    valid[i] = 1;
  }
  const std::vector<uint8_t> name32 = engine.hash_strings(names);
  const Engine::TreeDigests t = engine.tree_digests(shape.parent, shape.is_dir, name32, sizes, keys, digests, valid);
  const Engine::Confirm c = engine.confirm_duplicates(t.keys, t.digests, t.valid);
  const Engine::TreeTop top = engine.tree_top(shape.parent, c.rep);
  const Engine::Sets s = engine.duplicate_sets(top.top_rep, t.tree_bytes, SDCAS_SETS_BY_RECLAIMABLE);
  TreeReport out =
      tree_report_from(rows, t.tree_bytes, t.tree_files, s.set_rep, s.set_offsets, s.set_bytes, s.members, s.counts);
  out.tree = t.counts;
  out.top = top.counts;
  return out;
}

// ---- files that share most of their bytes ---------------------------------------------

Engine::Chunks Engine::chunk_messages(const std::vector<uint8_t>& blob, const std::vector<uint64_t>& offsets,
                                      const std::vector<uint64_t>& lens, const sdcas_chunk_params* params) {
  const size_t n = lens.size();
  if (offsets.size() != n) throw std::invalid_argument("chunk_messages: offsets / lens lengths differ");
  for (size_t i = 0; i < n; ++i)
    if (offsets[i] > blob.size() || lens[i] > blob.size() - offsets[i])
      throw std::invalid_argument("chunk_messages: file " + std::to_string(i) + " ends past the blob");
  uint64_t max_chunks = 0;
  int rc = sdcas_chunk_plan(lens.data(), n, params, &max_chunks, nullptr);
  if (rc != SDCAS_OK) throw LibraryError(rc, "sdcas_chunk_plan: the parameters or the lengths are refused");
  Chunks r;
  r.file_chunks.assign(n + 1, 0);
  r.chunk_off.assign(max_chunks, 0), r.chunk_len.assign(max_chunks, 0), r.keys.assign(max_chunks, 0);
  r.chunk_file.assign(max_chunks, 0);
  r.digests.assign(32 * max_chunks, 0);
  rc = sdcas_chunk_messages(ctx_, blob.data(), offsets.data(), lens.data(), n, params, r.file_chunks.data(),
                            r.chunk_off.data(), r.chunk_len.data(), r.chunk_file.data(), r.keys.data(),
                            r.digests.data(), &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_chunk_messages");
  const size_t m = r.counts.chunks;
  r.chunk_off.resize(m), r.chunk_len.resize(m), r.keys.resize(m), r.chunk_file.resize(m), r.digests.resize(32 * m);
  return r;
}

Engine::Sharing Engine::chunk_sharing(const std::vector<uint32_t>& chunk_file, const std::vector<uint64_t>& chunk_len,
                                      const std::vector<int64_t>& rep, size_t n_files) {
  const size_t m = chunk_file.size();
  if (chunk_len.size() != m || rep.size() != m) throw std::invalid_argument("chunk_sharing: the arrays' lengths differ");
  Sharing r;
  r.new_bytes.assign(n_files, 0), r.self_bytes.assign(n_files, 0), r.other_bytes.assign(n_files, 0);
  r.peer_bytes.assign(n_files, 0);
  r.peer.assign(n_files, -1);
  const int rc = sdcas_chunk_sharing(ctx_, chunk_file.data(), chunk_len.data(), rep.data(), m, n_files,
                                     r.new_bytes.data(), r.self_bytes.data(), r.other_bytes.data(), r.peer.data(),
                                     r.peer_bytes.data(), &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_chunk_sharing");
  return r;
}

SimilarityReport similarity_report_from(const std::vector<FilePathRow>& rows, const std::vector<uint64_t>& sizes,
                                        const std::vector<int64_t>& peer, const std::vector<uint64_t>& peer_bytes) {
  const size_t n = rows.size();
  if (sizes.size() != n || peer.size() != n || peer_bytes.size() != n)
    throw std::invalid_argument("similarity_report_from: sizes / peer / peer_bytes do not fit the rows");
  SimilarityReport out;
  for (size_t i = 0; i < n; ++i) {
    if (peer[i] == -1) {
      if (peer_bytes[i]) throw std::invalid_argument("similarity_report_from: row " + std::to_string(i) + " shares bytes with no peer");
      continue;
    }
    if (peer[i] < 0 || (uint64_t)peer[i] >= n || (size_t)peer[i] == i)
      throw std::invalid_argument("similarity_report_from: the peer of row " + std::to_string(i) + " is no other row");
    out.pairs.push_back(SimilarityReport::Pair{rows[i].id, rows[(size_t)peer[i]].id, peer_bytes[i], sizes[i]});
  }
  std::sort(out.pairs.begin(), out.pairs.end(), [](const SimilarityReport::Pair& a, const SimilarityReport::Pair& b) {
    return a.shared_bytes != b.shared_bytes ? a.shared_bytes > b.shared_bytes : a.file_path_id < b.file_path_id;
  });
  return out;
}

SimilarityReport similarity_report(Engine& engine, Library& db, const Location& location, const std::string& sub,
                                   uint64_t max_bytes) {
  std::vector<FilePathRow> rows;
  for (FilePathRow& r : db.file_paths_in_location(location.id, sub))
    if (!r.is_dir) rows.push_back(std::move(r));
  const size_t n = rows.size();
  if (n == 0) return SimilarityReport{};
  std::vector<uint8_t> blob;
  std::vector<uint64_t> offsets(n, 0), lens(n, 0);
  for (size_t i = 0; i < n; ++i) {
    offsets[i] = blob.size();
    std::FILE* f = std::fopen(full_path(location, rows[i]).c_str(), "rb");
    if (!f) continue;
    uint8_t buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) {
      if (blob.size() + got > max_bytes) {
        std::fclose(f);
        throw LibraryError(SDCAS_E_CAPACITY, "similarity_report: the files hold more than max_bytes = " +
                                                 std::to_string(max_bytes) + " bytes");
      }
      blob.insert(blob.end(), buf, buf + got);
    }
    std::fclose(f);
    lens[i] = blob.size() - offsets[i];
  }
  const Engine::Chunks ch = engine.chunk_messages(blob, offsets, lens);
  const Engine::Confirm c = engine.confirm_duplicates(ch.keys, ch.digests, {});
  const Engine::Sharing s = engine.chunk_sharing(ch.chunk_file, ch.chunk_len, c.rep, n);
  SimilarityReport out = similarity_report_from(rows, lens, s.peer, s.peer_bytes);
  out.chunks = ch.counts;
  out.counts = s.counts;
  return out;
}

// ---- the same for files that are not resident at once ----------------------------------

Engine::WindowChunks Engine::chunk_windows(const std::vector<uint8_t>& blob, const std::vector<uint64_t>& offsets,
                                           const std::vector<uint64_t>& lens, const std::vector<uint8_t>& final,
                                           const sdcas_chunk_params* params) {
  const size_t n = lens.size();
  if (offsets.size() != n || (!final.empty() && final.size() != n))
    throw std::invalid_argument("chunk_windows: offsets / lens / final lengths differ");
  for (size_t i = 0; i < n; ++i)
    if (offsets[i] > blob.size() || lens[i] > blob.size() - offsets[i])
      throw std::invalid_argument("chunk_windows: window " + std::to_string(i) + " ends past the blob");
  uint64_t max_chunks = 0;
  int rc = sdcas_chunk_plan(lens.data(), n, params, &max_chunks, nullptr);
  if (rc != SDCAS_OK) throw LibraryError(rc, "sdcas_chunk_plan: the parameters or the lengths are refused");
  WindowChunks r;
  r.file_chunks.assign(n + 1, 0), r.consumed.assign(n, 0);
  r.chunk_off.assign(max_chunks, 0), r.chunk_len.assign(max_chunks, 0), r.keys.assign(max_chunks, 0);
  r.chunk_file.assign(max_chunks, 0);
  r.digests.assign(32 * max_chunks, 0);
  rc = sdcas_chunk_windows(ctx_, blob.data(), offsets.data(), lens.data(), final.empty() ? nullptr : final.data(), n,
                           params, r.file_chunks.data(), r.chunk_off.data(), r.chunk_len.data(), r.chunk_file.data(),
                           r.keys.data(), r.digests.data(), r.consumed.data(), &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_chunk_windows");
  const size_t m = r.counts.chunks;
  r.chunk_off.resize(m), r.chunk_len.resize(m), r.keys.resize(m), r.chunk_file.resize(m), r.digests.resize(32 * m);
  return r;
}

std::vector<WindowPlan> plan_chunk_windows(const std::vector<uint64_t>& sizes, uint64_t window_bytes) {
  if (window_bytes == 0) throw std::invalid_argument("plan_chunk_windows: window_bytes must be positive");
  std::vector<WindowPlan> plan;
  size_t first = 0;
  uint64_t held = 0;
  for (size_t i = 0; i < sizes.size(); ++i) {
    if (sizes[i] > window_bytes) {
      if (i > first) plan.push_back(WindowPlan{first, i - first, false});
      plan.push_back(WindowPlan{i, 1, true});
      first = i + 1, held = 0;
    } else if (sizes[i] > window_bytes - held) {
      plan.push_back(WindowPlan{first, i - first, false});
      first = i, held = sizes[i];
    } else {
      held += sizes[i];
    }
  }
  if (sizes.size() > first) plan.push_back(WindowPlan{first, sizes.size() - first, false});
  return plan;
}

Engine::Chunks merge_chunk_windows(const std::vector<ChunkWindow>& windows, size_t n_files, std::vector<uint64_t>* sizes) {
  Engine::Chunks out;
  std::vector<uint64_t> per_file(n_files, 0), used(n_files, 0);
  size_t last_file = 0, last_n = 0;
  uint64_t last_pos = 0;
  for (const ChunkWindow& w : windows) {
    const Engine::WindowChunks& c = w.chunks;
    const size_t nf = w.offsets.size(), m = c.chunk_off.size();
    if (c.consumed.size() != nf || c.chunk_len.size() != m || c.chunk_file.size() != m || c.keys.size() != m ||
        c.digests.size() != 32 * m)
      throw std::invalid_argument("merge_chunk_windows: a window's arrays do not fit each other");
    // the next window of a streamed file follows in that file; any other begins behind the files before it
    const bool follows = nf == 1 && last_n == 1 && w.first_file == last_file && w.file_pos >= last_pos && w.file_pos;
    if ((!follows && w.first_file < last_file + last_n) || w.first_file > n_files || nf > n_files - w.first_file)
      throw std::invalid_argument("merge_chunk_windows: a window goes back or names a file past n_files");
    if (w.file_pos && nf != 1) throw std::invalid_argument("merge_chunk_windows: a window inside a file holds that file alone");
    uint32_t before = 0;
    for (size_t k = 0; k < m; ++k) {
      const uint32_t f = c.chunk_file[k];
      if (f >= nf || f < before || c.chunk_off[k] < w.offsets[f])
        throw std::invalid_argument("merge_chunk_windows: a window's chunks are not in its files' order");
      before = f;
      out.chunk_file.push_back((uint32_t)(w.first_file + f));
      out.chunk_off.push_back(c.chunk_off[k] - w.offsets[f] + w.file_pos);
      out.chunk_len.push_back(c.chunk_len[k]);
      out.keys.push_back(c.keys[k]);
      ++per_file[w.first_file + f];
    }
    out.digests.insert(out.digests.end(), c.digests.begin(), c.digests.end());
    for (size_t f = 0; f < nf; ++f) used[w.first_file + f] += c.consumed[f];
    out.counts.files += c.counts.files, out.counts.chunks += c.counts.chunks;
    out.counts.total_bytes += c.counts.total_bytes, out.counts.hash_cuts += c.counts.hash_cuts;
    out.counts.max_cuts += c.counts.max_cuts, out.counts.end_chunks += c.counts.end_chunks;
    if (nf) last_file = w.first_file, last_n = nf, last_pos = w.file_pos;
  }
  out.file_chunks.assign(n_files + 1, 0);
  for (size_t i = 0; i < n_files; ++i) out.file_chunks[i + 1] = out.file_chunks[i] + per_file[i];
  if (sizes) *sizes = used;
  return out;
}

namespace {

// up to `want` bytes of f from pos on, appended to blob -> the bytes read
uint64_t read_some(std::FILE* f, uint64_t pos, uint64_t want, std::vector<uint8_t>& blob) {
  if (!f || fseeko(f, (off_t)pos, SEEK_SET) != 0) return 0;
  uint8_t buf[1 << 16];
  uint64_t total = 0;
  while (total < want) {
    const size_t ask = (size_t)std::min<uint64_t>(sizeof buf, want - total);
    const size_t got = std::fread(buf, 1, ask, f);
    if (!got) break;
    blob.insert(blob.end(), buf, buf + got);
    total += got;
  }
  return total;
}

// the chunks of the rows' files, read through windows of at most window_bytes,
// as one call over the whole files would give them; used[i]: the bytes read of
// row i's file
Engine::Chunks chunk_rows_windowed(Engine& engine, const Location& location, const std::vector<FilePathRow>& rows,
                                   uint64_t window_bytes, std::vector<uint64_t>& used) {
  const size_t n = rows.size();
  std::vector<uint64_t> sizes(n, 0);  // a file that cannot be read counts as empty
  for (size_t i = 0; i < n; ++i)
    if (std::FILE* f = std::fopen(full_path(location, rows[i]).c_str(), "rb")) {
      if (fseeko(f, 0, SEEK_END) == 0 && ftello(f) > 0) sizes[i] = (uint64_t)ftello(f);
      std::fclose(f);
    }
  std::vector<ChunkWindow> windows;
  for (const WindowPlan& wp : plan_chunk_windows(sizes, window_bytes)) {
    if (!wp.streamed) {
      ChunkWindow w;
      w.first_file = wp.first_file;
      std::vector<uint8_t> blob;
      std::vector<uint64_t> lens(wp.n_files, 0);
      for (size_t k = 0; k < wp.n_files; ++k) {
        w.offsets.push_back(blob.size());
        std::FILE* f = std::fopen(full_path(location, rows[wp.first_file + k]).c_str(), "rb");
        lens[k] = read_some(f, 0, sizes[wp.first_file + k], blob);
        if (f) std::fclose(f);
      }
      w.chunks = engine.chunk_windows(blob, w.offsets, lens, {});
      windows.push_back(std::move(w));
      continue;
    }
    std::FILE* f = std::fopen(full_path(location, rows[wp.first_file]).c_str(), "rb");
    uint64_t pos = 0, want = window_bytes;
    for (;;) {
      ChunkWindow w;
      w.first_file = wp.first_file, w.file_pos = pos, w.offsets = {0};
      std::vector<uint8_t> blob;
      const uint64_t got = read_some(f, pos, want, blob);
      const bool final = got < want || pos + got >= sizes[wp.first_file];
      w.chunks = engine.chunk_windows(blob, w.offsets, {got}, {(uint8_t)final});
      const uint64_t used = w.chunks.consumed[0];
      if (!final && used == 0) {
        want *= 2;  // shorter than max_len: nothing could be decided
        continue;
      }
      windows.push_back(std::move(w));
      if (final) break;
      pos += used, want = window_bytes;
    }
    if (f) std::fclose(f);
  }
  return merge_chunk_windows(windows, n, &used);
}

}  // namespace

SimilarityReport similarity_report_streamed(Engine& engine, Library& db, const Location& location, const std::string& sub,
                                            uint64_t window_bytes) {
  std::vector<FilePathRow> rows;
  for (FilePathRow& r : db.file_paths_in_location(location.id, sub))
    if (!r.is_dir) rows.push_back(std::move(r));
  const size_t n = rows.size();
  if (n == 0) return SimilarityReport{};
  std::vector<uint64_t> used;
  const Engine::Chunks ch = chunk_rows_windowed(engine, location, rows, window_bytes, used);
  const Engine::Confirm c = engine.confirm_duplicates(ch.keys, ch.digests, {});
  const Engine::Sharing s = engine.chunk_sharing(ch.chunk_file, ch.chunk_len, c.rep, n);
  SimilarityReport out = similarity_report_from(rows, used, s.peer, s.peer_bytes);
  out.chunks = ch.counts;
  out.counts = s.counts;
  return out;
}

// ---- the same against the chunks stored before ------------------------------------------

Engine::IndexMatch Engine::chunk_index_match(const ChunkIndexData& index, const std::vector<uint64_t>& keys,
                                             const std::vector<uint8_t>& digests, const std::vector<uint8_t>& valid) {
  const size_t n = index.size(), m = keys.size();
  if (index.digests.size() != 32 * n || index.values.size() != n || index.bits > SDCAS_INDEX_MAX_BITS ||
      index.dir.size() != (size_t(1) << index.bits) + 1)
    throw std::invalid_argument("chunk_index_match: the index's arrays do not fit each other");
  if (digests.size() != 32 * m || (!valid.empty() && valid.size() != m))
    throw std::invalid_argument("chunk_index_match: keys / digests / valid lengths differ");
  IndexMatch r;
  r.pos.assign(m, -1), r.value.assign(m, 0);
  const int rc = sdcas_chunk_index_match(ctx_, index.keys.data(), index.digests.data(), index.values.data(),
                                         index.dir.data(), n, index.bits, keys.data(), digests.data(),
                                         valid.empty() ? nullptr : valid.data(), m, r.pos.data(), r.value.data(),
                                         &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_chunk_index_match");
  return r;
}

Engine::IndexAdd Engine::chunk_index_add(const ChunkIndexData& index, const std::vector<uint64_t>& keys,
                                         const std::vector<uint8_t>& digests, const std::vector<uint64_t>& values,
                                         const std::vector<uint8_t>& valid) {
  const size_t n = index.size(), m = keys.size();
  if (index.digests.size() != 32 * n || index.values.size() != n || index.bits > SDCAS_INDEX_MAX_BITS ||
      index.dir.size() != (size_t(1) << index.bits) + 1)
    throw std::invalid_argument("chunk_index_add: the index's arrays do not fit each other");
  if (digests.size() != 32 * m || values.size() != m || (!valid.empty() && valid.size() != m))
    throw std::invalid_argument("chunk_index_add: keys / digests / values / valid lengths differ");
  IndexAdd r;
  ChunkIndexData& out = r.index;
  out.bits = sdcas_chunk_index_dir_bits(n + m);
  out.keys.assign(n + m, 0), out.values.assign(n + m, 0), out.digests.assign(32 * (n + m), 0);
  out.dir.assign((size_t(1) << out.bits) + 1, 0);
  r.pos.assign(m, -1), r.flags.assign(m, 0);
  const int rc = sdcas_chunk_index_add(ctx_, index.keys.data(), index.digests.data(), index.values.data(),
                                       index.dir.data(), n, index.bits, keys.data(), digests.data(), values.data(),
                                       valid.empty() ? nullptr : valid.data(), m, out.keys.data(), out.digests.data(),
                                       out.values.data(), out.dir.data(), out.bits, r.pos.data(), r.flags.data(),
                                       &r.counts);
  if (rc != SDCAS_OK) fail(rc, "sdcas_chunk_index_add");
  const size_t e = r.counts.entries_new;
  out.keys.resize(e), out.values.resize(e), out.digests.resize(32 * e);
  return r;
}

IndexedSharing indexed_sharing(Engine& engine, const Engine::Chunks& chunks, const std::vector<int64_t>& rep,
                               const Engine::IndexMatch& match, const std::vector<uint64_t>& file_ids) {
  const size_t m = chunks.chunk_file.size(), n = file_ids.size();
  if (chunks.chunk_len.size() != m || rep.size() != m || match.pos.size() != m || match.value.size() != m)
    throw std::invalid_argument("indexed_sharing: the chunk arrays do not fit each other");
  for (size_t c = 0; c < m; ++c)
    if (chunks.chunk_file[c] >= n || rep[c] < 0 || (size_t)rep[c] > c)
      throw std::invalid_argument("indexed_sharing: chunk " + std::to_string(c) + " names no file or no earlier chunk");
  // Files get ordinals by the rank of their id over the stored owners and the
  // batch's ids, so that the sharing pass's tie rule (the lowest ordinal) is
  // the lowest id. One pseudo-chunk of no bytes per chunk that is its pair's
  // lowest in the batch and is in the index stands in front of the batch's
  // chunks, owned by the stored owner: a batch chunk the index holds then has
  // its lowest copy there.
  std::vector<size_t> heads;
  std::vector<uint64_t> all_ids(file_ids);
  for (size_t c = 0; c < m; ++c)
    if (match.pos[c] >= 0 && (size_t)rep[c] == c) {
      heads.push_back(c);
      all_ids.push_back(match.value[c]);
    }
  std::sort(all_ids.begin(), all_ids.end());
  all_ids.erase(std::unique(all_ids.begin(), all_ids.end()), all_ids.end());
  auto ordinal_of = [&](uint64_t id) { return (uint32_t)(std::lower_bound(all_ids.begin(), all_ids.end(), id) - all_ids.begin()); };
  std::vector<uint32_t> ordinal(n);
  for (size_t i = 0; i < n; ++i) ordinal[i] = ordinal_of(file_ids[i]);
  const size_t nh = heads.size();
  std::vector<uint32_t> s_file(nh + m);
  std::vector<uint64_t> s_len(nh + m, 0);
  std::vector<int64_t> s_rep(nh + m), slot(m, -1);
  for (size_t h = 0; h < nh; ++h) {
    s_file[h] = ordinal_of(match.value[heads[h]]);
    s_rep[h] = (int64_t)h;
    slot[heads[h]] = (int64_t)h;
  }
  for (size_t c = 0; c < m; ++c) {
    s_file[nh + c] = ordinal[chunks.chunk_file[c]];
    s_len[nh + c] = chunks.chunk_len[c];
    s_rep[nh + c] = match.pos[c] >= 0 ? slot[(size_t)rep[c]] : rep[c] + (int64_t)nh;
  }
  const Engine::Sharing s = engine.chunk_sharing(s_file, s_len, s_rep, all_ids.size());
  IndexedSharing out;
  out.indexed_bytes.assign(n, 0);
  for (size_t c = 0; c < m; ++c)
    if (match.pos[c] >= 0) out.indexed_bytes[chunks.chunk_file[c]] += chunks.chunk_len[c];
  for (size_t i = 0; i < n; ++i) {
    const uint32_t o = ordinal[i];
    out.new_bytes.push_back(s.new_bytes[o]), out.self_bytes.push_back(s.self_bytes[o]);
    out.other_bytes.push_back(s.other_bytes[o]), out.peer_bytes.push_back(s.peer_bytes[o]);
    out.peer.push_back(s.peer[o] < 0 ? -1 : (int64_t)all_ids[(size_t)s.peer[o]]);
  }
  return out;
}

SimilarityReport similarity_report_indexed(Engine& engine, SqliteLibrary& db, const Location& location,
                                           const std::string& sub, uint64_t window_bytes) {
  std::set<int32_t> done;
  for (const auto& f : db.chunk_indexed_files()) done.insert(f.first);
  std::vector<FilePathRow> rows;  // ascending by id: the order of the scan
  for (FilePathRow& r : db.file_paths_in_location(location.id, sub))
    if (!r.is_dir && !done.count(r.id)) rows.push_back(std::move(r));
  const size_t n = rows.size();
  if (n == 0) return SimilarityReport{};
  std::vector<uint64_t> used;
  const Engine::Chunks ch = chunk_rows_windowed(engine, location, rows, window_bytes, used);
  const size_t m = ch.keys.size();
  const Engine::Confirm c = engine.confirm_duplicates(ch.keys, ch.digests, {});
  const ChunkIndexData index = db.load_chunk_index();
  const Engine::IndexMatch match = engine.chunk_index_match(index, ch.keys, ch.digests, {});
  std::vector<uint64_t> file_ids(n), values(m);
  for (size_t i = 0; i < n; ++i) file_ids[i] = (uint64_t)rows[i].id;
  for (size_t k = 0; k < m; ++k) values[k] = file_ids[ch.chunk_file[k]];
  const IndexedSharing s = indexed_sharing(engine, ch, c.rep, match, file_ids);
  const Engine::IndexAdd add = engine.chunk_index_add(index, ch.keys, ch.digests, values, {});
  // what the add stored: the pairs whose value it took, with their rows
  std::vector<uint8_t> digests;
  std::vector<int32_t> owners;
  for (size_t k = 0; k < m; ++k)
    if (add.flags[k] & SDCAS_INDEX_ADDED) {
      digests.insert(digests.end(), ch.digests.begin() + 32 * k, ch.digests.begin() + 32 * (k + 1));
      owners.push_back((int32_t)values[k]);
    }
  std::vector<std::pair<int32_t, uint64_t>> files;
  for (size_t i = 0; i < n; ++i) files.emplace_back(rows[i].id, used[i]);
  db.append_chunk_index(digests, owners, files);
  SimilarityReport out;
  for (size_t i = 0; i < n; ++i)
    if (s.peer[i] >= 0) out.pairs.push_back(SimilarityReport::Pair{rows[i].id, (int32_t)s.peer[i], s.peer_bytes[i], used[i]});
  std::sort(out.pairs.begin(), out.pairs.end(), [](const SimilarityReport::Pair& a, const SimilarityReport::Pair& b) {
    return a.shared_bytes != b.shared_bytes ? a.shared_bytes > b.shared_bytes : a.file_path_id < b.file_path_id;
  });
  out.chunks = ch.counts;
  out.counts.files = n, out.counts.chunks = m, out.counts.files_with_peer = out.pairs.size();
  out.counts.distinct_chunks = add.counts.added, out.counts.total_bytes = ch.counts.total_bytes;
  for (size_t k = 0; k < m; ++k)
    if (add.flags[k] & SDCAS_INDEX_ADDED) out.counts.stored_bytes += ch.chunk_len[k];
  return out;
}

}  // namespace sdcore
