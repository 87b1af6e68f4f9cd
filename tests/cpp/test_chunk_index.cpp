// The chunk index in the C++ mirror (include/sdcore.hpp: SqliteLibrary's
// chunk_index / chunk_indexed_file tables, Engine::chunk_index_match / _add,
// similarity_report_indexed).
//
//   test_chunk_index            no GPU: the tables' round trip and order
//                               (digests from 0x00.. to 0xff..), an append
//                               that is refused leaves nothing, a table that
//                               is no index is refused on load
//   test_chunk_index --gpu DIR  the files under DIR/step1, step2, step3 (made
//                               by the caller) are moved into DIR/loc step by
//                               step; the union of similarity_report_indexed's
//                               reports must equal similarity_report_streamed
//                               over all of them, and a further run with
//                               nothing new reports and writes nothing
#include <dirent.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "sdcore.hpp"
#include "sqlite3_min.h"

using namespace sdcore;

static int failures = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      ++failures;                                              \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                       \
      std::fprintf(stderr, "\n");                              \
    }                                                          \
  } while (0)

// a digest whose first byte is `first`, the rest derived from `seed`
static std::vector<uint8_t> digest(uint8_t first, uint32_t seed) {
  std::vector<uint8_t> d(32);
  d[0] = first;
  for (int i = 1; i < 32; ++i) d[i] = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
  return d;
}

static void raw_sql(const std::string& path, const char* sql) {
  sqlite3* db = nullptr;
  if (sqlite3_open_v2(path.c_str(), &db, SQLITE_OPEN_READWRITE, nullptr) != SQLITE_OK) throw std::runtime_error("open " + path);
  char* err = nullptr;
  const int rc = sqlite3_exec(db, sql, nullptr, nullptr, &err);
  const std::string m = err ? err : "";
  sqlite3_free(err);
  sqlite3_close(db);
  if (rc != SQLITE_OK) throw std::runtime_error(std::string(sql) + ": " + m);
}

static void test_tables() {
  char tmpl[] = "/tmp/sd_chunk_index_XXXXXX";
  const char* dir = mkdtemp(tmpl);
  if (!dir) throw std::runtime_error("mkdtemp");
  const std::string path = std::string(dir) + "/lib.db";
  {
    auto db = SqliteLibrary::open(path);
    CHECK(db->load_chunk_index().size() == 0 && db->chunk_indexed_files().empty(), "a new library holds no chunks");
    ChunkIndexData empty = db->load_chunk_index();
    CHECK(empty.bits == 0 && (empty.dir == std::vector<uint32_t>{0, 0}), "the empty index's directory");
    // 40 digests appended out of order, first bytes from 0x00 to 0xff: SQLite
    // orders BLOBs as memcmp does, so 0x80.. and above come last
    const uint8_t firsts[] = {0xff, 0x00, 0x80, 0x7f, 0x81, 0x01, 0xfe, 0x40, 0xc0, 0x3f};
    std::vector<uint8_t> digests;
    std::vector<int32_t> owners;
    for (int round = 0; round < 4; ++round)
      for (int k = 0; k < 10; ++k) {
        const auto d = digest(firsts[k], 100u * round + k);
        digests.insert(digests.end(), d.begin(), d.end());
        owners.push_back(7 + round);
      }
    // two digests under one key (the first 8 bytes), ordered by a later byte
    auto twin = digest(0x55, 1), twin2 = twin;
    twin[20] = 0x01, twin2[20] = 0xf0;
    digests.insert(digests.end(), twin2.begin(), twin2.end()), owners.push_back(20);
    digests.insert(digests.end(), twin.begin(), twin.end()), owners.push_back(21);
    db->append_chunk_index(digests, owners, {{7, 1000}, {8, 0}, {10, 1ull << 40}, {9, 5}});
    const ChunkIndexData ix = db->load_chunk_index();
    CHECK(ix.size() == 42 && ix.digests.size() == 32 * 42 && ix.values.size() == 42, "42 entries come back");
    CHECK(ix.bits == sdcas_chunk_index_dir_bits(42) && ix.bits == 4 && ix.dir.size() == 17 && ix.dir.back() == 42, "the directory");
    bool ordered = true, keyed = true;
    for (size_t i = 0; i < ix.size(); ++i) {
      uint64_t key = 0;
      for (int b = 0; b < 8; ++b) key = key << 8 | ix.digests[32 * i + b];
      keyed = keyed && key == ix.keys[i];
      if (i) ordered = ordered && memcmp(&ix.digests[32 * (i - 1)], &ix.digests[32 * i], 32) < 0;
    }
    CHECK(ordered, "ascending as memcmp orders the digests");
    CHECK(keyed, "the key is the digest's first 8 bytes, big-endian");
    CHECK(ix.digests[0] == 0x00 && ix.digests[32 * 41] == 0xff && (ix.keys[41] >> 56) == 0xff, "0x00.. first, 0xff.. last");
    uint64_t bad = 0;
    CHECK(sdcas_chunk_index_check(ix.keys.data(), ix.digests.data(), ix.dir.data(), 42, ix.bits, &bad) == SDCAS_OK, "the check");
    // the owners travel with their digests
    size_t twins = 0;
    for (size_t i = 0; i + 1 < ix.size(); ++i)
      if (ix.keys[i] == ix.keys[i + 1]) {
        ++twins;
        CHECK(ix.values[i] == 21 && ix.values[i + 1] == 20 && ix.digests[32 * i + 20] == 0x01, "the twins' order and owners");
      }
    CHECK(twins == 1, "one key with two digests");
    const auto files = db->chunk_indexed_files();
    CHECK((files == std::vector<std::pair<int32_t, uint64_t>>{{7, 1000}, {8, 0}, {9, 5}, {10, 1ull << 40}}), "the indexed rows");
    // an append with a digest already stored, or a row already indexed, is refused whole
    bool threw = false;
    try {
      const auto fresh = digest(0x33, 9);
      std::vector<uint8_t> two(fresh);
      two.insert(two.end(), twin.begin(), twin.end());
      db->append_chunk_index(two, {30, 31}, {{11, 1}});
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw && db->load_chunk_index().size() == 42 && db->chunk_indexed_files().size() == 4, "a stored digest again");
    threw = false;
    try {
      db->append_chunk_index(digest(0x34, 9), {30}, {{8, 1}});
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw && db->load_chunk_index().size() == 42 && db->chunk_indexed_files().size() == 4, "an indexed row again");
    threw = false;
    try {
      db->append_chunk_index(std::vector<uint8_t>(31), {1}, {});
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw, "31 bytes are no digest");
    db->append_chunk_index({}, {}, {});
    CHECK(db->load_chunk_index().size() == 42, "nothing appended");
  }
  // a table that is no index: a digest of 4 bytes put there behind the library's back
  raw_sql(path, "INSERT INTO chunk_index (digest, file_path_id) VALUES (x'00112233', 5)");
  {
    auto db = SqliteLibrary::open(path);
    int code = 0;
    try {
      db->load_chunk_index();
    } catch (const LibraryError& e) {
      code = e.code;
    }
    CHECK(code == SDCAS_E_INVALID, "a 4-byte digest is refused on load (code %d)", code);
  }
  raw_sql(path, "DELETE FROM chunk_index WHERE length(digest) != 32");
  CHECK(SqliteLibrary::open(path)->load_chunk_index().size() == 42, "and loads again without it");
  std::remove(path.c_str());
  std::remove((path + "-wal").c_str());
  std::remove((path + "-shm").c_str());
  rmdir(dir);
}

// move every entry of `from` into `to`
static void move_all(const std::string& from, const std::string& to) {
  DIR* d = opendir(from.c_str());
  if (!d) throw std::runtime_error("opendir " + from);
  std::vector<std::string> names;
  while (dirent* e = readdir(d))
    if (std::strcmp(e->d_name, ".") && std::strcmp(e->d_name, "..")) names.push_back(e->d_name);
  closedir(d);
  for (const std::string& n : names)
    if (std::rename((from + "/" + n).c_str(), (to + "/" + n).c_str()) != 0) throw std::runtime_error("rename " + n);
}

static int test_gpu(const std::string& dir) {
  auto engine = Engine::open();
  const Location loc{1, dir + "/loc"};
  auto db = SqliteLibrary::open(dir + "/lib.db");
  std::set<std::string> known;
  std::vector<SimilarityReport::Pair> all;
  uint64_t chunks = 0;
  for (const char* step : {"step1", "step2", "step3"}) {
    move_all(dir + "/" + step, loc.path);
    std::vector<FilePathRow> fresh;
    for (FilePathRow r : walk_location(loc)) {
      r.location_id = 1;
      if (known.insert(r.materialized_path + r.name + "." + r.extension).second) fresh.push_back(r);
    }
    db->add_file_paths(fresh);  // ids ascend with the steps
    const size_t before = db->load_chunk_index().size();
    const SimilarityReport r = similarity_report_indexed(*engine, *db, loc, "", 200000);
    const size_t after = db->load_chunk_index().size();
    CHECK(after > before, "%s adds chunks (%zu -> %zu)", step, before, after);
    std::printf("%s: rows %zu pairs %zu index %zu\n", step, fresh.size(), r.pairs.size(), after);
    all.insert(all.end(), r.pairs.begin(), r.pairs.end());
    chunks += r.chunks.chunks;
  }
  const SimilarityReport want = similarity_report_streamed(*engine, *db, loc, "", 200000);
  std::sort(all.begin(), all.end(), [](const SimilarityReport::Pair& a, const SimilarityReport::Pair& b) {
    return a.shared_bytes != b.shared_bytes ? a.shared_bytes > b.shared_bytes : a.file_path_id < b.file_path_id;
  });
  CHECK(all == want.pairs, "the pairs differ: %zu and %zu", all.size(), want.pairs.size());
  CHECK(chunks == want.chunks.chunks, "the steps' chunks: %llu and %llu", (unsigned long long)chunks,
        (unsigned long long)want.chunks.chunks);
  CHECK(db->load_chunk_index().size() == want.counts.distinct_chunks, "the index holds the distinct chunks");
  bool crossed = false;  // a peer indexed by an earlier step
  const auto files = db->chunk_indexed_files();
  for (const auto& p : all) crossed = crossed || p.peer_id < p.file_path_id;
  CHECK(crossed && !all.empty(), "pairs reach back");
  // nothing new: nothing reported, nothing written
  const ChunkIndexData before = db->load_chunk_index();
  const SimilarityReport none = similarity_report_indexed(*engine, *db, loc, "", 200000);
  const ChunkIndexData after = db->load_chunk_index();
  CHECK(none.pairs.empty() && none.chunks.chunks == 0, "a run with nothing new reports nothing");
  CHECK(after.keys == before.keys && after.digests == before.digests && after.values == before.values &&
            db->chunk_indexed_files() == files,
        "and writes nothing");
  std::printf("pairs %zu chunks %llu\n", all.size(), (unsigned long long)chunks);
  return failures;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--gpu")) {
    const int f = test_gpu(argv[2]);
    std::printf(f ? "FAILED %d\n" : "ok\n", f);
    return f ? 1 : 0;
  }
  test_tables();
  std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
