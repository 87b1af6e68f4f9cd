// Files that share most of their bytes in the C++ mirror (include/sdcore.hpp:
// Engine::chunk_messages / chunk_sharing, similarity_report_from,
// similarity_report).
//
//   test_chunks              no GPU: similarity_report_from's shaping (rows to
//                            file_path ids, most shared bytes first, ties by id)
//                            and the arrays it refuses
//   test_chunks --gpu DIR    the files under DIR/loc (made by the caller):
//                            similarity_report on a MemoryLibrary and a
//                            SqliteLibrary; the two must be equal and nothing may
//                            be written; the report is printed for the caller to
//                            compare with its own reference:
//                              counts <chunks> <distinct_chunks> <stored_bytes> <files_with_peer>
//                              pair <path> <peer path> <shared_bytes> <size>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "sdcore.hpp"

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

template <typename F>
static bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static FilePathRow row(int32_t id, const std::string& name) {
  FilePathRow r;
  r.id = id, r.location_id = 1, r.name = name, r.extension = "bin";
  return r;
}

// ---- no GPU ---------------------------------------------------------------------------

static void test_cpu() {
  // ids that are not indices; rows 1 and 3 share 500 bytes with their peers (a tie: the lower id first)
  const std::vector<FilePathRow> rows{row(40, "a"), row(12, "b"), row(33, "c"), row(7, "d"), row(50, "e")};
  const std::vector<uint64_t> sizes{1000, 900, 800, 700, 0};
  const SimilarityReport r = similarity_report_from(rows, sizes, {-1, 0, 0, 1, -1}, {0, 500, 650, 500, 0});
  CHECK(r.pairs.size() == 3, "%zu pairs", r.pairs.size());
  if (r.pairs.size() == 3) {
    CHECK((r.pairs[0] == SimilarityReport::Pair{33, 40, 650, 800}), "the most shared bytes first");
    CHECK((r.pairs[1] == SimilarityReport::Pair{7, 12, 500, 700}), "a tie: the lower file_path id first");
    CHECK((r.pairs[2] == SimilarityReport::Pair{12, 40, 500, 900}), "then the higher id");
  }
  CHECK(similarity_report_from(rows, sizes, {-1, -1, -1, -1, -1}, {0, 0, 0, 0, 0}).pairs.empty(), "no peers, no pairs");
  CHECK(similarity_report_from({}, {}, {}, {}).pairs.empty(), "nothing at all");
  CHECK(throws_invalid([&] { similarity_report_from(rows, {1, 2}, {-1, 0, 0, 1, -1}, {0, 5, 5, 5, 0}); }),
        "sizes shorter than the rows");
  CHECK(throws_invalid([&] { similarity_report_from(rows, sizes, {-1, 0, 0}, {0, 5, 5, 5, 0}); }), "peer shorter");
  CHECK(throws_invalid([&] { similarity_report_from(rows, sizes, {-1, 0, 0, 1, -1}, {0, 5, 5}); }), "peer_bytes shorter");
  CHECK(throws_invalid([&] { similarity_report_from(rows, sizes, {-1, 5, 0, 1, -1}, {0, 5, 5, 5, 0}); }),
        "a peer past the rows");
  CHECK(throws_invalid([&] { similarity_report_from(rows, sizes, {-1, 1, 0, 1, -1}, {0, 5, 5, 5, 0}); }),
        "a row that is its own peer");
  CHECK(throws_invalid([&] { similarity_report_from(rows, sizes, {-1, -2, 0, 1, -1}, {0, 5, 5, 5, 0}); }),
        "a negative peer that is not -1");
  CHECK(throws_invalid([&] { similarity_report_from(rows, sizes, {-1, 0, 0, 1, -1}, {9, 5, 5, 5, 0}); }),
        "bytes shared with no peer");
}

// ---- GPU ------------------------------------------------------------------------------

static int test_gpu(const std::string& dir) {
  auto engine = Engine::open();
  const Location loc{1, dir + "/loc"};
  MemoryLibrary mem;
  auto sql = SqliteLibrary::open(dir + "/library.db");
  std::vector<FilePathRow> rows;
  for (FilePathRow r : walk_location(loc)) {
    r.location_id = 1;
    rows.push_back(r);
  }
  for (const FilePathRow& r : rows) mem.add_file_path(r);
  sql->add_file_paths(rows);
  const std::vector<FilePathRow> before = mem.file_paths;

  const SimilarityReport reports[2] = {similarity_report(*engine, mem, loc), similarity_report(*engine, *sql, loc)};
  CHECK(reports[0].pairs == reports[1].pairs, "the two libraries' reports differ");
  CHECK(!memcmp(&reports[0].chunks, &reports[1].chunks, sizeof reports[0].chunks) &&
            !memcmp(&reports[0].counts, &reports[1].counts, sizeof reports[0].counts),
        "the two libraries' counts differ");
  CHECK(reports[0].counts.files_with_peer == reports[0].pairs.size(), "a pair per file with a peer");
  for (size_t p = 1; p < reports[0].pairs.size(); ++p)
    CHECK(reports[0].pairs[p - 1].shared_bytes >= reports[0].pairs[p].shared_bytes, "most shared bytes first");
  // read-only
  CHECK(mem.file_paths.size() == before.size(), "rows after");
  for (size_t i = 0; i < before.size() && i < mem.file_paths.size(); ++i)
    CHECK(before[i].object_id == mem.file_paths[i].object_id && before[i].cas_id == mem.file_paths[i].cas_id &&
              before[i].integrity_checksum == mem.file_paths[i].integrity_checksum,
          "row %d changed", before[i].id);
  // another location has no rows; a budget below the contents is refused
  CHECK(similarity_report(*engine, mem, Location{2, loc.path}).pairs.empty(), "another location has no rows");
  bool refused = false;
  try {
    similarity_report(*engine, mem, loc, "", 1000);
  } catch (const LibraryError& e) {
    refused = e.code == SDCAS_E_CAPACITY;
  }
  CHECK(refused, "max_bytes below the contents is SDCAS_E_CAPACITY");

  std::map<int32_t, std::string> path_of;
  for (const FilePathRow& r : mem.file_paths) path_of[r.id] = (r.materialized_path + entry_name(r)).substr(1);
  std::printf("counts %llu %llu %llu %llu\n", (unsigned long long)reports[0].counts.chunks,
              (unsigned long long)reports[0].counts.distinct_chunks, (unsigned long long)reports[0].counts.stored_bytes,
              (unsigned long long)reports[0].counts.files_with_peer);
  for (const auto& p : reports[0].pairs)
    std::printf("pair %s %s %llu %llu\n", path_of[p.file_path_id].c_str(), path_of[p.peer_id].c_str(),
                (unsigned long long)p.shared_bytes, (unsigned long long)p.size);
  return failures;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--gpu")) {
    const int f = test_gpu(argv[2]);
    std::printf(f ? "FAILED %d\n" : "ok\n", f);
    return f ? 1 : 0;
  }
  test_cpu();
  std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
