// Duplicate directories in the C++ mirror (include/sdcore.hpp: tree_shape_from,
// tree_report_from, tree_report, Engine::tree_digests / tree_top).
//
//   test_dirtree              no GPU: tree_shape_from on hand-made rows (parents
//                             from materialized_path + name, absent directory
//                             rows, a sub scope), tree_report_from's mapping of
//                             entries to file_path ids, kinds and rollups, and
//                             arrays that do not fit together
//   test_dirtree --gpu DIR    the files under DIR/loc (made by the caller): the
//                             identifier job with checksums, then tree_report on
//                             a MemoryLibrary and a SqliteLibrary; the two must
//                             be equal and nothing may be written; the report is
//                             printed, one line per set, for the caller to
//                             compare with its own reference:
//                               set <d|f> <tree_bytes> <tree_files> <reclaimable> <path>|<path>...
#include <algorithm>
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

static FilePathRow row(int32_t id, const std::string& mp, const std::string& name, const std::string& ext, bool dir,
                       uint64_t size = 0) {
  FilePathRow r;
  r.id = id, r.location_id = 1, r.materialized_path = mp, r.name = name, r.extension = ext, r.is_dir = dir;
  r.size_in_bytes = size;
  return r;
}

// ---- no GPU ---------------------------------------------------------------------------

static void test_cpu() {
  // rows in no tree order: children before their directories, ids that are not indices
  //   0 /a/b/x.txt   1 /a/   2 /a/b/   3 /top.bin   4 /a/b/c/ (no row for /a/b/c/'s child's directory d)
  //   5 /a/b/c/d/deep.dat (its directory /a/b/c/d/ has no row: a root)   6 /a/README (no extension)
  const std::vector<FilePathRow> rows{row(70, "/a/b/", "x", "txt", false, 10), row(11, "/", "a", "", true),
                                      row(12, "/a/", "b", "", true),           row(13, "/", "top", "bin", false, 5),
                                      row(14, "/a/b/", "c", "", true),         row(15, "/a/b/c/d/", "deep", "dat", false, 7),
                                      row(16, "/a/", "README", "", false, 3)};
  const TreeShape t = tree_shape_from(rows);
  CHECK(t.parent == (std::vector<int64_t>{2, -1, 1, -1, 2, -1, 1}), "parents");
  CHECK(t.is_dir == (std::vector<uint8_t>{0, 1, 1, 0, 1, 0, 0}), "kinds");
  CHECK(entry_name(rows[0]) == "x.txt" && entry_name(rows[1]) == "a" && entry_name(rows[6]) == "README", "names");
  // a sub scope: the rows under /a/b/ alone: b's row is absent, so they are roots
  const TreeShape sub = tree_shape_from({rows[0], rows[4], rows[5]});
  CHECK(sub.parent == (std::vector<int64_t>{-1, -1, -1}), "a sub scope's rows are roots");
  // a directory named like its own parent path does not become its own parent
  const TreeShape self = tree_shape_from({row(1, "/", "", "", true)});
  CHECK(self.parent == (std::vector<int64_t>{-1}), "no entry is its own parent");
  CHECK(tree_shape_from({}).parent.empty(), "no rows");

  // the report's shaping: sets {1, 4}: directories of 17 bytes in 2 files; {0, 6, 3}: files of 10 bytes
  std::vector<uint64_t> tree_bytes{10, 17, 17, 10, 17, 7, 10}, tree_files{1, 2, 2, 1, 2, 1, 1};
  sdcas_sets_counts counts{};
  counts.files = 7, counts.sets = 2, counts.members = 5, counts.duplicate_files = 3, counts.reclaimable_bytes = 37;
  counts.largest_set = 3;
  const TreeReport r = tree_report_from(rows, tree_bytes, tree_files, {1, 0}, {0, 2, 5}, {17, 10}, {1, 4, 0, 3, 6}, counts);
  CHECK(r.sets.size() == 2, "%zu sets", r.sets.size());
  if (r.sets.size() == 2) {
    CHECK(r.sets[0].file_path_ids == (std::vector<int32_t>{11, 14}) && r.sets[0].is_dir, "set 0: the directories");
    CHECK(r.sets[0].tree_bytes == 17 && r.sets[0].tree_files == 2 && r.sets[0].reclaimable_bytes == 17, "set 0's bytes");
    CHECK(r.sets[1].file_path_ids == (std::vector<int32_t>{13, 16, 70}) && !r.sets[1].is_dir, "set 1: ids ascend");
    CHECK(r.sets[1].tree_bytes == 10 && r.sets[1].tree_files == 1 && r.sets[1].reclaimable_bytes == 20, "set 1's bytes");
  }
  CHECK(r.counts.sets == 2 && r.counts.reclaimable_bytes == 37, "the counts handed in");
  const sdcas_sets_counts zero{};
  CHECK(tree_report_from(rows, tree_bytes, tree_files, {}, {0}, {}, {}, zero).sets.empty(), "rows without sets");
  CHECK(tree_report_from({}, {}, {}, {}, {}, {}, {}, zero).sets.empty(), "nothing at all");
  CHECK(throws_invalid([&] { tree_report_from(rows, {1, 2}, tree_files, {1}, {0, 2}, {17}, {1, 4}, counts); }),
        "tree_bytes shorter than the rows");
  CHECK(throws_invalid([&] { tree_report_from(rows, tree_bytes, tree_files, {1}, {0, 2}, {18}, {1, 4}, counts); }),
        "set_bytes that are not the first row's tree_bytes");
  CHECK(throws_invalid([&] { tree_report_from(rows, tree_bytes, tree_files, {9}, {0, 2}, {17}, {1, 4}, counts); }),
        "a set_rep past the rows");
  CHECK(throws_invalid([&] { tree_report_from(rows, tree_bytes, tree_files, {1}, {0, 2}, {17}, {1, 7}, counts); }),
        "a member past the rows");
  CHECK(throws_invalid([&] { tree_report_from(rows, tree_bytes, tree_files, {1}, {0, 3}, {17}, {1, 4}, counts); }),
        "offsets past the members");
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
  FileIdentifierJobInit init{loc, "", 100};
  init.checksums = true;
  run_file_identifier_job(*engine, mem, init);
  run_file_identifier_job(*engine, *sql, init);
  const std::vector<FilePathRow> before = mem.file_paths;

  const TreeReport reports[2] = {tree_report(*engine, mem, 1), tree_report(*engine, *sql, 1)};
  CHECK(reports[0].sets == reports[1].sets, "the two libraries' reports differ");
  CHECK(!memcmp(&reports[0].tree, &reports[1].tree, sizeof reports[0].tree) &&
            !memcmp(&reports[0].top, &reports[1].top, sizeof reports[0].top) &&
            !memcmp(&reports[0].counts, &reports[1].counts, sizeof reports[0].counts),
        "the two libraries' counts differ");
  CHECK(reports[0].tree.entries == mem.file_paths.size(), "%llu entries", (unsigned long long)reports[0].tree.entries);
  uint64_t sum = 0;
  for (const auto& s : reports[0].sets) sum += s.reclaimable_bytes;
  CHECK(sum == reports[0].counts.reclaimable_bytes && reports[0].counts.sets == reports[0].sets.size(), "totals");
  for (size_t s = 1; s < reports[0].sets.size(); ++s)
    CHECK(reports[0].sets[s - 1].reclaimable_bytes >= reports[0].sets[s].reclaimable_bytes, "most reclaimable first");
  // read-only
  CHECK(mem.file_paths.size() == before.size(), "rows after");
  for (size_t i = 0; i < before.size() && i < mem.file_paths.size(); ++i)
    CHECK(before[i].object_id == mem.file_paths[i].object_id && before[i].cas_id == mem.file_paths[i].cas_id &&
              before[i].integrity_checksum == mem.file_paths[i].integrity_checksum,
          "row %d changed", before[i].id);
  // a sub scope reports what lies under it; another location has no rows
  const TreeReport scoped = tree_report(*engine, mem, 1, "/photos/");
  for (const auto& s : scoped.sets)
    for (int32_t id : s.file_path_ids)
      for (const FilePathRow& r : mem.file_paths)
        if (r.id == id) CHECK(r.materialized_path.compare(0, 8, "/photos/") == 0, "row %d is outside the scope", id);
  CHECK(tree_report(*engine, mem, 2).sets.empty(), "another location has no rows");

  std::map<int32_t, std::string> path_of;
  for (const FilePathRow& r : mem.file_paths) path_of[r.id] = (r.materialized_path + entry_name(r)).substr(1);
  std::printf("counts %llu %llu %llu\n", (unsigned long long)reports[0].tree.dirs,
              (unsigned long long)reports[0].top.dropped_classes, (unsigned long long)reports[0].counts.sets);
  for (const auto& s : reports[0].sets) {
    std::printf("set %c %llu %llu %llu ", s.is_dir ? 'd' : 'f', (unsigned long long)s.tree_bytes,
                (unsigned long long)s.tree_files, (unsigned long long)s.reclaimable_bytes);
    for (size_t k = 0; k < s.file_path_ids.size(); ++k)
      std::printf("%s%s", k ? "|" : "", path_of[s.file_path_ids[k]].c_str());
    std::printf("\n");
  }
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
