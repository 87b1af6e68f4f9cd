// Duplicate sets with their reclaimable bytes (include/sdcore.hpp:
// reclaim_report_from, reclaim_report, Engine::duplicate_sets).
//
//   test_dupsets              no GPU: reclaim_report_from on hand-made arrays:
//                             the mapping of file indices to file_path ids, the
//                             order of the sets, the totals, empty input and
//                             arrays that do not fit together
//   test_dupsets --gpu DIR    real files under DIR: the identifier job with
//                             checksums, then reclaim_report on a MemoryLibrary
//                             and a SqliteLibrary; the two must be equal to each
//                             other and to the sets expected from the files
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

static uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

template <typename F>
static bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// ---- no GPU: the shaping ------------------------------------------------------------------

static void test_cpu() {
  // ten rows whose ids are not their indices: id = 100 + 7 * index
  std::vector<FilePathRow> rows(10);
  for (size_t i = 0; i < rows.size(); ++i) {
    rows[i].id = (int32_t)(100 + 7 * i);
    rows[i].size_in_bytes = 1000 * (i + 1);
  }
  // sets in the order by reclaimable bytes: {2, 5, 9} of 3000 bytes (6000),
  // {0, 7} of 1000 (1000), {3, 4} of 0 bytes (0)
  const std::vector<int64_t> set_rep{2, 0, 3}, members{2, 5, 9, 0, 7, 3, 4};
  const std::vector<uint64_t> set_offsets{0, 3, 5, 7}, set_bytes{3000, 1000, 0};
  sdcas_sets_counts counts{};
  counts.files = 9, counts.sets = 3, counts.members = 7, counts.duplicate_files = 4;
  counts.reclaimable_bytes = 7000, counts.largest_set = 3;
  const ReclaimReport r = reclaim_report_from(rows, set_rep, set_offsets, set_bytes, members, counts);
  CHECK(r.sets.size() == 3, "%zu sets", r.sets.size());
  if (r.sets.size() == 3) {
    CHECK(r.sets[0].file_path_ids == (std::vector<int32_t>{114, 135, 163}), "set 0's ids");
    CHECK(r.sets[1].file_path_ids == (std::vector<int32_t>{100, 149}), "set 1's ids");
    CHECK(r.sets[2].file_path_ids == (std::vector<int32_t>{121, 128}), "set 2's ids");
    CHECK(r.sets[0].bytes == 3000 && r.sets[0].reclaimable_bytes == 6000, "set 0's bytes");
    CHECK(r.sets[1].bytes == 1000 && r.sets[1].reclaimable_bytes == 1000, "set 1's bytes");
    CHECK(r.sets[2].bytes == 0 && r.sets[2].reclaimable_bytes == 0, "set 2's bytes");
  }
  // the order is the arrays' own: nothing is re-sorted by the shaping
  uint64_t sum = 0, largest = 0, in_sets = 0;
  for (const auto& s : r.sets) {
    sum += s.reclaimable_bytes;
    in_sets += s.file_path_ids.size();
    largest = std::max<uint64_t>(largest, s.file_path_ids.size());
  }
  CHECK(sum == r.counts.reclaimable_bytes && in_sets == r.counts.members && largest == r.counts.largest_set &&
            r.counts.sets == r.sets.size() && r.counts.duplicate_files == in_sets - r.sets.size() &&
            r.counts.files == 9,
        "the totals are the counts handed in and agree with the sets");
  // the same sets in set_rep order
  const ReclaimReport q = reclaim_report_from(rows, {0, 2, 3}, {0, 2, 5, 7}, {1000, 3000, 0}, {0, 7, 2, 5, 9, 3, 4},
                                              counts);
  CHECK(q.sets.size() == 3 && q.sets[0] == r.sets[1] && q.sets[1] == r.sets[0] && q.sets[2] == r.sets[2],
        "the set_rep order holds the same sets");
  // reclaimable bytes wrap modulo 2^64, as the counts do
  const ReclaimReport w = reclaim_report_from(rows, {0}, {0, 3}, {0xC000000000000000ull}, {0, 1, 2}, counts);
  CHECK(w.sets.size() == 1 && w.sets[0].reclaimable_bytes == 0x8000000000000000ull, "2 * 0xC0.. wraps");

  // empty input: no rows, no sets; and rows without sets
  const sdcas_sets_counts zero{};
  CHECK(reclaim_report_from({}, {}, {0}, {}, {}, zero).sets.empty(), "no rows, offsets {0}");
  CHECK(reclaim_report_from({}, {}, {}, {}, {}, zero).sets.empty(), "no rows, no arrays");
  CHECK(reclaim_report_from(rows, {}, {0}, {}, {}, zero).sets.empty(), "rows without sets");
  CHECK(reclaim_report_from(rows, {}, {0}, {}, {}, zero).counts.sets == 0, "zero counts stay zero");

  // arrays that do not describe sets of these rows
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2}, {0, 3}, {}, {2, 5, 9}, counts); }), "set_bytes too short");
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2}, {0}, {3000}, {2, 5, 9}, counts); }), "offsets too short");
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2}, {0, 2}, {3000}, {2, 5, 9}, counts); }),
        "last offset is not the number of members");
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2}, {1, 3}, {3000}, {2, 5, 9}, counts); }),
        "first offset is not 0");
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2, 0}, {0, 3, 2}, {3000, 1}, {2, 5}, counts); }),
        "offsets that descend");
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2}, {0, 3}, {3000}, {2, 5, 10}, counts); }),
        "a member past the rows");
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2}, {0, 3}, {3000}, {2, -1, 9}, counts); }),
        "a negative member");
  CHECK(throws_invalid([&] { reclaim_report_from(rows, {2, 0}, {0, 3, 3}, {3000, 1}, {2, 5, 9}, counts); }),
        "an empty set");
}

// ---- GPU: real files, the job, then the report ----------------------------------------

static void write_bytes(const std::string& p, const std::string& b) {
  FILE* f = std::fopen(p.c_str(), "wb");
  if (!f || (!b.empty() && std::fwrite(b.data(), 1, b.size(), f) != b.size())) {
    std::fprintf(stderr, "cannot write %s\n", p.c_str());
    std::exit(2);
  }
  std::fclose(f);
}

static std::string content(uint64_t seed, size_t n) {
  std::string b(n, '\0');
  uint64_t x = seed;
  for (size_t i = 0; i < n; ++i) {
    if (i % 8 == 0) x = mix(x);
    b[i] = (char)(x >> (8 * (i % 8)));
  }
  return b;
}

static int test_gpu(const std::string& dir) {
  const std::string root = dir + "/loc";
  ::mkdir(root.c_str(), 0755);
  // four equal 3 KiB files (9 216 bytes to win back), two equal 150 KiB files
  // (153 600), three equal 100-byte files (200), and a 204 800-byte pair that
  // shares its cas_id while the byte at 20 000 (in no cas window) differs:
  // not a set. Singles and an empty file besides.
  const std::string small = content(1, 3072), mid = content(2, 150 * 1024), tiny = content(4, 100);
  std::string big = content(3, 204800);
  for (const char* nm : {"a1.bin", "a2.bin", "a3.bin", "a4.bin"}) write_bytes(root + "/" + nm, small);
  write_bytes(root + "/b1.bin", mid);
  write_bytes(root + "/b2.bin", mid);
  for (const char* nm : {"t1.bin", "t2.bin", "t3.bin"}) write_bytes(root + "/" + nm, tiny);
  write_bytes(root + "/c1.bin", big);
  big[20000] ^= 1;
  write_bytes(root + "/c2.bin", big);
  write_bytes(root + "/empty.bin", "");
  for (int k = 0; k < 6; ++k) write_bytes(root + "/u" + std::to_string(k) + ".dat", content(100 + k, 500 + 9000 * k));

  auto engine = Engine::open();
  const Location loc{1, root};
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

  std::map<std::string, int32_t> id_of;
  for (const FilePathRow& r : mem.file_paths) id_of[r.name] = r.id;
  const std::vector<FilePathRow> before = mem.file_paths;

  // expected: the group-by over the rows' two strings, ordered by reclaimable
  // bytes descending, ties by the first id
  std::vector<ReclaimReport::Set> want(3);
  want[0].file_path_ids = {id_of["b1"], id_of["b2"]};
  want[0].bytes = 150 * 1024, want[0].reclaimable_bytes = 150 * 1024;
  want[1].file_path_ids = {id_of["a1"], id_of["a2"], id_of["a3"], id_of["a4"]};
  want[1].bytes = 3072, want[1].reclaimable_bytes = 3 * 3072;
  want[2].file_path_ids = {id_of["t1"], id_of["t2"], id_of["t3"]};
  want[2].bytes = 100, want[2].reclaimable_bytes = 200;
  for (auto& s : want) std::sort(s.file_path_ids.begin(), s.file_path_ids.end());

  const ReclaimReport reports[2] = {reclaim_report(*engine, mem, 1), reclaim_report(*engine, *sql, 1)};
  for (int k = 0; k < 2; ++k) {
    const ReclaimReport& r = reports[k];
    CHECK(r.sets.size() == 3, "%d: %zu sets", k, r.sets.size());
    for (size_t s = 0; s < r.sets.size() && s < 3; ++s) CHECK(r.sets[s] == want[s], "%d: set %zu", k, s);
    CHECK(r.counts.sets == 3 && r.counts.members == 9 && r.counts.duplicate_files == 6 &&
              r.counts.reclaimable_bytes == 150 * 1024 + 3 * 3072 + 200 && r.counts.largest_set == 4,
          "%d: counts", k);
    // every row with both columns takes part: all files but the empty one
    CHECK(r.counts.files == mem.file_paths_with_checksum(1, "").size(), "%d: %llu files take part", k,
          (unsigned long long)r.counts.files);
  }
  CHECK(reports[0].sets == reports[1].sets, "the two libraries' reports differ");
  CHECK(mem.file_paths.size() == before.size(), "rows after");
  for (size_t i = 0; i < before.size() && i < mem.file_paths.size(); ++i)
    CHECK(before[i].object_id == mem.file_paths[i].object_id && before[i].cas_id == mem.file_paths[i].cas_id &&
              before[i].integrity_checksum == mem.file_paths[i].integrity_checksum,
          "row %d changed", before[i].id);
  // no rows: an empty report
  CHECK(reclaim_report(*engine, mem, 2).sets.empty(), "another location has no rows");
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
