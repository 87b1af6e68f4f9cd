// Duplicates confirmed by checksum (include/sdcore.hpp: duplicate_report_from,
// Library::file_paths_with_checksum, confirm_duplicates).
//
//   test_confirm              no GPU: file_paths_with_checksum on a MemoryLibrary
//                             and a SqliteLibrary(":memory:") over hand-built
//                             rows, and duplicate_report_from against a std::map
//                             group-by written here
//   test_confirm --gpu DIR    real files under DIR (identical sets, and a pair
//                             that shares its cas_id while one byte outside
//                             the cas windows differs): the identifier job with
//                             checksums links the pair to ONE Object, and
//                             confirm_duplicates reports it as a collision,
//                             on both libraries, writing nothing
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
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

static std::string synth_checksum(int v) {
  char h[65];
  for (int w = 0; w < 4; ++w) std::snprintf(h + 16 * w, 17, "%016llx", (unsigned long long)mix((uint64_t)v * 4 + w));
  return std::string(h, 64);
}

static bool same_row(const FilePathRow& a, const FilePathRow& b) {
  return a.id == b.id && a.pub_id == b.pub_id && a.location_id == b.location_id &&
         a.materialized_path == b.materialized_path && a.name == b.name && a.extension == b.extension &&
         a.is_dir == b.is_dir && a.size_in_bytes == b.size_in_bytes && a.cas_id == b.cas_id &&
         a.object_id == b.object_id && a.integrity_checksum == b.integrity_checksum &&
         a.date_created == b.date_created && a.kind == b.kind && a.inode == b.inode && a.hidden == b.hidden;
}

// ---- the checker: a std::map group-by over the rows' two strings ------------------

struct Expected {
  std::vector<std::pair<std::string, std::vector<int32_t>>> confirmed;  // cas_id + checksum, ids
  struct Collision {
    std::string cas_id;
    std::vector<std::vector<int32_t>> classes;
    std::vector<int32_t> object_ids;
  };
  std::vector<Collision> collisions;
  uint64_t counts[6] = {};
  std::vector<int64_t> rep, key_rep;
  std::vector<uint8_t> flags;
};

// rows in id order; skip[i]: the row takes no part
static Expected expect(const std::vector<FilePathRow>& rows, const std::vector<bool>& skip) {
  Expected e;
  std::map<std::pair<std::string, std::string>, std::vector<size_t>> classes;
  std::map<std::string, std::vector<size_t>> keys;
  for (size_t i = 0; i < rows.size(); ++i) {
    if (skip[i]) continue;
    classes[{*rows[i].cas_id, *rows[i].integrity_checksum}].push_back(i);
    keys[*rows[i].cas_id].push_back(i);
  }
  std::map<std::string, std::set<std::string>> sums;
  for (const auto& [k, m] : classes) sums[k.first].insert(k.second);
  const size_t n = rows.size();
  e.rep.assign(n, -1);
  e.key_rep.assign(n, -1);
  e.flags.assign(n, SDCAS_CONFIRM_SKIPPED);
  for (const auto& [k, m] : classes)
    for (size_t i : m) {
      e.rep[i] = (int64_t)m[0];
      e.key_rep[i] = (int64_t)keys[k.first][0];
      e.flags[i] = (uint8_t)((i != m[0] ? SDCAS_CONFIRM_DUPLICATE : 0) |
                             (sums[k.first].size() >= 2 ? SDCAS_CONFIRM_COLLISION : 0));
    }
  // ordered by first id: walk the rows
  for (size_t i = 0; i < n; ++i) {
    if (skip[i]) continue;
    const auto& m = classes[{*rows[i].cas_id, *rows[i].integrity_checksum}];
    if (m[0] == i && m.size() >= 2) {
      std::vector<int32_t> ids;
      for (size_t j : m) ids.push_back(rows[j].id);
      e.confirmed.push_back({*rows[i].cas_id + *rows[i].integrity_checksum, ids});
    }
    const auto& km = keys[*rows[i].cas_id];
    if (km[0] == i && sums[*rows[i].cas_id].size() >= 2) {
      Expected::Collision c;
      c.cas_id = *rows[i].cas_id;
      std::set<int32_t> objs;
      for (size_t j : km) {
        if (rows[j].object_id) objs.insert(*rows[j].object_id);
        const auto& cm = classes[{*rows[j].cas_id, *rows[j].integrity_checksum}];
        if (cm[0] != j) continue;
        std::vector<int32_t> ids;
        for (size_t q : cm) ids.push_back(rows[q].id);
        c.classes.push_back(ids);
      }
      c.object_ids.assign(objs.begin(), objs.end());
      e.collisions.push_back(c);
    }
  }
  for (size_t i = 0; i < n; ++i) e.counts[0] += !skip[i];
  e.counts[1] = classes.size();
  e.counts[2] = keys.size();
  for (const auto& [k, s] : sums)
    if (s.size() >= 2) {
      ++e.counts[3];
      e.counts[4] += keys[k].size();
    }
  e.counts[5] = e.counts[0] - e.counts[1];
  return e;
}

static void check_report(const char* what, const DuplicateReport& r, const Expected& e) {
  CHECK(r.confirmed.size() == e.confirmed.size(), "%s: %zu confirmed classes, expected %zu", what,
        r.confirmed.size(), e.confirmed.size());
  for (size_t i = 0; i < r.confirmed.size() && i < e.confirmed.size(); ++i) {
    CHECK(r.confirmed[i].cas_id + r.confirmed[i].checksum == e.confirmed[i].first, "%s: confirmed %zu: strings", what,
          i);
    CHECK(r.confirmed[i].file_path_ids == e.confirmed[i].second, "%s: confirmed %zu: ids", what, i);
  }
  CHECK(r.collisions.size() == e.collisions.size(), "%s: %zu collisions, expected %zu", what, r.collisions.size(),
        e.collisions.size());
  for (size_t i = 0; i < r.collisions.size() && i < e.collisions.size(); ++i) {
    CHECK(r.collisions[i].cas_id == e.collisions[i].cas_id, "%s: collision %zu: cas_id", what, i);
    CHECK(r.collisions[i].classes == e.collisions[i].classes, "%s: collision %zu: classes", what, i);
    CHECK(r.collisions[i].object_ids == e.collisions[i].object_ids, "%s: collision %zu: object ids", what, i);
  }
  const uint64_t got[6] = {r.counts.files,         r.counts.classes,        r.counts.keys,
                           r.counts.collided_keys, r.counts.collided_files, r.counts.duplicate_files};
  for (int k = 0; k < 6; ++k)
    CHECK(got[k] == e.counts[k], "%s: count %d is %llu, expected %llu", what, k, (unsigned long long)got[k],
          (unsigned long long)e.counts[k]);
}

// ---- no GPU -------------------------------------------------------------------------

struct Spec {
  int cas;       // < 0: no cas_id
  int checksum;  // < 0: no integrity_checksum
  int object;    // 0: none
  const char* dir;
  bool is_dir;
  int location;
};

// 31 rows: classes of 1, 2 and 3 rows; cas 1 collides with two classes (one of
// two rows) on two Objects, cas 4 with three classes on one Object; one
// checksum under two cas_ids (two classes, no collision); rows lacking either
// column, a directory, another location, and rows under /sub/
static const Spec kSpecs[] = {
    {1, 10, 1, "/", false, 1},      {2, 20, 2, "/", false, 1},     {1, 11, 1, "/", false, 1},
    {3, 30, 3, "/", false, 1},      {-1, 40, 0, "/", false, 1},    {2, 20, 4, "/", false, 1},
    {1, 10, 5, "/sub/", false, 1},  {4, 50, 6, "/", false, 1},     {5, -1, 7, "/", false, 1},
    {4, 51, 6, "/sub/", false, 1},  {4, 52, 6, "/", false, 1},     {6, 60, 0, "/", true, 1},
    {7, 30, 8, "/", false, 1},      {2, 20, 2, "/sub/", false, 1}, {1, 10, 1, "/", false, 2},
    {8, 80, 0, "/", false, 1},      {8, 80, 0, "/sub/x/", false, 1}, {-1, -1, 0, "/", false, 1},
    {9, 90, 9, "/", false, 1},      {9, 91, 0, "/", false, 1},     {10, 100, 0, "/", false, 1},
    {3, 30, 3, "/sub/", false, 1},  {11, 110, 0, "/sub/", false, 1}, {11, 110, 10, "/sub/", false, 1},
    {12, 120, 0, "/", false, 1},    {-1, 120, 0, "/sub/", false, 1}, {13, -1, 0, "/sub/", false, 1},
    {4, 50, 6, "/", false, 1},      {14, 140, 0, "/", false, 1},   {9, 90, 9, "/", false, 1},
    {15, 150, 0, "/", false, 1},
};

static std::vector<FilePathRow> hand_rows() {
  std::vector<FilePathRow> rows;
  int k = 0;
  for (const Spec& s : kSpecs) {
    FilePathRow r;
    r.location_id = s.location;
    r.materialized_path = s.dir;
    r.name = "f" + std::to_string(k);
    r.extension = "bin";
    r.is_dir = s.is_dir;
    r.size_in_bytes = 1000 + (uint64_t)k;
    r.date_created = 1700000000 + k;
    r.kind = k % 9;
    if (s.cas >= 0) r.cas_id = key_to_hex(mix((uint64_t)s.cas));
    if (s.checksum >= 0) r.integrity_checksum = synth_checksum(s.checksum);
    if (s.object) r.object_id = s.object;
    rows.push_back(r);
    ++k;
  }
  return rows;
}

// a Library that overrides none of the optional queries
struct BareLibrary : Library {
  size_t count_orphan_file_paths(int32_t, const std::string&) override { return 0; }
  std::vector<FilePathRow> get_orphan_file_paths(int32_t, int32_t, const std::string&, size_t) override { return {}; }
  size_t count_orphan_file_paths_in_dir(int32_t, const std::string&) override { return 0; }
  std::vector<FilePathRow> get_orphan_file_paths_in_dir(int32_t, int32_t, const std::string&, size_t) override {
    return {};
  }
  void set_cas_id(int32_t, const std::optional<std::string>&) override {}
  std::vector<std::pair<int32_t, std::vector<std::string>>> existing_objects(const std::vector<std::string>&) override {
    return {};
  }
  int32_t create_object(ObjectKind, int64_t) override { return 0; }
  void connect(int32_t, int32_t) override {}
  std::vector<FilePathRow> file_paths_without_checksum(int32_t, const std::string&) override { return {}; }
  void set_integrity_checksum(int32_t, const std::string&) override {}
};

static void test_cpu() {
  MemoryLibrary mem;
  auto sql = SqliteLibrary::open(":memory:");
  for (int o = 0; o < 10; ++o) {
    mem.create_object(ObjectKindUnknown, 1700000000 + o);
    sql->create_object(ObjectKindUnknown, 1700000000 + o);
  }
  std::vector<FilePathRow> rows = hand_rows();
  for (const FilePathRow& r : rows) mem.add_file_path(r);
  sql->add_file_paths(rows);  // assigns the ids MemoryLibrary assigned: 1, 2, ...
  CHECK(rows.size() >= 30 && rows.back().id == (int32_t)rows.size(), "ids");

  for (const char* sub : {"", "/sub/", "/sub/x/", "/none/"}) {
    std::vector<int32_t> want;
    for (const FilePathRow& r : mem.file_paths)
      if (r.location_id == 1 && !r.is_dir && r.cas_id && r.integrity_checksum &&
          r.materialized_path.compare(0, std::strlen(sub), sub) == 0)
        want.push_back(r.id);
    const auto a = mem.file_paths_with_checksum(1, sub);
    const auto b = sql->file_paths_with_checksum(1, sub);
    CHECK(a.size() == want.size() && b.size() == want.size(), "sub '%s': %zu / %zu rows, expected %zu", sub, a.size(),
          b.size(), want.size());
    for (size_t i = 0; i < a.size() && i < b.size() && i < want.size(); ++i) {
      CHECK(a[i].id == want[i], "sub '%s': row %zu is id %d, expected %d", sub, i, a[i].id, want[i]);
      CHECK(same_row(a[i], b[i]), "sub '%s': row %zu differs between the libraries (ids %d / %d)", sub, i, a[i].id,
            b[i].id);
    }
  }
  CHECK(mem.file_paths_with_checksum(1, "").size() == 24, "the hand-built rows select %zu",
        mem.file_paths_with_checksum(1, "").size());
  CHECK(mem.file_paths_with_checksum(2, "").size() == 1, "location 2");
  bool threw = false;
  try {
    BareLibrary bare;
    bare.file_paths_with_checksum(1, "");
  } catch (const LibraryError&) {
    threw = true;
  }
  CHECK(threw, "the default file_paths_with_checksum must throw LibraryError");

  // the report's shaping, on both libraries' rows
  for (Library* db : {(Library*)&mem, (Library*)sql.get()}) {
    const auto sel = db->file_paths_with_checksum(1, "");
    const Expected e = expect(sel, std::vector<bool>(sel.size(), false));
    const DuplicateReport r = duplicate_report_from(sel, e.rep, e.key_rep, e.flags);
    check_report("all rows", r, e);
    CHECK(r.confirmed.size() == 7 && r.collisions.size() == 3, "%zu confirmed, %zu collisions", r.confirmed.size(),
          r.collisions.size());
    if (r.collisions.size() == 3) {
      CHECK(r.collisions[0].classes.size() == 2 && r.collisions[0].object_ids == (std::vector<int32_t>{1, 5}),
            "cas 1: two classes on Objects 1 and 5");
      CHECK(r.collisions[1].classes.size() == 3 && r.collisions[1].object_ids == (std::vector<int32_t>{6}),
            "cas 4: three classes on Object 6");
      CHECK(r.collisions[2].classes.size() == 2 && r.collisions[2].object_ids == (std::vector<int32_t>{9}),
            "cas 9: two classes, one row without an Object");
    }
    // rows the group-by skipped (every third, among them classes' and keys'
    // first rows) appear nowhere
    std::vector<bool> skip(sel.size());
    for (size_t i = 0; i < sel.size(); ++i) skip[i] = i % 3 == 0;
    const Expected es = expect(sel, skip);
    check_report("every third row skipped", duplicate_report_from(sel, es.rep, es.key_rep, es.flags), es);
  }
  // no rows
  const DuplicateReport none = duplicate_report_from({}, {}, {}, {});
  CHECK(none.confirmed.empty() && none.collisions.empty() && none.counts.files == 0, "empty report");
  bool bad = false;
  try {
    duplicate_report_from(mem.file_paths_with_checksum(1, ""), {}, {}, {});
  } catch (const std::invalid_argument&) {
    bad = true;
  }
  CHECK(bad, "lengths that differ must throw");
}

// ---- GPU: real files, the job, then the report ------------------------------------------

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

static bool late(const FilePathRow& r) { return r.materialized_path.compare(0, 6, "/late/") == 0; }

static std::vector<FilePathRow> all_rows(MemoryLibrary& db) { return db.file_paths; }
static std::vector<FilePathRow> all_rows(SqliteLibrary& db, size_t n) {
  std::vector<FilePathRow> out;
  for (size_t id = 1; id <= n; ++id) {
    auto r = db.file_path((int32_t)id);
    if (r) out.push_back(*r);
  }
  return out;
}

static int test_gpu(const std::string& dir) {
  const std::string root = dir + "/loc";
  ::mkdir(root.c_str(), 0755);
  ::mkdir((root + "/late").c_str(), 0755);
  // three identical 3 KiB files (a fourth arrives later), two identical 150 KiB
  // files, and the colliding pair: 204 800 bytes, equal except for the byte at
  // 20 000, which lies in no cas window (header to 8192, samples at 8192,
  // 55 296, 102 400 and 149 504 of 10 240 bytes, footer from 196 608)
  const std::string small = content(1, 3072), mid = content(2, 150 * 1024);
  std::string big = content(3, 204800);
  for (const char* nm : {"a1.bin", "a2.bin", "a3.bin", "late/a4.bin"}) write_bytes(root + "/" + nm, small);
  write_bytes(root + "/b1.bin", mid);
  write_bytes(root + "/b2.bin", mid);
  write_bytes(root + "/c1.bin", big);
  big[20000] ^= 1;
  write_bytes(root + "/late/c2.bin", big);
  write_bytes(root + "/empty.bin", "");
  for (int k = 0; k < 10; ++k) write_bytes(root + "/u" + std::to_string(k) + ".dat", content(100 + k, 500 + 9000 * k));
  write_bytes(root + "/late/u10.dat", content(200, 120000));

  auto engine = Engine::open();
  const Location loc{1, root};
  MemoryLibrary mem;
  auto sql = SqliteLibrary::open(dir + "/library.db");
  std::vector<FilePathRow> first, second;
  for (FilePathRow r : walk_location(loc)) {
    r.location_id = 1;
    (late(r) ? second : first).push_back(r);
  }
  CHECK(first.size() >= 18 && second.size() == 3, "%zu + %zu rows", first.size(), second.size());
  // the job twice: the files under late/ are indexed after the first run, so
  // their step finds the Objects of the first (rows of ONE step each get an
  // Object of their own, mod.rs:246-254)
  FileIdentifierJobInit init{loc, "", 100};
  init.checksums = true;
  for (auto* part : {&first, &second}) {
    for (const FilePathRow& r : *part) mem.add_file_path(r);
    sql->add_file_paths(*part);
    run_file_identifier_job(*engine, mem, init);
    run_file_identifier_job(*engine, *sql, init);
  }
  const size_t total = mem.file_paths.size();
  const std::vector<FilePathRow> mem_before = all_rows(mem), sql_before = all_rows(*sql, total);
  CHECK(sql_before.size() == total, "sqlite holds %zu rows, memory %zu", sql_before.size(), total);
  std::map<std::string, int32_t> id_of;
  for (size_t i = 0; i < total && i < sql_before.size(); ++i) {
    CHECK(same_row(mem_before[i], sql_before[i]), "row %d differs between the libraries after the jobs",
          mem_before[i].id);
    id_of[mem_before[i].name] = mem_before[i].id;
  }
  const FilePathRow* c1 = mem.file_path(id_of["c1"]);
  const FilePathRow* c2 = mem.file_path(id_of["c2"]);
  CHECK(c1 && c2 && c1->cas_id && c2->cas_id && *c1->cas_id == *c2->cas_id, "the pair's cas_ids must be equal");
  CHECK(c1 && c2 && c1->integrity_checksum && c2->integrity_checksum &&
            *c1->integrity_checksum != *c2->integrity_checksum,
        "the pair's checksums must differ");
  CHECK(c1 && c2 && c1->object_id && c1->object_id == c2->object_id, "the job links the pair to ONE Object");

  DuplicateReport reports[2];
  reports[0] = confirm_duplicates(*engine, mem, 1);
  reports[1] = confirm_duplicates(*engine, *sql, 1);
  const std::vector<FilePathRow> mem_after = all_rows(mem), sql_after = all_rows(*sql, total);
  CHECK(mem_after.size() == total && sql_after.size() == total, "rows after");
  for (size_t i = 0; i < total && i < mem_after.size() && i < sql_after.size(); ++i) {
    CHECK(same_row(mem_before[i], mem_after[i]), "memory row %d changed", mem_before[i].id);
    CHECK(same_row(sql_before[i], sql_after[i]), "sqlite row %d changed", sql_before[i].id);
  }
  const auto sel = mem.file_paths_with_checksum(1, "");
  const Expected e = expect(sel, std::vector<bool>(sel.size(), false));
  CHECK(sel.size() == total - 2, "%zu rows with both columns of %zu (the directory and the empty file lack one)",
        sel.size(), total);
  for (int k = 0; k < 2; ++k) {
    const DuplicateReport& r = reports[k];
    check_report(k ? "sqlite" : "memory", r, e);
    CHECK(r.collisions.size() == 1, "%d: %zu collisions", k, r.collisions.size());
    if (r.collisions.size() == 1 && c1 && c2) {
      const auto& c = r.collisions[0];
      CHECK(c.cas_id == *c1->cas_id, "%d: the collision's cas_id", k);
      CHECK(c.classes == (std::vector<std::vector<int32_t>>{{c1->id}, {c2->id}}), "%d: the collision's classes", k);
      CHECK(c.object_ids == (std::vector<int32_t>{*c1->object_id}), "%d: the collision's Object", k);
    }
    CHECK(r.confirmed.size() == 2, "%d: %zu confirmed classes", k, r.confirmed.size());
    if (r.confirmed.size() == 2) {
      CHECK(r.confirmed[0].file_path_ids ==
                (std::vector<int32_t>{id_of["a1"], id_of["a2"], id_of["a3"], id_of["a4"]}),
            "%d: the 3 KiB set", k);
      CHECK(r.confirmed[1].file_path_ids == (std::vector<int32_t>{id_of["b1"], id_of["b2"]}), "%d: the 150 KiB set",
            k);
    }
    CHECK(r.counts.collided_keys == 1 && r.counts.collided_files == 2 && r.counts.duplicate_files == 4, "%d: counts",
          k);
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
