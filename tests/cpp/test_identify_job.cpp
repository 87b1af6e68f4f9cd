// The identifier job that also fills integrity_checksum
// (FileIdentifierJobInit::checksums, include/sdcore.hpp).
// TEST INFRASTRUCTURE: links oracle/build/liboracle.so as the checker.
//
//   test_identify_job              no GPU: the flag over a synthetic MetadataFn
//                                  that carries checksums, the oracle as group-by
//   test_identify_job --gpu DIR    a location of ~300 small files under DIR: the
//                                  job with checksums = true against the job
//                                  followed by run_object_validator_job
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../oracle/oracle.h"
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

static GroupBy oracle_group_by(size_t chunk_size) {
  return [chunk_size](const std::vector<uint64_t>& k, const std::vector<uint8_t>& h, const std::vector<int32_t>& st,
                      const std::vector<uint64_t>& e, sdcas_job_window& w) {
    Engine::Dedup d;
    d.link.assign(k.size(), 0);
    int64_t linked = 0;
    oracle_job_window ow{w.max_steps, (int32_t)w.more, 0, 0, 0, 0};
    d.created = oracle_identifier_job(k.size(), k.data(), h.data(), st.data(), chunk_size, e.size(),
                                      e.empty() ? nullptr : e.data(), &ow, d.link.data(), &linked);
    d.linked = linked;
    w.steps = ow.steps;
    w.rows = ow.rows;
    w.rereads = ow.rereads;
    return d;
  };
}

static bool same_row(const FilePathRow& a, const FilePathRow& b, bool with_checksum = true) {
  return a.id == b.id && a.pub_id == b.pub_id && a.location_id == b.location_id &&
         a.materialized_path == b.materialized_path && a.name == b.name && a.extension == b.extension &&
         a.is_dir == b.is_dir && a.size_in_bytes == b.size_in_bytes && a.cas_id == b.cas_id &&
         a.object_id == b.object_id && (!with_checksum || a.integrity_checksum == b.integrity_checksum) &&
         a.date_created == b.date_created && a.kind == b.kind && a.inode == b.inode && a.hidden == b.hidden;
}

// ---- no GPU: the flag ---------------------------------------------------------

static std::string synth_checksum(int32_t id) {
  char h[65];
  for (int w = 0; w < 4; ++w) std::snprintf(h + 16 * w, 17, "%016llx", (unsigned long long)mix((uint64_t)id * 4 + w));
  return std::string(h, 64);
}

// FileMetadata per row: duplicates in and across steps, I/O errors, and rows
// without cas_id — among them row 100, the first step's last row, which the
// second step reads again
static std::vector<Result<FileMetadata>> make_metadata(const std::vector<FilePathRow>& rows, bool checksums) {
  std::vector<Result<FileMetadata>> md;
  for (const auto& r : rows) {
    if (r.id % 37 == 5) {
      md.emplace_back(IoError{ENOENT, r.name});
      continue;
    }
    FileMetadata m;
    m.kind = r.kind;
    m.len = r.size_in_bytes;
    if (r.id % 100 != 0 && r.id % 53 != 7) m.cas_id = key_to_hex(mix((uint64_t)r.id % 180));
    if (checksums) m.integrity_checksum = synth_checksum(r.id);
    md.emplace_back(m);
  }
  return md;
}

static void fill(MemoryLibrary& db, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    FilePathRow r;
    r.location_id = 1;
    r.name = "f" + std::to_string(i);
    r.extension = "bin";
    r.size_in_bytes = 1 + i;
    r.date_created = (int64_t)(1700000000 + i);
    r.kind = (int32_t)(i % 9);
    db.add_file_path(r);
  }
}

static FileIdentifierJobRunMetadata run(MemoryLibrary& db, size_t batch, bool flag, bool md_checksums) {
  FileIdentifierJobInit init{Location{1, "/nowhere"}, "", batch};
  init.checksums = flag;
  return run_file_identifier_job_with(
      db, init, [&](const std::vector<FilePathRow>& rows) { return make_metadata(rows, md_checksums); },
      oracle_group_by(100));
}

static void test_flag() {
  for (size_t batch : {size_t(100), size_t(250), size_t(10000)}) {
    MemoryLibrary today, clear, set;
    fill(today, 450);
    fill(clear, 450);
    fill(set, 450);
    const auto mt = run(today, batch, false, false);  // the job as it was: no checksum anywhere
    const auto mc = run(clear, batch, false, true);   // metadata carries checksums, the flag is clear
    const auto ms = run(set, batch, true, true);
    CHECK(mt.rereads > 0, "batch %zu: no step read a row again", batch);
    CHECK(mt.steps == mc.steps && mt.steps == ms.steps && mt.total_objects_created == ms.total_objects_created &&
              mt.total_objects_linked == ms.total_objects_linked && mt.rereads == ms.rereads,
          "batch %zu: the jobs ran different steps", batch);
    CHECK(today.objects.size() == clear.objects.size() && today.objects.size() == set.objects.size(),
          "batch %zu: Object counts differ", batch);
    size_t with = 0;
    for (size_t i = 0; i < today.file_paths.size(); ++i) {
      const FilePathRow &t = today.file_paths[i], &c = clear.file_paths[i], &s = set.file_paths[i];
      CHECK(same_row(t, c), "batch %zu row %d: the flag clear changed the library", batch, t.id);
      CHECK(same_row(t, s, false), "batch %zu row %d: the flag changed more than the checksum", batch, t.id);
      // a step read the row iff it has an Object now (a row with a cas_id is
      // linked, one without gets an Object from every step that reads it; a
      // failed row is dropped)
      const bool read = s.object_id.has_value();
      CHECK(read == (s.id % 37 != 5), "batch %zu row %d: read by no step", batch, s.id);
      if (read) {
        CHECK(s.integrity_checksum && *s.integrity_checksum == synth_checksum(s.id), "batch %zu row %d: checksum", batch,
              s.id);
        ++with;
      } else {
        CHECK(!s.integrity_checksum, "batch %zu row %d: a checksum on a row no step read", batch, s.id);
      }
    }
    CHECK(with > 400, "batch %zu: %zu rows with a checksum", batch, with);
    CHECK(set.file_paths[99].id == 100 && !set.file_paths[99].cas_id && set.file_paths[99].integrity_checksum,
          "batch %zu: the reread row", batch);
  }
}

// ---- GPU: the job with checksums against job + validator --------------------------

static void write_file(const std::string& p, std::mt19937_64& g, size_t n) {
  std::string b(n, '\0');
  for (size_t i = 0; i < n; ++i) b[i] = (char)(g() >> 56);
  FILE* f = std::fopen(p.c_str(), "wb");
  if (!f || (n && std::fwrite(b.data(), 1, n, f) != n)) {
    std::fprintf(stderr, "cannot write %s\n", p.c_str());
    std::exit(2);
  }
  std::fclose(f);
}

static void copy_file(const std::string& from, const std::string& to) {
  FILE* a = std::fopen(from.c_str(), "rb");
  FILE* b = std::fopen(to.c_str(), "wb");
  if (!a || !b) std::exit(2);
  char buf[65536];
  size_t r;
  while ((r = std::fread(buf, 1, sizeof buf, a)) > 0) std::fwrite(buf, 1, r, b);
  std::fclose(a);
  std::fclose(b);
}

static int test_gpu(const std::string& dir) {
  std::mt19937_64 g(11);
  ::mkdir((dir + "/sub").c_str(), 0755);
  // 1..100 KiB mostly, the lengths around the kernel's branches, one above
  // 100 KiB, one streamed, an empty file, a few duplicates
  const size_t special[] = {0, 1, 56, 57, 1016, 1017, 1024, 102400, 102401, 300000, (1u << 20) + 9};
  size_t k = 0;
  for (size_t s : special) write_file(dir + "/s" + std::to_string(k++) + ".bin", g, s);
  for (size_t i = 0; i < 285; ++i)
    write_file(dir + (i % 5 == 0 ? "/sub/r" : "/r") + std::to_string(i) + ".dat", g, 1 + g() % 40000);
  copy_file(dir + "/r1.dat", dir + "/dup_a.dat");
  copy_file(dir + "/r1.dat", dir + "/sub/dup_b.dat");
  copy_file(dir + "/s7.bin", dir + "/dup_c.bin");
  copy_file(dir + "/s0.bin", dir + "/empty2.bin");

  auto engine = Engine::open();
  const Location loc{1, dir};
  MemoryLibrary fused, split;
  for (MemoryLibrary* db : {&fused, &split})
    for (FilePathRow r : walk_location(loc)) {
      r.location_id = 1;
      db->add_file_path(r);
    }
  CHECK(fused.file_paths.size() >= 300, "%zu rows", fused.file_paths.size());
  for (size_t batch : {size_t(100)}) {
    FileIdentifierJobInit a{loc, "", batch};
    a.checksums = true;
    const auto ma = run_file_identifier_job(*engine, fused, a);
    FileIdentifierJobInit b{loc, "", batch};
    const auto mb = run_file_identifier_job(*engine, split, b);
    const auto vr = run_object_validator_job(*engine, split, ObjectValidatorJobInit{loc, "", 100});
    CHECK(!vr.error, "validator: %s", vr.error ? vr.error->message().c_str() : "");
    CHECK(ma.steps == mb.steps && ma.total_objects_created == mb.total_objects_created &&
              ma.total_objects_linked == mb.total_objects_linked,
          "the jobs ran different steps");
    // dup_c.bin and sub/dup_b.dat sit in other steps than their originals and
    // link; dup_a.dat shares r1.dat's step, where duplicates each get an Object
    // (mod.rs:246-254)
    CHECK(ma.total_objects_linked >= 2, "duplicates linked: %zu", ma.total_objects_linked);
  }
  CHECK(fused.objects.size() == split.objects.size(), "Objects %zu != %zu", fused.objects.size(),
        split.objects.size());
  size_t files = 0;
  for (size_t i = 0; i < fused.file_paths.size(); ++i) {
    const FilePathRow &x = fused.file_paths[i], &y = split.file_paths[i];
    CHECK(same_row(x, y), "row %d (%s): cas_id %s / %s, object %d / %d, checksum %s / %s", x.id, x.name.c_str(),
          x.cas_id ? x.cas_id->c_str() : "-", y.cas_id ? y.cas_id->c_str() : "-", x.object_id.value_or(0),
          y.object_id.value_or(0), x.integrity_checksum ? x.integrity_checksum->c_str() : "-",
          y.integrity_checksum ? y.integrity_checksum->c_str() : "-");
    if (!x.is_dir) {
      ++files;
      // (a file indexed as empty is no orphan: it gets no Object, only its checksum)
      CHECK(x.integrity_checksum.has_value() && (x.object_id.has_value() || x.size_in_bytes == 0),
            "row %d (%s): not complete", x.id, x.name.c_str());
    }
  }
  CHECK(files >= 300, "%zu files", files);
  return failures;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--gpu")) {
    const int f = test_gpu(argv[2]);
    std::printf(f ? "FAILED %d\n" : "ok\n", f);
    return f ? 1 : 0;
  }
  test_flag();
  std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
