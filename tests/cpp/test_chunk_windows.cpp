// Chunk windows in the C++ mirror (include/sdcore.hpp: Engine::chunk_windows,
// plan_chunk_windows, merge_chunk_windows, similarity_report_streamed).
//
//   test_chunk_windows              no GPU: the window planner on lists of
//                                   sizes, and the merge of hand-made windows
//                                   (what it gives and what it refuses)
//   test_chunk_windows --gpu DIR W  the files under DIR/loc (made by the caller):
//                                   similarity_report_streamed with windows of W
//                                   bytes must equal similarity_report, pairs and
//                                   both counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

using Plan = std::vector<WindowPlan>;

static void test_planner() {
  CHECK(plan_chunk_windows({}, 100).empty(), "no files, no windows");
  CHECK((plan_chunk_windows({10, 20, 30}, 100) == Plan{{0, 3, false}}), "all fit in one window");
  CHECK((plan_chunk_windows({60, 40, 1}, 100) == Plan{{0, 2, false}, {2, 1, false}}), "a window filled exactly");
  CHECK((plan_chunk_windows({60, 41}, 100) == Plan{{0, 1, false}, {1, 1, false}}), "one byte too many");
  CHECK((plan_chunk_windows({100}, 100) == Plan{{0, 1, false}}), "a file of exactly the window is whole");
  CHECK((plan_chunk_windows({101}, 100) == Plan{{0, 1, true}}), "one byte more is streamed");
  CHECK((plan_chunk_windows({10, 500, 20, 30, 700, 0}, 100) ==
         Plan{{0, 1, false}, {1, 1, true}, {2, 2, false}, {4, 1, true}, {5, 1, false}}),
        "streamed files stand alone, in order");
  CHECK((plan_chunk_windows({0, 0, 0}, 1) == Plan{{0, 3, false}}), "empty files share a window");
  CHECK((plan_chunk_windows({500, 600}, 100) == Plan{{0, 1, true}, {1, 1, true}}), "two streamed files");
  CHECK((plan_chunk_windows({~0ull, 5}, ~0ull) == Plan{{0, 1, false}, {1, 1, false}}), "no sum wraps");
  CHECK(throws_invalid([] { plan_chunk_windows({1}, 0); }), "a window of no bytes");
}

// a window of files first..first + lens.size(), file f with `per[f]` chunks of 10 bytes
static ChunkWindow window(size_t first, uint64_t pos, const std::vector<uint32_t>& per, uint64_t key0, bool final = true) {
  ChunkWindow w;
  w.first_file = first, w.file_pos = pos;
  uint64_t at = 0;
  for (size_t f = 0; f < per.size(); ++f) {
    w.offsets.push_back(at);
    for (uint32_t k = 0; k < per[f]; ++k) {
      w.chunks.chunk_file.push_back((uint32_t)f);
      w.chunks.chunk_off.push_back(at + 10 * k);
      w.chunks.chunk_len.push_back(10);
      w.chunks.keys.push_back(key0++);
      w.chunks.digests.insert(w.chunks.digests.end(), 32, (uint8_t)key0);
    }
    w.chunks.consumed.push_back(10ull * per[f]);
    at += 10ull * per[f] + 16;
    w.chunks.counts.chunks += per[f];
    w.chunks.counts.total_bytes += 10ull * per[f];
    w.chunks.counts.files += final;
    w.chunks.counts.hash_cuts += per[f];
  }
  return w;
}

static void test_merge() {
  // files 0,1 whole in one window; file 2 streamed over three; files 3,4 (4 empty) in one
  const std::vector<ChunkWindow> ws{window(0, 0, {2, 1}, 100),        window(2, 0, {3}, 200, false),
                                    window(2, 30, {2}, 300, false), window(2, 50, {1}, 400),
                                    window(3, 0, {1, 0}, 500)};
  std::vector<uint64_t> sizes;
  const Engine::Chunks c = merge_chunk_windows(ws, 5, &sizes);
  CHECK((c.file_chunks == std::vector<uint64_t>{0, 2, 3, 9, 10, 10}), "file_chunks");
  CHECK((c.chunk_file == std::vector<uint32_t>{0, 0, 1, 2, 2, 2, 2, 2, 2, 3}), "chunk_file");
  CHECK((c.chunk_off == std::vector<uint64_t>{0, 10, 0, 0, 10, 20, 30, 40, 50, 0}), "offsets in the file");
  CHECK((c.keys == std::vector<uint64_t>{100, 101, 102, 200, 201, 202, 300, 301, 400, 500}), "keys in order");
  CHECK(c.digests.size() == 320 && c.digests[32 * 3] == (uint8_t)201, "digests in order");
  CHECK((sizes == std::vector<uint64_t>{20, 10, 60, 10, 0}), "the bytes consumed of each file");
  CHECK(c.counts.chunks == 10 && c.counts.files == 5 && c.counts.total_bytes == 100 && c.counts.hash_cuts == 10,
        "the counts summed: %llu chunks, %llu files", (unsigned long long)c.counts.chunks,
        (unsigned long long)c.counts.files);
  const Engine::Chunks none = merge_chunk_windows({}, 3, &sizes);
  CHECK((none.file_chunks == std::vector<uint64_t>{0, 0, 0, 0}) && none.chunk_off.empty() && sizes.size() == 3, "no windows");
  // refused
  CHECK(throws_invalid([&] { merge_chunk_windows({ws[4], ws[0]}, 5); }), "a window that goes back");
  CHECK(throws_invalid([&] { merge_chunk_windows({ws[0], window(1, 0, {1}, 1)}, 5); }), "a file given twice");
  CHECK(throws_invalid([&] { merge_chunk_windows({ws[1], ws[3], ws[2]}, 5); }), "a streamed file's windows out of order");
  CHECK(throws_invalid([&] { merge_chunk_windows({ws[4]}, 4); }), "a file past n_files");
  CHECK(throws_invalid([&] { merge_chunk_windows({window(0, 5, {1, 1}, 1)}, 5); }), "two files inside a file");
  ChunkWindow bad = ws[0];
  bad.chunks.keys.pop_back();
  CHECK(throws_invalid([&] { merge_chunk_windows({bad}, 5); }), "keys shorter than the chunks");
  bad = ws[0];
  bad.chunks.chunk_file[0] = 1;
  CHECK(throws_invalid([&] { merge_chunk_windows({bad}, 5); }), "chunks not in file order");
  bad = ws[0];
  bad.chunks.chunk_file[2] = 2;
  CHECK(throws_invalid([&] { merge_chunk_windows({bad}, 5); }), "a chunk of a file the window does not hold");
  bad = ws[0];
  bad.chunks.consumed.pop_back();
  CHECK(throws_invalid([&] { merge_chunk_windows({bad}, 5); }), "consumed shorter than the files");
}

static int test_gpu(const std::string& dir, uint64_t window_bytes) {
  auto engine = Engine::open();
  const Location loc{1, dir + "/loc"};
  MemoryLibrary mem;
  for (FilePathRow r : walk_location(loc)) {
    r.location_id = 1;
    mem.add_file_path(r);
  }
  const SimilarityReport want = similarity_report(*engine, mem, loc);
  const SimilarityReport got = similarity_report_streamed(*engine, mem, loc, "", window_bytes);
  CHECK(got.pairs == want.pairs, "the pairs differ: %zu and %zu", got.pairs.size(), want.pairs.size());
  CHECK(!memcmp(&got.chunks, &want.chunks, sizeof want.chunks), "the chunk counts differ");
  CHECK(!memcmp(&got.counts, &want.counts, sizeof want.counts), "the sharing counts differ");
  CHECK(similarity_report_streamed(*engine, mem, Location{2, loc.path}).pairs.empty(), "another location has no rows");
  std::printf("pairs %zu chunks %llu\n", got.pairs.size(), (unsigned long long)got.chunks.chunks);
  return failures;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--gpu")) {
    const int f = test_gpu(argv[2], std::strtoull(argv[3], nullptr, 10));
    std::printf(f ? "FAILED %d\n" : "ok\n", f);
    return f ? 1 : 0;
  }
  test_planner();
  test_merge();
  std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
