// sdcas_io::read_identify (spacedrive_amd/host/cas_io.cpp), the GPU-free open
// helper of sdcas_identify_checksums: it stats first and opens only regular
// files. Built from cas_io.cpp alone (plain and ASan+UBSan).
//
//   test_identify_io DIR    DIR: an empty scratch directory
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <string>
#include <thread>
#include <vector>

#include "../../spacedrive_amd/host/cas_io.hpp"

using namespace sdcas_io;

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

static std::string write_file(const std::string& p, size_t n) {
  std::string b(n, '\0');
  for (size_t i = 0; i < n; ++i) b[i] = (char)(i * 131 + 7);
  FILE* f = std::fopen(p.c_str(), "wb");
  if (!f || (n && std::fwrite(b.data(), 1, n, f) != n)) std::exit(2);
  std::fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  const uint64_t kMax = 1 << 20;
  std::vector<uint8_t> buf(8192, 0xEE);

  // a FIFO without a writer: open(O_RDONLY) would block for ever. The call
  // runs on a worker thread; the test fails, not waits, if it has not
  // returned in 5 s.
  {
    const std::string fifo = dir + "/fifo";
    if (mkfifo(fifo.c_str(), 0600) != 0) return 2;
    IdentifyRead r;
    r.size = 99;
    std::packaged_task<int()> task([&] { return read_identify(fifo.c_str(), false, buf.data(), buf.size(), kMax, &r); });
    std::future<int> fut = task.get_future();
    std::thread th(std::move(task));
    if (fut.wait_for(std::chrono::seconds(5)) != std::future_status::ready) {
      std::fprintf(stderr, "FAIL: read_identify blocked on a FIFO\n");
      std::fflush(stderr);
      _exit(1);  // the worker is stuck in open(): no join
    }
    th.join();
    CHECK(fut.get() == 0, "FIFO status");
    CHECK(r.size == 0 && r.kind == kKindOther && r.fd < 0 && !r.opened && r.need == 0, "FIFO: size %llu kind %d",
          (unsigned long long)r.size, r.kind);
  }
  // the same with O_DIRECT asked for
  {
    IdentifyRead r;
    CHECK(read_identify((dir + "/fifo").c_str(), true, buf.data(), buf.size(), kMax, &r) == 0 && r.kind == kKindOther,
          "FIFO, direct");
  }
  // a directory, a missing path
  {
    IdentifyRead r;
    CHECK(read_identify(dir.c_str(), false, buf.data(), buf.size(), kMax, &r) == 0 && r.kind == kKindDir && r.fd < 0,
          "directory");
    CHECK(read_identify((dir + "/none").c_str(), false, buf.data(), buf.size(), kMax, &r) == ENOENT, "missing");
  }
  // regular files: empty, read whole, no room, handed over
  {
    IdentifyRead r;
    write_file(dir + "/empty", 0);
    CHECK(read_identify((dir + "/empty").c_str(), false, buf.data(), buf.size(), kMax, &r) == 0 && r.size == 0 &&
              r.kind == kKindRegular && r.opened && r.fd < 0 && r.need == 0,
          "empty file");
    const std::string want = write_file(dir + "/small", 5000);
    for (bool direct : {false, true}) {
      std::fill(buf.begin(), buf.end(), 0xEE);
      CHECK(read_identify((dir + "/small").c_str(), direct, buf.data(), buf.size(), kMax, &r) == 0 && r.size == 5000 &&
                r.need == 0 && r.fd < 0,
            "small file");
      CHECK(!std::memcmp(buf.data(), want.data(), 5000) && buf[5000] == 0xEE, "small file bytes (direct %d)", direct);
    }
    std::fill(buf.begin(), buf.end(), 0xEE);
    CHECK(read_identify((dir + "/small").c_str(), false, buf.data(), 4999, kMax, &r) == 0 && r.size == 5000 &&
              r.need == 5000 && r.fd < 0 && buf[0] == 0xEE,
          "no room: need %llu", (unsigned long long)r.need);
    CHECK(read_identify((dir + "/small").c_str(), false, buf.data(), buf.size(), 4999, &r) == 0 && r.size == 5000 &&
              r.fd >= 0 && buf[0] == 0xEE,
          "handed over");
    if (r.fd >= 0) {
      struct stat sb;
      CHECK(fstat(r.fd, &sb) == 0 && sb.st_size == 5000, "the descriptor handed over");
      close(r.fd);
    }
  }
  std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
