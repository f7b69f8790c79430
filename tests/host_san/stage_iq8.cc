// Host-only harness for the 8-bit row path of the staging half (amcpy_amd/csrc/amcx_upload.h: kinds kSrcCi8 / kSrcCu8 through
// classify_layout, stage_runs over memory and over a file, staged_elem_bytes), built by tests/test_iq8_host.py three ways --
//   g++ -O1 -g -fsanitize=address,undefined     g++ -O1 -g -fsanitize=thread     g++ -O2
// -- and run in the CPU suite.  No HIP, no GPU.  An 8-bit element is 2 bytes and goes up as it lies, so what staging must
// deliver is a byte copy of the first N samples of every row: random (S, K, N) containers with padded rows and padded snr
// blocks, random runs of frames (starting mid-container, ragged ends), 1 ... 8 threads, memory and file (at an odd byte
// offset: nothing promises a file's samples any alignment), and a file cut short, which must say EIO and nothing else.
//
//   stage_iq8 [seed]     exit code 0 and "STAGE_IQ8_OK ..." on success; any mismatch aborts with a message
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>

#include <string>

#include "../../amcpy_amd/csrc/amcx_upload.h"

namespace {

struct Rng {
  unsigned long long s;
  explicit Rng(unsigned long long seed) : s(seed * 2654435761ULL + 88172645463325252ULL) {}
  unsigned long long next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  int64_t range(int64_t lo, int64_t hi) { return lo + (int64_t)(next() % (unsigned long long)(hi - lo)); }   // [lo, hi)
};

[[noreturn]] void die(const char* what, int64_t a = 0, int64_t b = 0, int64_t c = 0) {
  fprintf(stderr, "stage_iq8: %s (%lld, %lld, %lld)\n", what, (long long)a, (long long)b, (long long)c);
  abort();
}

// the first N samples of frames [g0, g1) of the (S, K, L) container, copied byte by byte
std::vector<unsigned char> expect(const std::vector<unsigned char>& box, int64_t K, int64_t N, int64_t ss, int64_t sk, int64_t g0,
                                  int64_t g1) {
  std::vector<unsigned char> out;
  out.reserve((size_t)((g1 - g0) * N * 2));
  for (int64_t g = g0; g < g1; ++g) {
    const int64_t e = (g / K) * ss + (g % K) * sk;
    for (int64_t b = 0; b < 2 * N; ++b) out.push_back(box[(size_t)(2 * e + b)]);
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  Rng rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
  char path[] = "/tmp/stage_iq8_XXXXXX";
  const int tmp = mkstemp(path);
  if (tmp < 0) die("mkstemp");
  close(tmp);
  int64_t staged_bytes = 0;
  int cases = 0;
  for (int round = 0; round < 120; ++round) {
    const int kind = (round & 1) ? amcx::kSrcCu8 : amcx::kSrcCi8;
    if (!amcx::src_kind_ok(kind) || !amcx::src_iq8(kind) || !amcx::src_as_it_lies(kind)) die("kind predicates", kind);
    if (amcx::staged_elem_bytes(kind, false) != 2) die("staged_elem_bytes", kind);
    // a few rounds are large enough for parts of >= 256 KiB to be handed to several threads
    const bool big = round % 20 == 19;
    const int64_t S = rng.range(1, 4), K = rng.range(1, big ? 40 : 12), N = big ? rng.range(30000, 32769) : rng.range(2, 700);
    const int64_t sk = N + rng.range(0, 9), ss = K * sk + rng.range(0, 5);
    const int64_t elems = S * ss + 3;
    std::vector<unsigned char> box((size_t)(2 * elems));
    for (auto& b : box) b = (unsigned char)rng.next();
    bool rows = false, inner = false;
    amcx::RunMap map;
    if (!amcx::classify_layout(S, K, (int32_t)N, ss, sk, 1, &rows, &inner, &map) || !rows) die("classify_layout", S, K, N);
    const int64_t F = S * K;
    const int64_t g0 = rng.range(0, F), g1 = rng.range(g0, F + 1);
    const std::vector<unsigned char> want = expect(box, K, N, ss, sk, g0, g1);
    // the file: an odd number of bytes in front of the container
    const int64_t lead = 2 * rng.range(0, 40) + 1;
    {
      FILE* f = fopen(path, "wb");
      if (f == nullptr) die("fopen");
      const std::vector<unsigned char> pad((size_t)lead, 0x5a);
      if (fwrite(pad.data(), 1, pad.size(), f) != pad.size() || fwrite(box.data(), 1, box.size(), f) != box.size()) die("fwrite");
      fclose(f);
    }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) die("open");
    for (int threads = 1; threads <= 8; threads += (round % 3) + 1) {
      amcx::Pool pool;
      pool.resize(threads);
      for (int from_file = 0; from_file < 2; ++from_file) {
        std::atomic<int> io_error{0};
        amcx::Source src = from_file ? amcx::Source::file(fd, lead, 12345, kind)      // (an imaginary offset: dropped)
                                     : amcx::Source::memory(box.data(), box.data(), kind);
        if (src.has_im()) die("an interleaved kind kept an imaginary part");
        src.io_error = &io_error;
        std::vector<unsigned char> got(want.size() + 16, 0xee);
        amcx::stage_runs(pool, reinterpret_cast<char*>(got.data()), src, map, g0, g1, false);
        if (io_error.load() != 0) die("io_error", io_error.load());
        for (size_t i = 0; i < want.size(); ++i)
          if (got[i] != want[i]) die("staged byte differs", round, threads, (int64_t)i);
        for (size_t i = want.size(); i < got.size(); ++i)
          if (got[i] != 0xee) die("wrote behind the staged rows", round, threads, (int64_t)i);
        staged_bytes += (int64_t)want.size();
        ++cases;
      }
    }
    close(fd);
    // the file ends inside the last row that is asked for: EIO, whatever the thread count
    if (g1 > g0) {
      const int64_t last = ((g1 - 1) / K) * ss + ((g1 - 1) % K) * sk;
      if (truncate(path, (off_t)(lead + 2 * (last + N) - 1)) != 0) die("truncate");
      const int fd2 = open(path, O_RDONLY);
      if (fd2 < 0) die("open (short)");
      amcx::Pool pool;
      pool.resize((int)rng.range(1, 9));
      std::atomic<int> io_error{0};
      amcx::Source src = amcx::Source::file(fd2, lead, -1, kind);
      src.io_error = &io_error;
      std::vector<unsigned char> got(want.size(), 0);
      amcx::stage_runs(pool, reinterpret_cast<char*>(got.data()), src, map, g0, g1, false);
      if (io_error.load() != EIO) die("a short file did not say EIO", io_error.load());
      close(fd2);
    }
  }
  unlink(path);
  printf("STAGE_IQ8_OK %d cases, %lld bytes staged\n", cases, (long long)staged_bytes);
  return 0;
}
