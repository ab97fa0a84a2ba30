// gather_walk_check.cpp -- the block walk of the gather kernels
// (csrc/sha1_gather_walk.h) run on the CPU, built with
// -fsanitize=address,undefined (make gather_walk_check;
// tests/test_gather_walk_host.py runs it as a child process).
//
// Every segment is a heap allocation of exactly its own size, so a read one
// byte outside a listed segment is an AddressSanitizer report.  The blocks the
// walk assembles must equal the concatenation of the segments, the tail and
// the total length included.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sha1_gather_walk.h"

using namespace btsha1;

namespace {

struct Sink {
  std::vector<uint8_t> out;
  void fence() {}
  void block(const uint32_t (&w)[16]) {
    for (int k = 0; k < 16; ++k)
      for (int b = 0; b < 4; ++b) out.push_back((uint8_t)(w[k] >> (24 - 8 * b)));
  }
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint8_t)(g_rng >> 56);
}

int g_failed = 0, g_cases = 0;

// One message whose segments have these lengths, listed in this order; the
// allocations are made in `order` (a permutation, so address order differs
// from list order).
void run(const char *name, const std::vector<uint32_t> &lens, bool reverse_alloc = false) {
  ++g_cases;
  const size_t n = lens.size();
  std::vector<uint8_t *> ptr(n, nullptr);
  std::vector<uint8_t> want;
  std::vector<std::vector<uint8_t>> bytes(n);
  for (size_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < lens[i]; ++k) {
      bytes[i].push_back(next_byte());
      want.push_back(bytes[i].back());
    }
  for (size_t t = 0; t < n; ++t) {
    const size_t i = reverse_alloc ? n - 1 - t : t;
    if (!lens[i]) continue;
    ptr[i] = (uint8_t *)malloc(lens[i]);
    memcpy(ptr[i], bytes[i].data(), lens[i]);
  }
  uint8_t *base = nullptr;
  for (size_t i = 0; i < n; ++i)
    if (ptr[i] && (!base || ptr[i] < base)) base = ptr[i];
  std::vector<GatherSeg> segs(n);
  for (size_t i = 0; i < n; ++i) segs[i] = GatherSeg{ptr[i] ? (uint64_t)(ptr[i] - base) : 0u, lens[i], 0u};

  GatherCursor c;
  gather_begin(c, base, segs.data(), (uint32_t)n);
  Sink sink;
  uint32_t w[16];
  const uint32_t r = gather_walk(c, w, sink);
  bool ok = c.total == want.size() && r == want.size() % 64 && sink.out.size() == want.size() - r &&
            std::equal(sink.out.begin(), sink.out.end(), want.begin());
  for (uint32_t k = 0; ok && k < 64; ++k) {
    const uint8_t got = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
    ok = got == (k < r ? want[want.size() - r + k] : 0);
  }
  if (!ok) {
    ++g_failed;
    printf("FAIL %s: %zu segments, %zu bytes (walk: total %llu, tail %u, %zu block bytes)\n", name, n, want.size(),
           (unsigned long long)c.total, r, sink.out.size());
  }
  for (uint8_t *p : ptr) free(p);
}

std::vector<uint32_t> ones(size_t n) { return std::vector<uint32_t>(n, 1u); }

}  // namespace

int main() {
  // every split position of a block across two segments, between long
  // segments (the regular path) and with nothing around (the byte path)
  for (uint32_t cut = 1; cut <= 63; ++cut) {
    run("split long", {64 + cut, 200 - cut});
    run("split long, descending addresses", {64 + cut, 200 - cut}, true);
    run("split bare", {cut, 64 - cut});
    run("split, short second segment", {128 + cut, 64 - cut});
    run("split, short first segment", {cut, 300});
  }
  run("three segments in one block", {20, 20, 24});
  run("three segments in one block, long ends", {100, 7, 100});
  run("64 segments in one block", ones(64));
  {
    std::vector<uint32_t> v = ones(64);
    v.push_back(200);
    v.insert(v.begin(), 200);
    run("64 one-byte segments between long ones", v);
  }
  run("empty segment first", {0, 130});
  run("empty segment in the middle", {70, 0, 70});
  run("empty segments in the middle of a cut", {100, 0, 0, 100});
  run("empty segment last", {130, 0});
  run("only empty segments", {0, 0, 0});
  run("empty segments everywhere", {0, 33, 0, 0, 31, 0, 64, 0, 5, 0});
  run("segment ends on a block boundary", {128, 100});
  run("segment ends on a block boundary, then a short one", {64, 10});
  run("segments of exactly one block", {64, 64, 64});
  run("16-byte segments", std::vector<uint32_t>(12, 16u));
  run("15-byte segments", std::vector<uint32_t>(13, 15u));
  run("17-byte segments", std::vector<uint32_t>(13, 17u));
  for (uint32_t tail : {0u, 1u, 55u, 56u, 63u}) {
    run("tail in one segment", {128 + tail});
    if (tail) run("tail alone", {tail});
    if (tail > 1) run("tail over three segments", {130, tail / 2, 62 + tail - tail / 2});
    run("tail after a cut", {100, 28 + tail});
    if (tail) run("tail of one-byte segments", ones(64 + tail));
  }
  run("empty message", {});
  {  // one whole 512 KiB chunk as datagram payloads: 353 x 1484 + 436
    std::vector<uint32_t> v(353, 1484u);
    v.push_back(436u);
    run("datagram pattern", v);
    run("datagram pattern, descending addresses", v, true);
  }
  printf("%d cases, %d failed\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
