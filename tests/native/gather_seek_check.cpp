// gather_seek_check.cpp -- the random access of the chain-form gather kernels
// (gather_seek / gather_block_at / gather_tail_at / gather_span_at,
// csrc/sha1_gather_walk.h)
// run on the CPU, built with -fsanitize=address,undefined (make
// gather_seek_check; tests/test_gather_seek_host.py runs it as a child process
// and hands it tests/gather_cases.WALK_CASES in a file, one list per line).
//
// Every segment is a heap allocation of exactly its own size, and for every
// listed prefix the descriptor and pos arrays are allocations of exactly that
// many entries while the message's real list is longer: a read of one byte
// outside a listed segment, or of one table entry at or past nseg, is an
// AddressSanitizer report.  Every whole block inside the prefix, built from
// every hint from 0 to its true segment (and from hints that are wrong), must
// equal the same 64 bytes of the concatenation; so must the tails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sha1_gather_walk.h"

using namespace btsha1;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint8_t)(g_rng >> 56);
}

int g_failed = 0, g_cases = 0;
long long g_blocks = 0, g_tails = 0;
const uint32_t kTails[] = {0u, 1u, 55u, 56u, 63u};

bool same(const uint32_t (&w)[16], const uint8_t *want, uint32_t n) {
  for (uint32_t k = 0; k < 64; ++k) {
    const uint8_t got = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
    if (got != (k < n ? want[k] : 0)) return false;
  }
  return true;
}

// One message whose segments have these lengths.  all_hints: every hint from 0
// to the true segment; otherwise 0, three before the true segment, and it.
void run(const char *name, const std::vector<uint32_t> &lens, const std::vector<size_t> &prefixes, bool all_hints) {
  ++g_cases;
  const size_t n = lens.size();
  std::vector<uint8_t *> ptr(n, nullptr);
  std::vector<uint8_t> want;
  uint8_t *base = nullptr;
  for (size_t t = 0; t < n; ++t) {
    const size_t i = n - 1 - t;  // allocated against the list order
    if (!lens[i]) continue;
    ptr[i] = (uint8_t *)malloc(lens[i]);
    if (!base || ptr[i] < base) base = ptr[i];
  }
  for (size_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < lens[i]; ++k) {
      ptr[i][k] = next_byte();
      want.push_back(ptr[i][k]);
    }
  bool ok = true;
  for (size_t p : prefixes) {
    if (p == 0 || p > n) continue;
    GatherSeg *segs = (GatherSeg *)malloc(p * sizeof(GatherSeg));
    uint64_t *pos = (uint64_t *)malloc(p * sizeof(uint64_t));
    uint64_t total = 0;
    for (size_t i = 0; i < p; ++i) {
      segs[i] = GatherSeg{ptr[i] ? (uint64_t)(ptr[i] - base) : 0u, lens[i], 0xABCDu};
      pos[i] = total;
      total += lens[i];
    }
    for (uint64_t g = 0; 64 * g < total; ++g) {
      const uint64_t m = 64 * g;
      uint32_t truth = 0;  // largest k with pos[k] <= m
      for (size_t i = 0; i < p; ++i)
        if (pos[i] <= m) truth = (uint32_t)i;
      std::vector<uint32_t> hints;
      if (all_hints)
        for (uint32_t h = 0; h <= truth; ++h) hints.push_back(h);
      else
        hints = {0u, truth > 3u ? truth - 3u : 0u, truth};
      hints.push_back(truth + 1u);  // wrong ones: past the segment, at and past nseg
      hints.push_back((uint32_t)p);
      hints.push_back(0xFFFFFFFFu);
      for (uint32_t h : hints) {
        if (m + 64 <= total) {
          uint32_t w[16], seg = 0xFFFFFFFFu;
          gather_block_at(w, base, segs, pos, (uint32_t)p, m, h, &seg);
          ++g_blocks;
          uint32_t w2[16] = {0}, seg2 = 0xFFFFFFFFu;  // the kernels' form: block and tail behind one seek
          gather_span_at(w2, base, segs, pos, (uint32_t)p, m, 64u, h, &seg2);
          if (seg != truth || !same(w, want.data() + m, 64) || seg2 != truth || !same(w2, want.data() + m, 64)) {
            ok = false;
            printf("FAIL %s: prefix %zu, block %llu, hint %u: segment %u (want %u)\n", name, p, (unsigned long long)g,
                   h, seg, truth);
          }
        }
        for (uint32_t r : kTails) {
          if (m + r > total || (r == 0 && h != 0)) continue;
          uint32_t w[16];
          gather_tail_at(w, base, segs, pos, (uint32_t)p, m, r, h);
          ++g_tails;
          bool span_ok = true;
          if (r) {
            uint32_t w2[16] = {0}, seg2 = 0;
            gather_span_at(w2, base, segs, pos, (uint32_t)p, m, r, h, &seg2);
            span_ok = same(w2, want.data() + m, r);
          }
          if (!span_ok || !same(w, want.data() + m, r)) {
            ok = false;
            printf("FAIL %s: prefix %zu, tail of %u bytes at %llu, hint %u\n", name, p, r, (unsigned long long)m, h);
          }
        }
      }
    }
    {  // r == 0 where the message ends: nothing is read, not even a table entry
      uint32_t w[16];
      gather_tail_at(w, base, nullptr, nullptr, 0u, total, 0u, 0u);
      if (!same(w, nullptr, 0)) ok = false;
    }
    free(segs);
    free(pos);
  }
  if (!ok) ++g_failed;
  for (uint8_t *q : ptr) free(q);
}

std::vector<size_t> every_prefix(size_t n) {
  std::vector<size_t> v;
  for (size_t p = 1; p <= n; ++p) v.push_back(p);
  return v;
}

}  // namespace

int main(int argc, char **argv) {
  std::vector<std::vector<uint32_t>> cases;
  if (argc > 1) {  // one list of segment lengths per line (an empty line: the empty list)
    std::ifstream in(argv[1]);
    if (!in) {
      printf("cannot read %s\n", argv[1]);
      return 2;
    }
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      std::vector<uint32_t> v;
      uint32_t x;
      while (ss >> x) v.push_back(x);
      cases.push_back(v);
    }
  } else {
    for (uint32_t cut = 1; cut < 64; ++cut) cases.push_back({cut, 64 - cut});
    cases.push_back({20, 20, 24});
    cases.push_back({90, 7, 90});
    cases.push_back(std::vector<uint32_t>(64, 1u));
    cases.push_back({70, 0, 70});
    cases.push_back({100, 0, 0, 100});
    cases.push_back({0, 33, 0, 0, 31, 0, 64, 0, 5, 0});
    cases.push_back({0, 0, 0});
    cases.push_back({});
  }
  for (const auto &lens : cases) run("case", lens, every_prefix(lens.size()), true);
  {  // resume across loader batches: 64 x 130 + 63 bytes in the tests' cycle of lengths
    const uint32_t cyc[] = {1484u, 15u, 0u, 17u, 1u, 436u};
    std::vector<uint32_t> v;
    uint32_t left = 64u * 130u + 63u;
    for (size_t k = 0; left; ++k) {
      const uint32_t l = cyc[k % 6] < left ? cyc[k % 6] : left;
      v.push_back(l);
      left -= l;
    }
    run("seam cycle", v, every_prefix(v.size()), true);
  }
  {  // one whole 512 KiB chunk as datagram payloads: 353 x 1484 + 436
    std::vector<uint32_t> v(353, 1484u);
    v.push_back(436u);
    run("datagram pattern", v, {1, 2, 177, 354}, false);
  }
  {  // thousands of one-byte and empty segments
    std::vector<uint32_t> v;
    for (uint32_t k = 0; k < 3000; ++k) v.push_back(k % 3 == 2 ? 0u : 1u);
    run("thousands of tiny segments", v, {1, 1500, 3000}, false);
  }
  printf("%lld blocks, %lld tails\n", g_blocks, g_tails);
  printf("%d cases, %d failed\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
