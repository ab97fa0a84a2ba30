// gather_step_check.cpp -- the stepper of k_sha1_gather_lat's loader wave
// (gather_step, csrc/sha1_gather_walk.h) run on the CPU, built with
// -fsanitize=address,undefined (make gather_step_check;
// tests/test_gather_step_host.py runs it as a child process).
//
// Every segment is a heap allocation of exactly its own size, the descriptor
// table one of exactly nseg entries and the idle block one of 16 bytes, so a
// read outside them is an AddressSanitizer report.  The stepper must yield,
// one block per call: gather_walk's whole blocks, then the padding block(s)
// as the oracle lays them out (sha.c:529-543: the r tail bytes, 0x80, zeros,
// the 64-bit bit count; two blocks when r >= 56), then zeros -- and those
// calls past the end are made AFTER the segments and the table were freed.
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

// The oracle's layout of a whole padded message.
std::vector<uint8_t> padded(const std::vector<uint8_t> &msg) {
  std::vector<uint8_t> p = msg;
  p.push_back(0x80);
  while (p.size() % 64 != 56) p.push_back(0);
  const uint64_t bits = (uint64_t)msg.size() * 8u;
  for (int k = 7; k >= 0; --k) p.push_back((uint8_t)(bits >> (8 * k)));
  return p;
}

// One message whose segments have these lengths (a 16-byte header allocated in
// front of each payload when `headers`: the segment starts 16 bytes into its
// allocation, as a datagram's payload does).
void run(const char *name, const std::vector<uint32_t> &lens, bool reverse_alloc = false, bool headers = false) {
  ++g_cases;
  const size_t n = lens.size();
  const uint32_t hdr = headers ? 16u : 0u;
  std::vector<uint8_t *> ptr(n, nullptr);
  std::vector<uint8_t> msg;
  std::vector<std::vector<uint8_t>> bytes(n);
  for (size_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < lens[i]; ++k) {
      bytes[i].push_back(next_byte());
      msg.push_back(bytes[i].back());
    }
  for (size_t t = 0; t < n; ++t) {
    const size_t i = reverse_alloc ? n - 1 - t : t;
    if (!lens[i]) continue;
    ptr[i] = (uint8_t *)malloc(hdr + lens[i]);
    memset(ptr[i], 0xEE, hdr);
    memcpy(ptr[i] + hdr, bytes[i].data(), lens[i]);
  }
  uint8_t *base = nullptr;
  for (size_t i = 0; i < n; ++i)
    if (ptr[i] && (!base || ptr[i] < base)) base = ptr[i];
  uint8_t *idle = (uint8_t *)malloc(16);
  memset(idle, 0xA5, 16);
  if (!base) base = idle;  // no bytes listed: any pointer, never dereferenced
  // the table: exactly n descriptors (n == 0: a zero-length allocation)
  GatherSeg *segs = (GatherSeg *)malloc(n * sizeof(GatherSeg));
  for (size_t i = 0; i < n; ++i) segs[i] = GatherSeg{ptr[i] ? (uint64_t)(ptr[i] + hdr - base) : 0u, lens[i], 0u};

  // gather_walk's blocks of the same list
  Sink walk;
  {
    GatherCursor c;
    gather_begin(c, base, segs, (uint32_t)n);
    uint32_t w[16];
    gather_walk(c, w, walk);
  }
  const std::vector<uint8_t> want = padded(msg);
  const uint64_t total = gather_total(segs, (uint32_t)n);
  GatherStepper st;
  gather_step_begin(st, base, segs, (uint32_t)n, total, idle);
  bool ok = total == msg.size() && st.nb == want.size() / 64 && st.nfull == msg.size() / 64;
  Sink got;
  for (uint64_t b = 0; ok && b < st.nb; ++b) {
    uint32_t w[16];
    gather_step(st, w, idle);
    got.block(w);
  }
  ok = ok && got.out == want && walk.out.size() == (msg.size() & ~(size_t)63) &&
       std::equal(walk.out.begin(), walk.out.end(), got.out.begin());
  // past the end: nothing of the message may be read -- it is gone
  for (uint8_t *p : ptr) free(p);
  free(segs);
  for (int k = 0; ok && k < 3; ++k) {
    uint32_t w[16];
    gather_step(st, w, idle);
    for (int j = 0; j < 16; ++j) ok = ok && w[j] == 0u;
  }
  free(idle);
  if (!ok) {
    ++g_failed;
    printf("FAIL %s: %zu segments, %zu bytes (total %llu, nb %llu, %zu of %zu padded bytes)\n", name, n, msg.size(),
           (unsigned long long)total, (unsigned long long)st.nb, got.out.size(), want.size());
  }
}

std::vector<uint32_t> ones(size_t n) { return std::vector<uint32_t>(n, 1u); }

}  // namespace

int main() {
  run("empty message", {});
  run("only empty segments", {0, 0, 0});
  for (uint32_t len : {1u, 55u, 56u, 63u, 64u, 119u, 120u, 127u, 128u}) {
    run("one segment", {len});
    run("one segment behind a header", {len}, false, true);
    run("one-byte segments", ones(len));
    if (len > 2) run("three segments", {len / 3, len / 3, len - 2 * (len / 3)});
  }
  // a cut at every byte of a block (each of its four quads), between long
  // segments (the regular path), bare and with short neighbours (the byte path)
  for (uint32_t cut = 1; cut <= 63; ++cut) {
    run("split long", {64 + cut, 200 - cut});
    run("split long, descending addresses", {64 + cut, 200 - cut}, true);
    run("split long, tail past 56", {64 + cut, 188 - cut});
    run("split bare", {cut, 64 - cut});
    run("split, short second segment", {128 + cut, 64 - cut});
    run("split, short first segment", {cut, 300});
  }
  run("three segments in one block", {20, 20, 24});
  run("three segments in one block, long ends", {100, 7, 100});
  run("five segments in one block, long ends", {100, 3, 4, 5, 100});
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
  run("empty segments last, whole blocks", {128, 0, 0});
  run("empty segments everywhere", {0, 33, 0, 0, 31, 0, 64, 0, 5, 0});
  run("segment ends on a block boundary", {128, 100});
  run("segment ends on a block boundary, then a short one", {64, 10});
  run("segments of exactly one block", {64, 64, 64});
  run("16-byte segments", std::vector<uint32_t>(12, 16u));
  run("15-byte segments", std::vector<uint32_t>(13, 15u));
  run("17-byte segments", std::vector<uint32_t>(13, 17u));
  run("nine descriptors (two trips of the sum)", std::vector<uint32_t>(9, 70u));
  for (uint32_t tail : {0u, 1u, 55u, 56u, 63u}) {
    run("tail in one segment", {128 + tail});
    if (tail > 1) run("tail over three segments", {130, tail / 2, 62 + tail - tail / 2});
    run("tail after a cut", {100, 28 + tail});
    if (tail) run("tail of one-byte segments", ones(64 + tail));
  }
  {  // 1484-byte payloads behind 16-byte headers: 8 datagrams, and a whole 512 KiB chunk (353 x 1484 + 436)
    run("datagrams", std::vector<uint32_t>(8, 1484u), false, true);
    run("datagrams, descending addresses", std::vector<uint32_t>(8, 1484u), true, true);
    std::vector<uint32_t> v(353, 1484u);
    v.push_back(436u);
    run("datagram pattern", v, false, true);
    run("datagram pattern, descending addresses", v, true, true);
  }
  printf("%d cases, %d failed\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
