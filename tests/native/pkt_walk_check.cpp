// pkt_walk_check.cpp -- the block walk of k_sha1_pkts (csrc/sha1_pkt_walk.h)
// on the CPU, under AddressSanitizer / UBSan (Makefile: pkt_walk_check;
// tests/test_pkt_walk_host.py builds and runs it).
//
// The walk's contract is about addresses, so the fetch handed to it records
// every one.  For every geometry, length and order of tests/pkts_cases.py, for
// order arrays full of out-of-range entries and for a byte-misaligned slot:
//   * the slot is an allocation of exactly slot_pkts * stride bytes and the
//     order array one of exactly npkt entries, so an over-read of either is an
//     ASan error;
//   * every 16-byte load must lie in the payload area of one packet buffer of
//     the slot; every order read inside the npkt entries (or be the idle word
//     of an empty message);
//   * the blocks handed to the sink must be those of the assembled message,
//     padding included, with every byte outside the listed payloads poison --
//     and again with different poison.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sha1_pkt_walk.h"

using namespace btsha1;

static int g_fail = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      if (g_fail++ < 20) {            \
        fprintf(stderr, "FAIL: ");    \
        fprintf(stderr, __VA_ARGS__); \
        fprintf(stderr, "\n");        \
      }                               \
    }                                 \
  } while (0)

static uint32_t rng(uint64_t &s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(s >> 33);
}

struct Fetch {
  const uint8_t *slot;
  PktGeom g;
  const uint32_t *ord;
  uint32_t npkt;
  const uint32_t *idle;
  uint64_t nquad = 0, nord = 0;
  uint32_t order(const uint32_t *p) {
    ++nord;
    if (npkt == 0)
      CHECK(p == idle, "empty message read an order entry");
    else
      CHECK(p >= ord && p < ord + npkt, "order read at index %td of %u", p - ord, npkt);
    return *p;
  }
  void quad(PktQuad &q, const uint8_t *p) {
    ++nquad;
    const int64_t off = p - slot;
    const int64_t slot_len = (int64_t)g.slot_pkts * g.stride;
    CHECK(off >= 0 && off + 16 <= slot_len, "load at slot offset %lld of %lld", (long long)off, (long long)slot_len);
    if (off >= 0 && off + 16 <= slot_len) {
      const int64_t in = off % g.stride;
      CHECK(in >= g.header && in + 16 <= (int64_t)g.header + g.payload, "load at %lld outside a payload area",
            (long long)off);
      memcpy(&q, p, 16);
    } else {
      memset(&q, 0, 16);
    }
  }
};

struct Sink {
  std::vector<uint32_t> words;
  void fence() {}
  void block(uint32_t (&w)[16]) { words.insert(words.end(), w, w + 16); }
};

// The padded blocks of a message (sha.c:529-543) as big-endian words.
static std::vector<uint32_t> padded(const std::vector<uint8_t> &msg) {
  std::vector<uint8_t> b(msg);
  b.push_back(0x80);
  while (b.size() % 64 != 56) b.push_back(0);
  const uint64_t bits = (uint64_t)msg.size() * 8;
  for (int k = 7; k >= 0; --k) b.push_back((uint8_t)(bits >> (8 * k)));
  std::vector<uint32_t> w(b.size() / 4);
  for (size_t i = 0; i < w.size(); ++i)
    w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
  return w;
}

enum Order { IDENT, REVERSED, PERMUTED, ONE_BUFFER, OUT_OF_RANGE };

static void run_case(const PktGeom &g, uint32_t len, Order kind, uint32_t misalign, uint64_t seed) {
  const uint32_t npkt = pkt_npkt(len, g.payload);
  const uint64_t slot_len = (uint64_t)g.slot_pkts * g.stride;
  // The order array: exactly npkt entries, an allocation of its own.
  uint32_t *ord = (uint32_t *)malloc(npkt ? npkt * sizeof(uint32_t) : 1);
  std::vector<uint32_t> pool(g.slot_pkts);
  for (uint32_t j = 0; j < g.slot_pkts; ++j) pool[j] = j;
  uint64_t s = seed;
  for (uint32_t j = g.slot_pkts; j > 1; --j) std::swap(pool[j - 1], pool[rng(s) % j]);
  for (uint32_t k = 0; k < npkt; ++k) {
    switch (kind) {
      case IDENT: ord[k] = k; break;
      case REVERSED: ord[k] = npkt - 1 - k; break;
      case PERMUTED: ord[k] = pool[k]; break;
      case ONE_BUFFER: ord[k] = g.slot_pkts / 2; break;
      case OUT_OF_RANGE: ord[k] = k % 3 == 0 ? 0xFFFFFFFFu : g.slot_pkts + k; break;
    }
  }
  std::vector<uint32_t> first;
  for (int pass = 0; pass < 2; ++pass) {
    // The slot: exactly slot_len bytes (plus the misalignment in front).
    uint8_t *alloc = (uint8_t *)malloc(slot_len + misalign);
    uint8_t *slot = alloc + misalign;
    for (uint64_t b = 0; b < slot_len; ++b) alloc[misalign + b] = (uint8_t)(pass ? 0x5A ^ b : 0xEE);  // poison
    // Payloads in sequence order; a buffer named twice holds what the LAST
    // position wrote, so the message is read back from the slot afterwards.
    uint64_t ms = seed ^ 0x1234;
    for (uint32_t k = 0; k < npkt; ++k) {
      const uint32_t j = ord[k] < g.slot_pkts - 1 ? ord[k] : g.slot_pkts - 1;
      const uint32_t nbytes = k + 1 < npkt ? g.payload : len - k * g.payload;
      for (uint32_t b = 0; b < nbytes; ++b) slot[(uint64_t)j * g.stride + g.header + b] = (uint8_t)rng(ms);
    }
    std::vector<uint8_t> msg(len);
    for (uint32_t m = 0; m < len; ++m) {
      const uint32_t k = m / g.payload;
      const uint32_t j = ord[k] < g.slot_pkts - 1 ? ord[k] : g.slot_pkts - 1;
      msg[m] = slot[(uint64_t)j * g.stride + g.header + m % g.payload];
    }
    if (kind != ONE_BUFFER && kind != OUT_OF_RANGE) {
      // Distinct buffers: the message is exactly what was written, and a
      // duplicate datagram (an unused buffer) holds other bytes.
      uint64_t chk = seed ^ 0x1234;
      for (uint32_t m = 0; m < len; ++m) CHECK(msg[m] == (uint8_t)rng(chk), "case construction");
    }
    const uint32_t idle = len;
    Fetch f{slot, g, ord, npkt, &idle};
    Sink sink;
    pkt_walk(g, slot, ord, len, &idle, f, sink);
    const std::vector<uint32_t> want = padded(msg);
    CHECK(sink.words.size() == want.size() && pkt_nblocks(len) * 16u == want.size(),
          "geometry %u/%u/%u len %u order %d: %zu words, want %zu", g.stride, g.header, g.payload, len, (int)kind,
          sink.words.size(), want.size());
    if (sink.words.size() == want.size())
      for (size_t i = 0; i < want.size(); ++i)
        if (sink.words[i] != want[i]) {
          CHECK(false, "geometry %u/%u/%u len %u order %d misalign %u: block %zu word %zu is %08x, want %08x",
                g.stride, g.header, g.payload, len, (int)kind, misalign, i / 16, i % 16, sink.words[i], want[i]);
          break;
        }
    if (pass == 0) first = sink.words;
    else CHECK(first == sink.words, "len %u order %d: the blocks depend on bytes outside the listed payloads", len, (int)kind);
    free(alloc);
  }
  free(ord);
}

int main() {
  const PktGeom geoms[] = {{1500, 16, 1484, 24}, {76, 4, 68, 24}, {64, 0, 64, 24}, {144, 16, 128, 24}};
  uint64_t cases = 0;
  for (const PktGeom &g : geoms) {
    const uint32_t p = g.payload;
    const uint32_t lens[] = {0,      1,      55,         56,         63,          64,          65,          p - 1,
                             p,      p + 1,  p + 55,     p + 56,     17 * p,      17 * p + 4,  17 * p + 55, 17 * p + 56,
                             17 * p + 63, 3 * p - 1, 24 * p, 24 * p - 64};
    for (uint32_t len : lens)
      for (int kind = IDENT; kind <= OUT_OF_RANGE; ++kind) {
        run_case(g, len, (Order)kind, 0, 0x9E3779B97F4A7C15ull * (len + 1) + kind);
        ++cases;
      }
    for (uint32_t mis = 1; mis < 4; ++mis) {
      run_case(g, 17 * p + 55, PERMUTED, mis, mis);
      ++cases;
    }
  }
  // A slot of one buffer: every position clamps to it.
  run_case(PktGeom{64, 0, 64, 1}, 64, OUT_OF_RANGE, 0, 7);
  run_case(PktGeom{64, 0, 64, 1}, 63, IDENT, 0, 8);
  cases += 2;
  if (g_fail) {
    fprintf(stderr, "pkt_walk_check: %d failures in %llu cases\n", g_fail, (unsigned long long)cases);
    return 1;
  }
  printf("pkt_walk_check: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
