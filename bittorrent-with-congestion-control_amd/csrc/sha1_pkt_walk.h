// sha1_pkt_walk.h -- the block walk of k_sha1_pkts (sha1_kernels.hip): a
// message held as the payloads of equal-sized packet buffers -> 64-byte blocks
// as 16 big-endian words (sha.c:186-189), padding included.
//
// Plain C++ that compiles for the device and for the host, like
// sha1_gather_walk.h: the kernel supplies the loads, the CPU check
// (tests/native/pkt_walk_check.cpp) a fetch that records every address, and
// runs this very text under AddressSanitizer.
//
// The layout (bt_sha1_pkt_geom, include/bt_sha1.h): a slot is slot_pkts packet
// buffers `stride` bytes apart, each `header` bytes followed by up to
// `payload` bytes of message.  Byte m of a message is at sequence position
// k = m / payload, in buffer j = order[k], at slot + j*stride + header +
// m % payload.  stride, header and payload are multiples of 4, payload >= 64.
//
// READ CONTRACT, for a message of len bytes, npkt = ceil(len / payload):
//   * data is read only inside [header, header + payload) of a buffer
//     j <= slot_pkts - 1 of the message's own slot: every order entry is
//     clamped to slot_pkts - 1 before it is used, so no byte outside
//     [slot, slot + slot_pkts*stride) is read whatever `order` holds.  Every
//     load is 16 bytes at or after a buffer's payload start and ends at or
//     before that buffer's payload end, so nothing needs a clamp at the end of
//     the slot, header + payload == stride included;
//   * no order entry at or past npkt is read: an index read ahead is replaced
//     by the cursor's own position k when it lies past the message's end, and
//     a message of no bytes reads the word `idle` instead (any readable u32;
//     the kernel passes the message's own length).  The cursor never moves to
//     a position that holds no byte of the message, and "past the end" is a
//     compare of byte counts (`left`), so a message costs no division;
//   * bytes read and not listed (a short last datagram's slack, the far side
//     of a cut that a clamped fetch re-reads, buffer `idle` of an empty
//     message) are discarded by position: none reaches a block.
//
// The walk.  The cursor is (k, a): sequence position k with a of its bytes
// consumed; it moves by 64 per block with one compare-and-wrap.  A block lies
// in datagram A = position k, or in A's last rem = payload - a bytes (4..60, a
// multiple of 4) plus the head of B = position k + 1.  Four 16-byte loads at
// A + 16*i or B + 16*i - rem; the one quad that straddles the cut is put
// together from A's last 16 bytes (loaded in that quad's place) and B's first
// 16 (a fifth load) by a shift of whole words -- every cut is on a word
// boundary, so there is no funnel shift and no byte path.  No branch: cursor
// step, addresses and merge are selects.  Order entries are read two wraps
// ahead (positions k + 2 and k + 3 are in registers or in flight).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BT_PKT_HD __host__ __device__ __forceinline__
#else
#define BT_PKT_HD inline
#endif

namespace btsha1 {

struct PktGeom {  // bt_sha1_pkt_geom (include/bt_sha1.h)
  uint32_t stride, header, payload, slot_pkts;
};
static_assert(sizeof(PktGeom) == 16, "packet geometry layout");

struct PktQuad {
  uint32_t v[4];
};

// What the 64 + 16 bytes of one block are: five loads and how to merge them.
struct PktSlot {
  PktQuad q[4], xb;
  uint32_t sq, cc;  // quad sq (4: none) = A's last cc bytes (4, 8 or 12), then B's first 16 - cc
};

struct PktCursor {
  const uint8_t *slot;
  const uint32_t *ord;  // the message's order entries; `idle` when it has none
  uint32_t k, a;
  uint32_t left;        // len - k * payload: position k + j holds message bytes iff left > j * payload
  uint32_t oa, ob;      // payload offsets in the slot of positions k and k + 1
  uint32_t x, y;        // order entries of positions k + 2 and k + 3; y may be in flight
                        // (a position past the message's end stands for position k: never used for data)
};

// c ? a : b with both sides evaluated first (sha1_gather_walk.h, gather_sel).
BT_PKT_HD uint32_t pkt_sel(bool c, uint32_t a, uint32_t b) { return c ? a : b; }

BT_PKT_HD uint32_t pkt_npkt(uint32_t len, uint32_t payload) { return len / payload + (len % payload ? 1u : 0u); }

// Offset in the slot of the payload of the buffer an order entry names.
BT_PKT_HD uint32_t pkt_off(const PktGeom &g, uint32_t entry) {
  const uint32_t j = entry < g.slot_pkts - 1u ? entry : g.slot_pkts - 1u;
  return j * g.stride + g.header;
}

// Where the order entry of position k + j (j = 1..3) is read: position k's
// when k + j holds no byte of the message.  j * payload saturates, uniformly.
BT_PKT_HD const uint32_t *pkt_ord_at(const PktCursor &c, const PktGeom &g, uint32_t j) {
  const uint64_t jp = (uint64_t)j * g.payload;
  return c.ord + c.k + (c.left > (jp > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)jp) ? j : 0u);
}

// F: uint32_t order(const uint32_t *) and void quad(PktQuad &, const uint8_t *).
template <class F>
BT_PKT_HD void pkt_begin(PktCursor &c, const PktGeom &g, const uint8_t *slot, const uint32_t *ord, uint32_t len,
                         const uint32_t *idle, F &f) {
  c.slot = slot;
  c.ord = len ? ord : idle;
  c.k = c.a = 0;
  c.left = len;
  c.oa = pkt_off(g, f.order(c.ord));
  c.ob = pkt_off(g, f.order(pkt_ord_at(c, g, 1)));
  c.x = f.order(pkt_ord_at(c, g, 2));
  c.y = 0;  // pkt_ahead's first call reads it, after the first block's loads
}

// Past one block when `adv`, which the caller gives only while the next block
// holds a byte of the message (so position k stays inside it); else the cursor
// stays and a fetch re-reads the block.  Uses x, never y: see pkt_ahead.
BT_PKT_HD bool pkt_step(PktCursor &c, const PktGeom &g, bool adv) {
  const uint32_t a1 = c.a + 64u;
  const bool wrap = adv && a1 >= g.payload;
  c.a = adv ? (wrap ? a1 - g.payload : a1) : c.a;
  c.k += wrap ? 1u : 0u;
  c.left -= wrap ? g.payload : 0u;
  c.oa = pkt_sel(wrap, c.ob, c.oa);
  c.ob = pkt_sel(wrap, pkt_off(g, c.x), c.ob);
  return wrap;
}

// After the block's own loads were issued: y (read one block ago) becomes x
// when the step wrapped, and position k + 3 is read again -- one
// unconditional load per block, as gather_plan's, issued last so that the
// loads a block waits for always have one behind them.
template <class F>
BT_PKT_HD void pkt_ahead(PktCursor &c, const PktGeom &g, bool wrapped, F &f) {
  c.x = pkt_sel(wrapped, c.y, c.x);
  c.y = f.order(pkt_ord_at(c, g, 3));
}

// The loads of the block at the cursor.
template <class F>
BT_PKT_HD void pkt_fetch(PktSlot &s, const PktCursor &c, const PktGeom &g, F &f) {
  const uint32_t rem = g.payload - c.a;  // >= 4
  const bool cut = rem < 64u;
  const uint32_t a0 = c.oa + c.a, b0 = c.ob - rem, win = c.oa + g.payload - 16u;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t lo = 16u * i;
    f.quad(s.q[i], c.slot + (lo + 16u <= rem ? a0 + lo : (lo >= rem ? b0 + lo : win)));
  }
  f.quad(s.xb, c.slot + (cut ? c.ob : a0));
  const uint32_t cc = rem & 15u;
  s.sq = cut && cc ? rem >> 4 : 4u;
  s.cc = cc;
}

// The fetched block as 16 big-endian words: quad sq is words sh .. sh + 3 of
// (A's last 16 bytes : B's first 16), sh = (16 - cc) / 4 = 3, 2 or 1, in two
// select stages: by 2 when cc < 12, by 1 when cc is 4 or 12.
BT_PKT_HD void pkt_words(uint32_t (&w)[16], const PktSlot &s) {
  uint32_t x[8], y[5], m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t v = s.q[0].v[k];
    v = pkt_sel(s.sq == 1u, s.q[1].v[k], v);
    v = pkt_sel(s.sq == 2u, s.q[2].v[k], v);
    v = pkt_sel(s.sq == 3u, s.q[3].v[k], v);
    x[k] = v;
    x[4 + k] = s.xb.v[k];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) y[k] = pkt_sel(s.cc < 12u, x[k + 2], x[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = pkt_sel(s.cc & 4u, y[k + 1], y[k]);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) w[4 * i + k] = __builtin_bswap32(pkt_sel(s.sq == (uint32_t)i, m[k], s.q[i].v[k]));
}

// Block b >= nfull of a message of nfull whole blocks and r more bytes
// (sha.c:529-543, laid out as k_sha1_ragged's tail): block nfull keeps its r
// bytes and takes the 0x80 mark; the last block, which is nfull + 1 when
// r >= 56, takes the bit count.  Whole blocks pass unchanged.  A message has
// at most two such blocks, so this is written for size, not speed: one word
// per trip of a loop that is kept rolled, the block rotating through w[0]
// (sixteen unrolled copies of the body are 0.6 KB of a library whose size is
// bounded, tests/test_abi.py).
BT_PKT_HD void pkt_pad(uint32_t (&w)[16], uint32_t b, uint32_t nfull, uint32_t r, uint32_t len) {
  if (b < nfull) return;
  const bool tail = b == nfull;
  const uint32_t wi = tail ? r >> 2 : 0u, sh = (r & 3u) * 8u;
  const uint32_t keep = tail ? ~(0xFFFFFFFFu >> sh) : 0u, mark = tail ? 0x80000000u >> sh : 0u;
#pragma nounroll
  for (uint32_t j = 0; j < 16; ++j) {
    const uint32_t v = j < wi ? w[0] : (j == wi ? (w[0] & keep) | mark : 0u);
#pragma unroll
    for (int k = 0; k < 15; ++k) w[k] = w[k + 1];
    w[15] = v;
  }
  if (!tail || r < 56u) {
    w[14] = len >> 29;
    w[15] = len << 3;
  }
}

// Blocks a message of len bytes is hashed as.
BT_PKT_HD uint32_t pkt_nblocks(uint32_t len) { return (len >> 6) + ((len & 63u) >= 56u ? 2u : 1u); }

// The loads of a message's first block, position 0 with nothing consumed: no
// cut (payload >= 64), so no selects -- pkt_fetch(s, c, g, f) would fetch the
// same, in ten times the code of a library whose size is bounded.  B's window
// is loaded all the same (A's head again), so that the loop meets the same
// loads in flight on its first trip as on every other.
template <class F>
BT_PKT_HD void pkt_fetch_first(PktSlot &s, const PktCursor &c, F &f) {
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) f.quad(s.q[i], c.slot + c.oa + 16u * i);
  f.quad(s.xb, c.slot + c.oa);
  s.sq = 4u;
  s.cc = 0u;
}

// The whole message: sink.block(w) for each of its pkt_nblocks(len) blocks, in
// order.  One block's loads are in flight while the one before it is consumed;
// sink.fence() stands between the two (the device pins the order there).  The
// loop holds ONE sink.block: the slot is turned into words before its
// registers take the next block's loads, so the two never need a copy.
template <class F, class Sink>
BT_PKT_HD void pkt_walk(const PktGeom &g, const uint8_t *slot, const uint32_t *ord, uint32_t len, const uint32_t *idle,
                        F &f, Sink &sink) {
  const uint32_t nfull = len >> 6, r = len & 63u, nb = pkt_nblocks(len);
  const uint32_t nheld = nfull + (r ? 1u : 0u);  // blocks that hold a byte of the message
  PktCursor c;
  pkt_begin(c, g, slot, ord, len, idle, f);
  PktSlot s;
  pkt_fetch_first(s, c, f);
  sink.fence();  // as in the loop: the entry read ahead is the last load in flight
  pkt_ahead(c, g, false, f);
  sink.fence();
  for (uint32_t b = 0; b < nb; ++b) {
    uint32_t w[16];
    pkt_words(w, s);
    pkt_pad(w, b, nfull, r, len);
    const bool wrapped = pkt_step(c, g, b + 1u < nheld);  // past the last block held, that one again
    pkt_fetch(s, c, g, f);
    sink.fence();  // y is waited for behind this block's loads, not in front of them
    pkt_ahead(c, g, wrapped, f);
    sink.fence();
    sink.block(w);
  }
}

}  // namespace btsha1
