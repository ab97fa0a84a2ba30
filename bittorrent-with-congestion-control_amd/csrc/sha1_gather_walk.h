// sha1_gather_walk.h -- the block walk of the scatter-gather SHA-1 kernels
// (k_sha1_gather, sha1_kernels.hip): a cursor over a message's segment list
// -> one 64-byte block as 16 big-endian words (sha.c:186-189).
//
// Plain C++ that compiles for the device and for the host: the CPU check
// (tests/native/gather_walk_check.cpp) runs this very text under
// AddressSanitizer with every segment in an allocation of its own, because the
// walk's contract is about addresses: NO BYTE OUTSIDE THE LISTED SEGMENTS IS
// READ (the caller may be writing elsewhere in the slot; a segment may end an
// allocation).  Every load below lies inside one segment of the message; where
// a load has nothing to fetch its address is clamped to bytes of a segment
// that the block reads anyway, never branched around (absorb_ring's reason:
// a load inside a branch costs the prefetch its overlap).
//
// Two ways to a block:
//   regular  the block lies in the current segment A, or in A's last a bytes
//            (1 <= a < 64) and the head of the next segment B, both at least 16
//            bytes long.  Four unaligned 16-byte loads at A + 16*i or
//            B + 16*i - a; the one quad that straddles the cut is merged from
//            two 16-byte windows, A's last 16 bytes (loaded in that quad's
//            place) and B's first 16 (a fifth load), with a funnel shift.  No
//            branch: the cursor step, the five addresses and the merge are
//            selects.  This is every block
//            of a chunk received as datagrams but its last.
//   bytes    anything else (segments shorter than 16 bytes, three or more
//            segments in a block, empty segments, the message's tail): one
//            byte load per byte, stepping over segments as they run out.
// gather_walk() runs a message through both, keeping one regular block in
// flight ahead of the block being consumed; gather_step() (below) does the
// same one block per call, padding included, for k_sha1_gather_lat.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BT_GATHER_HD __host__ __device__ __forceinline__
#else
#define BT_GATHER_HD inline
#endif

namespace btsha1 {

struct GatherSeg {  // bt_sha1_seg (include/bt_sha1.h)
  uint64_t off;
  uint32_t len;
  uint32_t reserved;
};
static_assert(sizeof(GatherSeg) == 16, "segment layout");

struct GatherQuad {
  uint32_t v[4];
};

// Where the message stands: segment ja ("A") with ra of its la bytes unread
// at pa, and a copy of segment ja + 1 ("B"; lb == 0 when there is none), read
// one segment ahead so that stepping into B waits for no table load.
struct GatherCursor {
  const uint8_t *base;
  const GatherSeg *segs;  // the message's first segment
  uint32_t nseg, ja;
  const uint8_t *pa;
  uint32_t ra, la;
  uint64_t boff;
  uint32_t lb;
  uint64_t total;  // bytes taken so far; the message's length once it is exhausted
};

// The addresses of one regular block (all inside A or B) and how to merge.
struct GatherPlan {
  const uint8_t *q[4];
  const uint8_t *wb;
  uint32_t sq, c;  // quad sq (4: none) = A's last c bytes, then B's first 16 - c
};

struct GatherSlot {
  GatherQuad q[4], wb;
  uint32_t sq, c;
};

BT_GATHER_HD GatherSeg gather_seg(const GatherSeg *p) {
  GatherSeg s;
  __builtin_memcpy(&s, p, sizeof s);
  return s;
}

BT_GATHER_HD void gather_load_b(GatherCursor &c) {
  c.boff = 0;
  c.lb = 0;
  if (c.ja + 1 < c.nseg) {
    const GatherSeg s = gather_seg(c.segs + c.ja + 1);
    c.boff = s.off;
    c.lb = s.len;
  }
}

BT_GATHER_HD void gather_begin(GatherCursor &c, const uint8_t *base, const GatherSeg *segs, uint32_t nseg) {
  c.base = base;
  c.segs = segs;
  c.nseg = nseg;
  c.ja = 0;
  c.pa = base;
  c.ra = c.la = 0;
  c.total = 0;
  if (nseg) {
    const GatherSeg s = gather_seg(segs);
    c.pa = base + s.off;
    c.ra = c.la = s.len;
  }
  gather_load_b(c);
}

BT_GATHER_HD bool gather_regular(const GatherCursor &c) {
  return c.ra >= 64u || (c.ra >= 1u && c.la >= 16u && c.lb >= 16u && c.lb >= 64u - c.ra);
}

// Needs gather_regular(c).  The addresses of the next block, then the cursor
// moves past it; its one table load (the new B, or B again) is issued here,
// before the block's own loads, so that waiting for it never waits for them.
BT_GATHER_HD void gather_plan(GatherCursor &c, GatherPlan &p) {
  const uint32_t a = c.ra < 64u ? c.ra : 64u;
  const bool cut = a < 64u;
  const uint8_t *pb = cut ? c.base + c.boff : c.pa;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t lo = 16u * i;
    const uint8_t *in_a = c.pa + lo, *in_b = pb + lo - a, *win_a = c.pa + a - 16u;
    p.q[i] = lo + 16u <= a ? in_a : (lo >= a ? in_b : win_a);
  }
  p.wb = pb;
  p.c = a & 15u;
  p.sq = cut && p.c ? a >> 4 : 4u;
  // Step: past 64 bytes of A; into B when the block cut into it, or when A is
  // used up exactly.
  const uint32_t into_b = cut ? 64u - a : 0u;
  const bool step = cut || c.ra == 64u;
  c.total += 64u;
  c.pa = step ? c.base + c.boff + into_b : c.pa + 64u;
  c.ra = step ? c.lb - into_b : c.ra - 64u;
  c.la = step ? c.lb : c.la;
  c.ja += step ? 1u : 0u;
  // B again, or the new B after a step: one unconditional descriptor load per
  // block.  Guarding it with `if (step)` was tried: the wave then waits for the
  // descriptor inside the branch (s_waitcnt vmcnt(0) behind it in the listing),
  // one memory round trip per block in which any lane steps -- 94 % of them.
  uint32_t jb = c.ja + 1u;
  const bool has_b = jb < c.nseg;
  jb = has_b ? jb : c.nseg - 1u;
  const GatherSeg s = gather_seg(c.segs + jb);
  c.boff = s.off;
  c.lb = has_b ? s.len : 0u;
}

BT_GATHER_HD void gather_fetch(GatherSlot &s, const GatherPlan &p) {
#pragma unroll
  for (int i = 0; i < 4; ++i) __builtin_memcpy(&s.q[i], p.q[i], 16);
  __builtin_memcpy(&s.wb, p.wb, 16);
  s.sq = p.sq;
  s.c = p.c;
}

// c ? a : b with both sides evaluated first.  A `?:` whose arms read two
// elements of an array is compiled into ONE read at a selected index, which
// puts the array into scratch memory; values passed through here stay in
// registers.
BT_GATHER_HD uint32_t gather_sel(bool c, uint32_t a, uint32_t b) { return c ? a : b; }

// The fetched block as 16 big-endian words.  The straddling quad is bytes
// [16 - c, 32 - c) of (A's last 16 bytes : B's first 16): a word shift of
// (16 - c) / 4 in two select stages, then a funnel shift by the odd bytes.
BT_GATHER_HD void gather_words(uint32_t (&w)[16], const GatherSlot &s) {
  uint32_t x[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t v = s.q[0].v[k];
    v = gather_sel(s.sq == 1u, s.q[1].v[k], v);
    v = gather_sel(s.sq == 2u, s.q[2].v[k], v);
    v = gather_sel(s.sq == 3u, s.q[3].v[k], v);
    x[k] = v;
    x[4 + k] = s.wb.v[k];
  }
  const uint32_t sh = 16u - s.c, bits = (sh & 3u) * 8u;
  uint32_t y[6], z[5], m[4];
#pragma unroll
  for (int k = 0; k < 6; ++k) y[k] = gather_sel(sh & 8u, x[k + 2], x[k]);
#pragma unroll
  for (int k = 0; k < 5; ++k) z[k] = gather_sel(sh & 4u, y[k + 1], y[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = (z[k] >> bits) | ((z[k + 1] << 1) << (31u - bits));
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) w[4 * i + k] = __builtin_bswap32(gather_sel(s.sq == (uint32_t)i, m[k], s.q[i].v[k]));
}

// One block by bytes, from any cursor: w = the next up to 64 bytes as
// big-endian words, zero past them; returns how many there were (fewer than
// 64 only where the message ends).  Leaves the cursor as gather_begin would.
BT_GATHER_HD uint32_t gather_bytes(GatherCursor &c, uint32_t (&w)[16]) {
  uint32_t got = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    uint32_t v = 0;
#pragma nounroll
    for (uint32_t b = 0; b < 4; ++b) {
      while (c.ra == 0 && c.ja + 1 < c.nseg) {
        const GatherSeg s = gather_seg(c.segs + ++c.ja);
        c.pa = c.base + s.off;
        c.ra = c.la = s.len;
      }
      if (c.ra) {
        v |= (uint32_t)*c.pa++ << (24u - 8u * b);
        --c.ra;
        ++got;
      }
    }
    w[k] = v;
  }
  c.total += got;
  gather_load_b(c);
  return got;
}

// The whole message: sink.block(w) for each whole block, in order; then w
// holds the r = length % 64 trailing bytes (zero past them) and r is returned,
// with c.total the message's length.  sink.fence() stands between a block's
// loads being issued and the previous block being consumed (the device pins
// the order there; the host does nothing).
template <class Sink>
BT_GATHER_HD uint32_t gather_walk(GatherCursor &c, uint32_t (&w)[16], Sink &sink) {
  for (;;) {
    if (gather_regular(c)) {
      GatherPlan p;
      // Two slots that swap roles by position in the loop, not by a copy: a
      // copy of the slot just fetched would wait for its loads on the spot.
      GatherSlot s0, s1;
      gather_plan(c, p);
      gather_fetch(s0, p);
      while (gather_regular(c)) {
        gather_plan(c, p);
        gather_fetch(s1, p);
        sink.fence();
        gather_words(w, s0);
        sink.block(w);
        if (!gather_regular(c)) {
          s0 = s1;  // long arrived: a block was consumed since its loads
          break;
        }
        gather_plan(c, p);
        gather_fetch(s0, p);
        sink.fence();
        gather_words(w, s1);
        sink.block(w);
      }
      gather_words(w, s0);
      sink.block(w);
      continue;
    }
    const uint32_t got = gather_bytes(c, w);
    if (got < 64u) return got;
    sink.block(w);
  }
}

// ---------------------------------------------------------------------------
// Random access, for the chain-form gather kernels (k_sha1_gather_resume):
// their S wave has lane j build block b0 + j of ONE message, 64 blocks side by
// side, so every lane has to find the segment that holds its block's first
// byte.  pos[k] is the message position of segment k's first byte (the sum of
// the lengths before it), parallel to segs.  The contract above is kept and
// extended: no byte outside the listed segments is read, and NO DESCRIPTOR OR
// pos ENTRY AT INDEX >= nseg IS READ (the host may be appending there while
// the launch runs).
// ---------------------------------------------------------------------------

// The segment that holds message byte m (m below the listed total): the
// largest k < nseg with pos[k] <= m; among empty segments that share a
// position that is the one with bytes in it.  Gallops forward from `hint`
// (1, 2, 4, ... entries), then bisects the last stride: with 1484-byte
// payloads a block of the batch that `hint` was taken for lies at most three
// segments on, found with three dependent reads, where a bisection of the
// whole list would take nine.  Any hint gives the same answer: one at or past
// nseg, or past the segment sought, restarts the search from segment 0.
BT_GATHER_HD uint32_t gather_seek_seg(const uint64_t *pos, uint32_t nseg, uint64_t m, uint32_t hint) {
  uint32_t lo = hint < nseg ? hint : 0u;
  lo = pos[lo] <= m ? lo : 0u;
  uint32_t step = 1u, hi = nseg;  // pos[lo] <= m; pos[hi] > m, or hi == nseg
  while (lo + step < nseg) {
    const uint32_t k = lo + step;
    if (pos[k] > m) {
      hi = k;
      break;
    }
    lo = k;
    step += step;
  }
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (pos[mid] <= m) lo = mid;
    else hi = mid;
  }
  return lo;
}

// A cursor standing at message byte m (below the listed total), as the walk
// would have left it there; returns the segment through *seg for the next hint.
BT_GATHER_HD void gather_seek(GatherCursor &c, const uint8_t *base, const GatherSeg *segs, const uint64_t *pos,
                              uint32_t nseg, uint64_t m, uint32_t hint, uint32_t *seg) {
  const uint32_t k = gather_seek_seg(pos, nseg, m, hint);
  const GatherSeg s = gather_seg(segs + k);
  const uint32_t in = (uint32_t)(m - pos[k]);
  c.base = base;
  c.segs = segs;
  c.nseg = nseg;
  c.ja = k;
  c.pa = base + s.off + in;
  c.ra = s.len - in;
  c.la = s.len;
  c.total = m;
  gather_load_b(c);
  *seg = k;
}

// gather_bytes with a bound: the next min(limit, what is listed) bytes,
// limit <= 64, and not one byte more -- the r tail bytes of a finishing entry,
// behind which further segments may already be listed.
BT_GATHER_HD uint32_t gather_bytes_upto(GatherCursor &c, uint32_t (&w)[16], uint32_t limit) {
  uint32_t got = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = 0u;
  // Rolled, unlike gather_bytes: the chain-form kernels carry this loop once
  // per instantiation beside their round wave, and its time hides behind R.
  // The word goes into w through selects (a store at a variable index would
  // put w into scratch memory).
#pragma nounroll
  for (uint32_t k = 0; k < 16u && got < limit; ++k) {
    uint32_t v = 0;
#pragma nounroll
    for (uint32_t b = 0; b < 4; ++b) {
      while (got < limit && c.ra == 0 && c.ja + 1 < c.nseg) {
        const GatherSeg s = gather_seg(c.segs + ++c.ja);
        c.pa = c.base + s.off;
        c.ra = c.la = s.len;
      }
      if (got < limit && c.ra) {
        v |= (uint32_t)*c.pa++ << (24u - 8u * b);
        --c.ra;
        ++got;
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) w[j] = gather_sel(j == k, v, w[j]);
  }
  c.total += got;
  return got;
}

// "Block at position": the whole block at message bytes [m, m + 64), all of
// them listed, as 16 big-endian words -- seek, then the walk's two ways to a
// block.  The regular way's loads stay clamped inside A and B; its trailing
// descriptor load (the cursor's next B) is clamped below nseg like the walk's.
BT_GATHER_HD void gather_block_at(uint32_t (&w)[16], const uint8_t *base, const GatherSeg *segs, const uint64_t *pos,
                                  uint32_t nseg, uint64_t m, uint32_t hint, uint32_t *seg) {
  GatherCursor c;
  gather_seek(c, base, segs, pos, nseg, m, hint, seg);
  if (gather_regular(c)) {
    GatherPlan p;
    GatherSlot s;
    gather_plan(c, p);
    gather_fetch(s, p);
    gather_words(w, s);
  } else {
    gather_bytes_upto(c, w, 64u);
  }
}

// Both in one: the `want` bytes (1 .. 64, all listed) at [m, m + want) as
// big-endian words, zero past them -- a whole block by the regular path where
// it applies, anything else by bytes.  One seek and one copy of each path for
// a caller (the chain-form kernels' S wave) that builds blocks and tails alike.
BT_GATHER_HD void gather_span_at(uint32_t (&w)[16], const uint8_t *base, const GatherSeg *segs, const uint64_t *pos,
                                 uint32_t nseg, uint64_t m, uint32_t want, uint32_t hint, uint32_t *seg) {
  GatherCursor c;
  gather_seek(c, base, segs, pos, nseg, m, hint, seg);
  if (want == 64u && gather_regular(c)) {
    GatherPlan p;
    GatherSlot s;
    gather_plan(c, p);
    gather_fetch(s, p);
    gather_words(w, s);
  } else {
    gather_bytes_upto(c, w, want);
  }
}

// The r < 64 bytes at [m, m + r) (listed; r == 0 reads nothing, and m may then
// be the listed total) as big-endian words, zero past them: the tail of a
// finishing entry before the 0x80 mark goes in.
BT_GATHER_HD void gather_tail_at(uint32_t (&w)[16], const uint8_t *base, const GatherSeg *segs, const uint64_t *pos,
                                 uint32_t nseg, uint64_t m, uint32_t r, uint32_t hint) {
#pragma unroll
  for (int k = 0; k < 16; ++k) w[k] = 0u;
  if (r == 0) return;
  GatherCursor c;
  uint32_t seg;
  gather_seek(c, base, segs, pos, nseg, m, hint, &seg);
  gather_bytes_upto(c, w, r);
}

// ---------------------------------------------------------------------------
// The stepper, for the latency-form gather kernel (k_sha1_gather_lat): its S
// wave has lane j stream message j forward like gather_walk, but it meets the
// round wave at one barrier per block, so every lane must yield EXACTLY ONE
// block per call, in control flow the caller can keep wave-uniform --
// gather_walk's loops have lane-dependent trip counts.  gather_step() yields
// block b of the padded message (sha.c:529-543), one of
//   regular   fetched by the call before (one block's loads stay in flight
//             ahead of the block being produced, as in gather_walk);
//   bytes     a whole block the regular path does not take;
//   padding   the r tail bytes + 0x80, the 64-bit bit count in the last block
//             (a block of its own when r >= 56);
// and zeros, reading nothing, once the message is through (b >= nb).  The
// contract above holds, with one addition: `idle` points to 16 readable bytes
// of the CALLER's (any content).  The five loads of a block and its descriptor
// load are issued on every call; a lane with no regular block next aims them
// at `idle` instead of branching around them.  So a call for a lane past its
// message, or for a message with no segments, reads `idle` and nothing else.
// ---------------------------------------------------------------------------

// The message's length: the 64-bit sum of its segment lengths, eight
// descriptors per trip (indices clamped below nseg), so that the pass costs
// nseg / 8 memory round trips and not nseg.
BT_GATHER_HD uint64_t gather_total(const GatherSeg *segs, uint32_t nseg) {
  uint64_t t = 0;
  for (uint32_t j = 0; j < nseg; j += 8u) {
    uint32_t l[8];
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) l[u] = gather_seg(segs + (j + u < nseg ? j + u : nseg - 1u)).len;
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) t += j + u < nseg ? l[u] : 0u;
  }
  return t;
}

struct GatherStepper {
  GatherCursor c;  // behind the last block planned or taken by bytes
  GatherSlot s;    // block b, fetched by the call before, when ahead
  GatherSeg d;     // the descriptor that fetch asked for: the cursor's next B
  uint32_t dsel;   // 0: keep the cursor's B; 1: none follows; 2: d
  uint32_t ahead;
  uint64_t b;          // the block the next call yields
  uint64_t nfull, nb;  // whole blocks; blocks with the padding
  uint64_t bits;
  uint32_t r;
};

// gather_plan + gather_fetch where `go` (which needs gather_regular(c)), the
// same six loads aimed at `idle` and the cursor left alone where not.
//
// The descriptor goes into the cursor one call later (gather_step_settle):
// a select on it here would wait for it on the spot, one memory round trip
// per block ahead of produce_block.
BT_GATHER_HD void gather_fetch_if(GatherStepper &st, bool go, const uint8_t *idle) {
  GatherCursor &c = st.c;
  GatherSlot &s = st.s;
  const uint32_t a = c.ra < 64u ? c.ra : 64u;
  const bool cut = a < 64u;
  const uint8_t *pb = cut ? c.base + c.boff : c.pa;
  GatherPlan p;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t lo = 16u * i;
    const uint8_t *in_a = c.pa + lo, *in_b = pb + lo - a, *win_a = c.pa + a - 16u;
    const uint8_t *q = lo + 16u <= a ? in_a : (lo >= a ? in_b : win_a);
    p.q[i] = go ? q : idle;
  }
  p.wb = go ? pb : idle;
  p.c = a & 15u;
  p.sq = go && cut && p.c ? a >> 4 : 4u;
  const uint32_t into_b = cut ? 64u - a : 0u;
  const bool step = go && (cut || c.ra == 64u);
  const uint64_t boff = c.boff;
  // The descriptor first, as in gather_plan: waiting for it never waits for
  // the block's own loads.
  const uint32_t jb = c.ja + (step ? 2u : 1u);
  const bool has_b = go && jb < c.nseg;
  const uint32_t kb = has_b ? jb : (go ? c.nseg - 1u : 0u);
  __builtin_memcpy(&st.d, go ? (const uint8_t *)(c.segs + kb) : idle, sizeof st.d);
  st.dsel = go ? (has_b ? 2u : 1u) : 0u;
  gather_fetch(s, p);
  c.total += go ? 64u : 0u;
  c.pa = step ? c.base + boff + into_b : c.pa + (go ? 64u : 0u);
  c.ra = step ? c.lb - into_b : c.ra - (go ? 64u : 0u);
  c.la = step ? c.lb : c.la;
  c.ja += step ? 1u : 0u;
}

BT_GATHER_HD void gather_step_settle(GatherStepper &st) {
  st.c.boff = st.dsel ? st.d.off : st.c.boff;
  st.c.lb = st.dsel ? (st.dsel == 2u ? st.d.len : 0u) : st.c.lb;
  st.dsel = 0u;
}

// Block 0's loads.  `len` is gather_total() of the same list.
BT_GATHER_HD void gather_step_begin(GatherStepper &st, const uint8_t *base, const GatherSeg *segs, uint32_t nseg,
                                    uint64_t len, const uint8_t *idle) {
  gather_begin(st.c, base, segs, nseg);
  st.b = 0;
  st.nfull = len >> 6;
  st.r = (uint32_t)len & 63u;
  st.nb = st.nfull + (st.r >= 56u ? 2u : 1u);
  st.bits = len * 8ull;
  const bool go = st.nfull != 0 && gather_regular(st.c);
  gather_fetch_if(st, go, idle);
  st.ahead = go ? 1u : 0u;
}

// w = block b as 16 big-endian words, then the loads of block b + 1.
BT_GATHER_HD void gather_step(GatherStepper &st, uint32_t (&w)[16], const uint8_t *idle) {
  gather_step_settle(st);
  gather_words(w, st.s);
  if (!st.ahead) {
    // By bytes; behind this branch no load is in flight (the slot was waited
    // for above), so its join costs the prefetch nothing.
    const uint32_t want = st.b < st.nfull ? 64u : (st.b == st.nfull ? st.r : 0u);
    gather_bytes_upto(st.c, w, want);  // zeroes w; want == 0 reads nothing
    if (want) gather_load_b(st.c);
    const bool tail = st.b == st.nfull, last = st.b + 1u == st.nb;
    const uint32_t wi = st.r >> 2, mark = 0x80000000u >> ((st.r & 3u) * 8u);
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) w[j] |= tail && j == wi ? mark : 0u;
    w[14] = last ? (uint32_t)(st.bits >> 32) : w[14];
    w[15] = last ? (uint32_t)st.bits : w[15];
  }
  ++st.b;
  const bool go = st.b < st.nfull && gather_regular(st.c);
  gather_fetch_if(st, go, idle);
  st.ahead = go ? 1u : 0u;
}

}  // namespace btsha1
