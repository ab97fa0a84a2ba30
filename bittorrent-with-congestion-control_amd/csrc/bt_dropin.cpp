// bt_dropin.cpp -- the reference's sha.h / chunk.h surface re-implemented over
// the gfx950 kernels: link-compatible with the reference's own callers
// (include/sha.h and include/chunk.h mirror its headers prototype for prototype).
//
// Reference interfaces replaced (yunfanye/Bittorrent-with-Congestion-Control):
//   SHA1Init/SHA1Update/SHA1Final  sha.c:149-163, 453-527, 529-558 (sha.h:58-60)
//   shahash                        chunk.c:33-49  (chunk.h:28)
//   make_chunks                    chunk.c:13-25  (chunk.h:25)
//   binary2hex / hex2binary        chunk.c:55-83  (chunk.h:31,34)
//
// Host-side work here is bookkeeping only (staging, padding-byte layout, hex
// formatting); every compression runs in a HIP kernel.  No CPU hashing path.
#include "bt_runtime.h"
#include "chunk.h"

namespace btsha1 {
namespace {

// Wait for a drop-in call's chain kernel: spin on the completion word it
// stores into pinned memory after its results (a stream wait sleeps and wakes
// late; ~354 such waits per chunk in SHA1Update's packet-sized calls).  The
// stream is polled too, so an error or a kernel that ended without the word
// cannot hang the caller, and after 1 ms the wait blocks on the stream instead
// (long messages do not burn a core; the wake-up latency is then noise).
// BT_SHA1_SYNC=stream always waits on the stream.
bool spin_sync() {
  static const bool on = [] {
    const char *e = getenv("BT_SHA1_SYNC");
    return !(e && !strcmp(e, "stream"));
  }();
  return on;
}

int wait_chain(DevCtx *c, const volatile uint32_t *done, uint32_t seq) {
  if (!spin_sync()) {
    BT_CK(hipStreamSynchronize(c->s));
    return 0;
  }
  const double t0 = now_s();
  for (uint32_t it = 0;; ++it) {
    if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == seq) return 0;
    if ((it & 1023u) == 1023u && now_s() - t0 > 1e-3) {
      BT_CK(hipStreamSynchronize(c->s));
      if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == seq) return 0;
      set_err("chain kernel finished without its completion word");
      return -1;
    }
    if ((it & 63u) == 63u) {
      const hipError_t q = hipStreamQuery(c->s);
      if (q == hipSuccess) {
        if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == seq) return 0;
        set_err("chain kernel finished without its completion word");
        return -1;
      }
      if (q != hipErrorNotReady) {
        set_err("chain kernel: %s", hipGetErrorString(q));
        return -1;
      }
    }
  }
}

uint32_t *done_word(DevCtx *c) { return reinterpret_cast<uint32_t *>(c->h_state.as<uint8_t>() + 32); }

// The reference leaves no copy of the message or of the chaining state behind
// a call: shahash zeroes its context (chunk.c:48) and SHA1Update burns its
// stack frame (sha.c:165-174, 526).  The drop-in's copies live in the
// context's pinned staging, so each call zeroes what it staged there once the
// chain kernel has finished with it (explicit_bzero: not elided as a dead
// store).  The completion word at h_state + 32 is a sequence number, not data.
void wipe_staging(DevCtx *c, size_t msg_bytes) {
  if (msg_bytes) explicit_bzero(c->h_msg.p, std::min(msg_bytes, c->h_msg.cap));
  explicit_bzero(c->h_state.p, kStateBytes);
}

// Single message on the GPU (shahash): copy it into the context's pinned
// staging buffer and launch the chain kernel on it there -- the kernel reads
// the message over PCIe itself (64 blocks per load batch, far ahead of the
// round wave) and writes the digest straight into pinned memory -- so one
// synchronous call is one memcpy, one launch and a wait on the kernel's
// completion word: no H2D or D2H copies (each a queue round trip of its own).
int hash_one(DevCtx *c, const uint8_t *buf, uint32_t len, uint8_t out[20]) {
  if (ensure_streams(c)) return -1;
  if (c->h_msg.ensure((size_t)len + 64) || c->h_state.ensure(64)) return -1;
  if (len) memcpy(c->h_msg.p, buf, len);
  const uint32_t seq = ++c->seq;
  *done_word(c) = seq - 1u;
  const hipError_t e = btsha1_launch_chain_one(c->h_msg.p, len, c->h_state.as<uint8_t>(), c->s, done_word(c), seq);
  if (e != hipSuccess) set_err("chain kernel launch: %s", hipGetErrorString(e));
  const int rc = e != hipSuccess ? -1 : wait_chain(c, done_word(c), seq);
  if (!rc) memcpy(out, c->h_state.p, 20);
  wipe_staging(c, len);
  return rc;
}

// Advance h over `head` (0 or 64 bytes: SHA1Update's completed staging block)
// followed by nblocks whole blocks at host address `blocks`: both go straight
// into pinned memory with the state, the chain kernel reads them from there
// and writes the state back in place (one launch, one wait per call).
int midstate(DevCtx *c, uint32_t h[5], const uint8_t *head, const uint8_t *blocks, uint64_t nblocks) {
  const uint64_t total = nblocks + (head ? 1 : 0);
  if (!total) return 0;
  if (ensure_streams(c)) return -1;
  if (c->h_msg.ensure((size_t)total * 64) || c->h_state.ensure(64)) return -1;
  uint8_t *dst = c->h_msg.as<uint8_t>();
  if (head) memcpy(dst, head, 64);
  if (nblocks) memcpy(dst + (head ? 64 : 0), blocks, (size_t)nblocks * 64);
  memcpy(c->h_state.p, h, 20);
  nblocks = total;
  const uint32_t seq = ++c->seq;
  *done_word(c) = seq - 1u;
  const hipError_t e = btsha1_launch_chain_midstate(c->h_state.as<uint32_t>(), c->h_msg.p, nblocks, c->s,
                                                    done_word(c), seq);
  if (e != hipSuccess) set_err("chain kernel launch: %s", hipGetErrorString(e));
  const int rc = e != hipSuccess ? -1 : wait_chain(c, done_word(c), seq);
  if (!rc) memcpy(h, c->h_state.p, 20);
  wipe_staging(c, (size_t)total * 64);
  return rc;
}

DevCtx *dropin_ctx(const char *who) {
  DevCtx *c = ctx_for(t_dev);
  if (!c) die(who);
  if (hipSetDevice(t_dev) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", t_dev);
    die(who);
  }
  return c;
}

}  // namespace
}  // namespace btsha1

using namespace btsha1;

extern "C" {

// ---- drop-in: chunk.h --------------------------------------------------------

// chunk.c:13-25.  Same contract: reads fp to EOF in BT_CHUNK_SIZE pieces,
// digest i -> chunk_hashes[i] (caller-sized, as make_chunks.c:32-45 does).
int make_chunks(FILE *fp, uint8_t **chunk_hashes) {
  if (!fp || !chunk_hashes) {
    set_err("null pointer");
    return -1;
  }
  int64_t n = chunks_file_on(t_dev, fp, BT_CHUNK_SIZE, [&](uint64_t first, uint64_t count, const uint8_t *d) {
    for (uint64_t i = 0; i < count; ++i) memcpy(chunk_hashes[first + i], d + 20 * i, 20);
  });
  if (n < 0) {
    fprintf(stderr, "make_chunks: %s\n", t_err.c_str());
    return -1;
  }
  return (int)n;
}

// chunk.c:33-49 (int length, like the reference).
void shahash(uint8_t *str, int len, uint8_t *hash) {
  if (len < 0) {
    set_err("negative length %d", len);
    die("shahash");
  }
  KeepDevice keep_dev;
  DevCtx *c = dropin_ctx("shahash");
  std::lock_guard<std::mutex> g(c->mu);
  if (hash_one(c, str, (uint32_t)len, hash)) die("shahash");
}

// chunk.c:55-61: "%.2x" per byte, NUL-terminated.
void binary2hex(uint8_t *buf, int len, char *hex) {
  static const char dig[] = "0123456789abcdef";
  for (int i = 0; i < len; ++i) {
    hex[2 * i] = dig[buf[i] >> 4];
    hex[2 * i + 1] = dig[buf[i] & 15];
  }
  hex[len < 0 ? 0 : 2 * len] = 0;
}

// chunk.c:66-83: toupper, '0'..'9' -> 0..9, otherwise ch - ('A' - 10); no
// validation (kept bug-compatible: garbage in, garbage out).
static inline uint8_t hexval(char ch) {
  if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 32);
  return (uint8_t)(ch <= '9' ? ch - '0' : ch - ('A' - 10));
}
void hex2binary(char *hex, int len, uint8_t *buf) {
  for (int i = 0; i < len; i += 2) buf[i / 2] = (uint8_t)((hexval(hex[i]) << 4) | hexval(hex[i + 1]));
}

// ---- drop-in: sha.h ------------------------------------------------------------

void SHA1Init(SHA1Context *sc) {  // sha.c:149-163
  sc->totalLength = 0;
  sc->hash[0] = 0x67452301u;
  sc->hash[1] = 0xefcdab89u;
  sc->hash[2] = 0x98badcfeu;
  sc->hash[3] = 0x10325476u;
  sc->hash[4] = 0xc3d2e1f0u;
  sc->bufferLength = 0;
}

// sha.c:453-527: bytes top up the 64-byte staging block; every completed
// block (the staged one plus all whole blocks of `data`) is compressed in one
// GPU call; the remainder is staged.  totalLength counts bits like sha.c:511.
void SHA1Update(SHA1Context *sc, const void *vdata, uint32_t len) {
  if (!len) return;
  const uint8_t *p = (const uint8_t *)vdata;
  sc->totalLength += (uint64_t)len * 8u;
  uint32_t take = 0;
  if (sc->bufferLength) {
    take = std::min<uint32_t>(64u - sc->bufferLength, len);
    memcpy(sc->buffer.bytes + sc->bufferLength, p, take);
    sc->bufferLength += take;
    p += take;
    len -= take;
    if (sc->bufferLength < 64u) return;
  }
  const uint64_t nfull = len / 64u;
  const bool staged_full = sc->bufferLength == 64u;
  if (staged_full || nfull) {
    KeepDevice keep_dev;
    DevCtx *c = dropin_ctx("SHA1Update");
    std::lock_guard<std::mutex> g(c->mu);
    if (midstate(c, sc->hash, staged_full ? sc->buffer.bytes : nullptr, p, nfull)) die("SHA1Update");
    sc->bufferLength = 0;
  }
  const uint32_t rest = len - (uint32_t)(64u * nfull);
  if (rest) {
    memcpy(sc->buffer.bytes, p + 64u * nfull, rest);
    sc->bufferLength = rest;
  }
}

// sha.c:529-558: 0x80, zeros to 56 mod 64, 64-bit big-endian bit count; the
// last one or two blocks are compressed on the GPU; digest big-endian.
void SHA1Final(SHA1Context *sc, uint8_t hash[SHA1_HASH_SIZE]) {
  const uint32_t bl = sc->bufferLength;
  uint32_t npad = 120u - bl;
  if (npad > 64u) npad -= 64u;
  uint8_t blk[128];
  memset(blk, 0, sizeof blk);
  memcpy(blk, sc->buffer.bytes, bl);
  blk[bl] = 0x80;
  const uint64_t bits = sc->totalLength;
  const uint32_t end = bl + npad + 8u;  // 64 or 128
  for (int i = 0; i < 8; ++i) blk[end - 8 + i] = (uint8_t)(bits >> (56 - 8 * i));
  KeepDevice keep_dev;
  DevCtx *c = dropin_ctx("SHA1Final");
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (midstate(c, sc->hash, nullptr, blk, end / 64u)) die("SHA1Final");
  }
  explicit_bzero(blk, sizeof blk);  // the message tail (sha.c:165-174's burnStack)
  sc->totalLength += (uint64_t)(npad + 8u) * 8u;
  sc->bufferLength = 0;
  if (hash)
    for (int i = 0; i < SHA1_HASH_WORDS; ++i) {
      hash[4 * i] = (uint8_t)(sc->hash[i] >> 24);
      hash[4 * i + 1] = (uint8_t)(sc->hash[i] >> 16);
      hash[4 * i + 2] = (uint8_t)(sc->hash[i] >> 8);
      hash[4 * i + 3] = (uint8_t)sc->hash[i];
    }
}

}  // extern "C"
