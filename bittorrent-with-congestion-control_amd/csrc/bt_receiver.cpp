// bt_receiver.cpp -- the progressive receiver (bt_sha1_receiver_*,
// include/bt_sha1.h): a chunk is hashed WHILE it is received.
//
// Reference interface replaced (yunfanye/Bittorrent-with-Congestion-Control):
//   save_data_packet + save_chunk   util.c:250-337, for in-order delivery
// The reference appends each payload at chunk->data + received_byte_number
// (util.c:275) and hashes all 512 KiB once the chunk is complete
// (util.c:311-313): one serial chain after the last packet.  Here every slot
// carries its chaining state, and whenever `stride` bytes of new whole blocks
// have arrived one launch of the resumable chain kernel (k_sha1_resume)
// advances the state over them, reading the pinned slot in place over PCIe;
// commit then hashes only what is left, appends the padding and compares.
//
// Each slot's launches are ordered on one stream; the slots are spread over
// at most four non-blocking streams (HIP maps streams onto 4 hardware queues
// here, and streams that share a queue serialise: DESIGN.md §6).  Every launch
// stores the slot's sequence number into a pinned completion word after its
// results, so poll reads memory and never waits on a stream.
//
// Host-side work here is bookkeeping only; every compression runs in a HIP
// kernel.  No CPU hashing path.
#include "bt_runtime.h"

#include <deque>

namespace btsha1 {
namespace {

constexpr uint32_t kMaxSlots = 64, kStreams = 4;
constexpr uint32_t kDefaultStride = 64u << 10;
constexpr uint32_t kMaxChunk = 32u << 20;
// Pinned control block of a slot, two 64-byte lines: the first is written by
// the host between launches (expected hash) and carries the chaining state,
// the second is written by the finishing kernel and polled by the host.
constexpr size_t kCtl = 128;
constexpr uint32_t kIV[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};  // sha.c:149-163

enum : uint32_t { kFree = 0, kOut = 1, kCommitted = 2 };

struct RSlot {
  uint8_t *data = nullptr, *ctl = nullptr;
  uint32_t status = kFree;
  uint32_t filled = 0, hashed = 0;  // bytes the caller called final / bytes queued for hashing
  uint32_t seq = 0;                 // what the slot's last queued launch stores in its completion word
  uint64_t tag = 0;
  uint32_t *state() const { return reinterpret_cast<uint32_t *>(ctl); }
  uint8_t *expected() const { return ctl + 20; }
  uint8_t *digest() const { return ctl + 64; }
  uint8_t *ok() const { return ctl + 84; }
  uint32_t *done() const { return reinterpret_cast<uint32_t *>(ctl + 88); }
  bool idle() const { return __atomic_load_n(done(), __ATOMIC_ACQUIRE) == seq; }
  void restart() {
    memcpy(state(), kIV, sizeof kIV);
    filled = hashed = 0;
  }
};

struct Done {
  bt_sha1_verdict v;
};

struct Receiver {
  int dev = 0;
  uint32_t chunk_len = 0, nslots = 0, stride = 0;
  size_t pitch = 0;
  uint8_t *h_data = nullptr, *h_ctl = nullptr;
  hipStream_t streams[kStreams] = {};
  RSlot slot[kMaxSlots];
  uint32_t order[kMaxSlots];  // committed slots, oldest first
  uint32_t norder = 0;
  uint32_t empty_polls = 0;
  std::deque<Done> done;
  int64_t queued = 0;  // committed, verdict not yet returned
  bt_sha1_receiver_stats stats = {};
};

Receiver *impl(bt_sha1_receiver *r) { return reinterpret_cast<Receiver *>(r); }

hipStream_t &stream_of(Receiver *r, const RSlot &s) { return r->streams[(uint32_t)(&s - r->slot) % kStreams]; }

// Wait for the slot's queued launches: spin on its completion word, watching
// the stream as wait_chain does (bt_dropin.cpp), so a failed launch or a
// kernel that ended without the word returns -1 instead of spinning forever;
// after 1 ms the wait blocks on the stream.
int wait_slot(Receiver *r, RSlot &s) {
  if (s.idle()) return 0;
  hipStream_t st = stream_of(r, s);
  const double t0 = now_s();
  for (uint32_t it = 0;; ++it) {
    if (s.idle()) return 0;
    const bool late = (it & 1023u) == 1023u && now_s() - t0 > 1e-3;
    if (late || (it & 63u) == 63u) {
      const hipError_t q = late ? hipStreamSynchronize(st) : hipStreamQuery(st);
      if (q == hipSuccess) {
        if (s.idle()) return 0;
        set_err("receiver: resume kernel finished without its completion word");
        return -1;
      }
      if (q != hipErrorNotReady) {
        set_err("receiver: resume kernel: %s", hipGetErrorString(q));
        return -1;
      }
    }
  }
}

// One launch over bytes [from, to) of the slot: an advance (total == 0) or
// the finish of a total-byte chunk with the fused compare.
int launch(Receiver *r, RSlot &s, uint32_t from, uint32_t to, uint64_t total) {
  hipStream_t &st = stream_of(r, s);
  if (!st) BT_CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  const uint32_t seq = s.seq + 1u;
  const hipError_t e =
      btsha1_launch_resume_one(s.data + from, to - from, total, s.state(), total ? s.digest() : nullptr,
                               total ? s.expected() : nullptr, total ? s.ok() : nullptr, st, s.done(), seq);
  if (e != hipSuccess) {
    set_err("receiver: resume kernel launch: %s", hipGetErrorString(e));
    return -1;
  }
  s.seq = seq;
  ++r->stats.launches;
  return 0;
}

void harvest(Receiver *r, uint32_t k) {
  RSlot &s = r->slot[k];
  Done d;
  d.v.tag = s.tag;
  d.v.ok = *s.ok() ? 1 : 0;
  memcpy(d.v.digest, s.digest(), 20);
  r->done.push_back(d);
  s.status = kFree;
}

// Committed slots whose finishing kernel has stored its completion word.
int harvest_ready(Receiver *r) {
  uint32_t keep = 0, got = 0;
  for (uint32_t j = 0; j < r->norder; ++j) {
    const uint32_t k = r->order[j];
    if (r->slot[k].idle()) {
      harvest(r, k);
      ++got;
    } else {
      r->order[keep++] = k;
    }
  }
  r->norder = keep;
  return (int)got;
}

int take(Receiver *r, bt_sha1_verdict *out, int max) {
  int n = 0;
  while (n < max && !r->done.empty()) {
    out[n++] = r->done.front().v;
    r->done.pop_front();
  }
  r->queued -= n;
  return n;
}

// Slot pointer -> outstanding slot; NULL with a message otherwise.
RSlot *locate(Receiver *r, const uint8_t *p) {
  if (p >= r->h_data && p < r->h_data + r->pitch * r->nslots && (size_t)(p - r->h_data) % r->pitch == 0) {
    RSlot &s = r->slot[(size_t)(p - r->h_data) / r->pitch];
    if (s.status == kOut) return &s;
  }
  set_err("receiver: pointer is not an outstanding slot");
  return nullptr;
}

}  // namespace
}  // namespace btsha1

using namespace btsha1;

extern "C" {

bt_sha1_receiver *bt_sha1_receiver_create(int device, uint32_t chunk_len, uint32_t nslots, uint32_t stride) {
  if (chunk_len == 0 || chunk_len > kMaxChunk) {
    set_err("receiver: chunk_len must be in [1, 32 MiB]");
    return nullptr;
  }
  if (nslots == 0 || nslots > kMaxSlots) {
    set_err("receiver: nslots must be in [1, %u]", kMaxSlots);
    return nullptr;
  }
  if (!ctx_for(device)) return nullptr;
  KeepDevice keep_dev;
  if (hipSetDevice(device) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", device);
    return nullptr;
  }
  auto *r = new Receiver;
  r->dev = device;
  r->chunk_len = chunk_len;
  r->nslots = nslots;
  r->stride = stride ? stride : kDefaultStride;
  r->pitch = ((size_t)chunk_len + 63) & ~(size_t)63;
  if (hipHostMalloc((void **)&r->h_data, r->pitch * nslots, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&r->h_ctl, kCtl * nslots, hipHostMallocDefault) != hipSuccess) {
    set_err("receiver: allocation of %u pinned slots of %u bytes failed", nslots, chunk_len);
    bt_sha1_receiver_destroy(reinterpret_cast<bt_sha1_receiver *>(r));
    return nullptr;
  }
  memset(r->h_ctl, 0, kCtl * nslots);
  for (uint32_t k = 0; k < nslots; ++k) {
    r->slot[k].data = r->h_data + k * r->pitch;
    r->slot[k].ctl = r->h_ctl + k * kCtl;
    r->slot[k].restart();
  }
  return reinterpret_cast<bt_sha1_receiver *>(r);
}

void bt_sha1_receiver_destroy(bt_sha1_receiver *rr) {
  Receiver *r = impl(rr);
  if (!r) return;
  KeepDevice keep_dev;
  (void)hipSetDevice(r->dev);
  for (hipStream_t st : r->streams)
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  if (r->h_data) (void)hipHostFree(r->h_data);
  if (r->h_ctl) (void)hipHostFree(r->h_ctl);
  delete r;
}

uint8_t *bt_sha1_receiver_slot(bt_sha1_receiver *rr) {
  Receiver *r = impl(rr);
  if (!r) {
    set_err("null pointer");
    return nullptr;
  }
  for (int pass = 0; pass < 2; ++pass) {
    for (uint32_t k = 0; k < r->nslots; ++k) {
      RSlot &s = r->slot[k];
      if (s.status != kFree) continue;
      s.restart();  // nothing of the slot is in flight: it was harvested, released or never used
      s.status = kOut;
      return s.data;
    }
    if (pass || !harvest_ready(r)) break;  // a finished chunk's slot is free again
  }
  set_err("receiver: all %u slots are outstanding (commit or release one, or take its verdict)", r->nslots);
  return nullptr;
}

int bt_sha1_receiver_advance(bt_sha1_receiver *rr, uint8_t *slot, uint32_t filled) {
  Receiver *r = impl(rr);
  if (!r || !slot) {
    set_err("null pointer");
    return -1;
  }
  RSlot *s = locate(r, slot);
  if (!s) return -1;
  if (filled < s->filled || filled > r->chunk_len) {
    set_err("receiver: filled = %u must not decrease (was %u) or exceed chunk_len %u", filled, s->filled,
            r->chunk_len);
    return -1;
  }
  s->filled = filled;
  const uint32_t whole = filled & ~63u;
  if (whole <= s->hashed || whole - s->hashed < r->stride) return 0;
  KeepDevice keep_dev;
  if (hipSetDevice(r->dev) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", r->dev);
    return -1;
  }
  if (launch(r, *s, s->hashed, whole, 0)) return -1;
  ++r->stats.advance_launches;
  r->stats.advanced_bytes += whole - s->hashed;
  s->hashed = whole;
  return 0;
}

int bt_sha1_receiver_commit(bt_sha1_receiver *rr, uint8_t *slot, uint32_t len, const uint8_t expected[20],
                            uint64_t tag) {
  Receiver *r = impl(rr);
  if (!r || !slot || !expected) {
    set_err("null pointer");
    return -1;
  }
  RSlot *s = locate(r, slot);
  if (!s) return -1;
  if (len == 0 || len < s->hashed || len > r->chunk_len) {
    set_err("receiver: commit of %u bytes: must be in [max(1, %u already hashed), chunk_len %u]", len, s->hashed,
            r->chunk_len);
    return -1;
  }
  KeepDevice keep_dev;
  if (hipSetDevice(r->dev) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", r->dev);
    return -1;
  }
  memcpy(s->expected(), expected, 20);
  if (launch(r, *s, s->hashed, len, len)) return -1;
  s->tag = tag;
  s->filled = len;
  s->status = kCommitted;
  r->order[r->norder++] = (uint32_t)(s - r->slot);
  ++r->queued;
  ++r->stats.committed;
  return 0;
}

int bt_sha1_receiver_release(bt_sha1_receiver *rr, uint8_t *slot) {
  Receiver *r = impl(rr);
  if (!r || !slot) {
    set_err("null pointer");
    return -1;
  }
  RSlot *s = locate(r, slot);
  if (!s) return -1;
  if (!s->idle()) {  // advances still queued on the slot: it is handed out again only after them
    KeepDevice keep_dev;
    if (hipSetDevice(r->dev) != hipSuccess) {
      set_err("hipSetDevice(%d) failed", r->dev);
      return -1;
    }
    if (wait_slot(r, *s)) return -1;
  }
  s->restart();
  s->status = kFree;
  ++r->stats.released;
  return 0;
}

int bt_sha1_receiver_poll(bt_sha1_receiver *rr, bt_sha1_verdict *out, int max) {
  Receiver *r = impl(rr);
  if (!r || (!out && max > 0)) {
    set_err("null pointer");
    return -1;
  }
  if (harvest_ready(r) || r->norder == 0 || !r->done.empty()) {
    r->empty_polls = 0;
    return take(r, out, max);
  }
  // Nothing finished.  Every 64th such poll in a row looks at the oldest
  // chunk's stream (a query, not a wait), so a failed launch surfaces here too.
  if ((++r->empty_polls & 63u) == 0) {
    RSlot &s = r->slot[r->order[0]];
    const hipError_t q = hipStreamQuery(stream_of(r, s));
    if (q == hipSuccess && !s.idle()) {
      set_err("receiver: resume kernel finished without its completion word");
      return -1;
    }
    if (q != hipSuccess && q != hipErrorNotReady) {
      set_err("receiver: resume kernel: %s", hipGetErrorString(q));
      return -1;
    }
  }
  return 0;
}

int bt_sha1_receiver_drain(bt_sha1_receiver *rr, bt_sha1_verdict *out, int max) {
  Receiver *r = impl(rr);
  if (!r || (!out && max > 0)) {
    set_err("null pointer");
    return -1;
  }
  if (r->norder) {
    KeepDevice keep_dev;
    if (hipSetDevice(r->dev) != hipSuccess) {
      set_err("hipSetDevice(%d) failed", r->dev);
      return -1;
    }
    for (uint32_t j = 0; j < r->norder; ++j)
      if (wait_slot(r, r->slot[r->order[j]])) return -1;
    harvest_ready(r);
  }
  return take(r, out, max);
}

int64_t bt_sha1_receiver_pending(bt_sha1_receiver *r) { return r ? impl(r)->queued : -1; }

int bt_sha1_receiver_get_stats(bt_sha1_receiver *r, bt_sha1_receiver_stats *out) {
  if (!r || !out) {
    set_err("null pointer");
    return -1;
  }
  *out = impl(r)->stats;
  return 0;
}

}  // extern "C"
