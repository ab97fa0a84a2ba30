// bt_intake.cpp -- progressive receive for many chunks at once
// (bt_sha1_intake_*, include/bt_sha1.h): the receiver's slot life cycle for up
// to 512 chunks in flight, every due slot advanced by ONE launch.
//
// Reference interface replaced (yunfanye/Bittorrent-with-Congestion-Control):
//   save_data_packet + save_chunk   util.c:250-337, for in-order delivery
// The receiver (bt_receiver.cpp) queues one single-workgroup launch per slot
// per stride, so at most four chains advance at a time.  Here advance and
// commit only RECORD what has arrived; kick builds one table from every slot
// that is due and has no launch in flight, and queues one launch of the
// table-driven resumable chain kernel (k_sha1_resume_table) whose workgroup w
// serves table entry w.  A slot is in at most one queued launch at a time, so
// launches need no ordering among themselves: they are issued round-robin over
// at most four non-blocking streams.  Every entry stores its
// slot's sequence number into the slot's pinned completion word after its
// results, so poll reads memory and never waits on a stream.
//
// Host-side work here is bookkeeping only; every compression runs in a HIP
// kernel.  No CPU hashing path.
#include "bt_runtime.h"

#include <cstddef>
#include <deque>

namespace btsha1 {
namespace {

constexpr uint32_t kMaxSlots = BTSHA1_TABLE_MAX, kStreams = 4;
constexpr uint32_t kTables = 8;  // ring of tables: launches that may be in flight at once
constexpr uint32_t kDefaultStride = 64u << 10;
constexpr uint32_t kMaxChunk = 32u << 20;
constexpr uint64_t kMaxPinned = 2ull << 30;  // what the host pipelines keep: 2 x 1 GiB lanes
constexpr size_t kCtl = BTSHA1_TABLE_CTL;    // the receiver's control block (bt_receiver.cpp)
constexpr uint32_t kMaxGatherSlot = 33u << 20;   // the gather verifier's slot bound (bt_verifier.cpp)
constexpr uint64_t kMaxSegTables = 256ull << 20;  // descriptors + positions, 24 bytes per segment
// A gather entry is a table entry with two of its pad words in use: the ring
// of tables, published() and launch_finished() serve both kinds.
static_assert(offsetof(BtSha1GatherEntry, slot) == offsetof(BtSha1TableEntry, slot) &&
                  offsetof(BtSha1GatherEntry, from) == offsetof(BtSha1TableEntry, from) &&
                  offsetof(BtSha1GatherEntry, len) == offsetof(BtSha1TableEntry, len) &&
                  offsetof(BtSha1GatherEntry, total) == offsetof(BtSha1TableEntry, total) &&
                  offsetof(BtSha1GatherEntry, seq) == offsetof(BtSha1TableEntry, seq) &&
                  offsetof(BtSha1GatherEntry, nseg) == offsetof(BtSha1TableEntry, pad) &&
                  sizeof(BtSha1GatherEntry) == sizeof(BtSha1TableEntry),
              "gather entry layout");
constexpr uint32_t kIV[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};  // sha.c:149-163

enum : uint32_t { kFree = 0, kOut = 1, kCommitted = 2 };

struct ISlot {
  uint8_t *data = nullptr, *ctl = nullptr;
  uint32_t status = kFree;
  uint32_t filled = 0, hashed = 0;  // bytes the caller called final / bytes queued for hashing
  uint32_t len = 0;                 // committed length
  uint32_t seq = 0;                 // what the slot's last queued entry stores in its completion word
  uint32_t table = 0;               // ring index of the launch that carried it
  bool due = false;                 // a span or a commit waits for the next kick
  bool finishing = false;           // committed and its finishing entry is queued
  bool expected_held = false;       // commit found a launch in flight: `held` goes in at the finishing kick
  uint8_t held[20] = {};
  uint64_t tag = 0;
  // Gather intake: segments listed so far (their bytes are `filled`) and the
  // segment that holds message byte `hashed`, the next entry's seg_hint.
  uint32_t nseg = 0, hint = 0;
  uint32_t *state() const { return reinterpret_cast<uint32_t *>(ctl); }
  uint8_t *expected() const { return ctl + 20; }
  uint8_t *digest() const { return ctl + 64; }
  uint8_t *ok() const { return ctl + 84; }
  uint32_t *done() const { return reinterpret_cast<uint32_t *>(ctl + 88); }
  bool idle() const { return __atomic_load_n(done(), __ATOMIC_ACQUIRE) == seq; }
  void restart() {
    memcpy(state(), kIV, sizeof kIV);
    filled = hashed = len = 0;
    nseg = hint = 0;
    due = finishing = expected_held = false;
  }
};

struct Done {
  bt_sha1_verdict v;
};

// One queued launch: its table in the pinned ring and the stream it went to.
struct Flight {
  uint32_t n = 0;
  hipStream_t st = nullptr;
};

struct Intake {
  int dev = 0;
  uint32_t chunk_len = 0, nslots = 0, stride = 0;
  size_t pitch = 0;
  uint8_t *h_data = nullptr, *h_ctl = nullptr;
  BtSha1TableEntry *h_tables = nullptr;  // kTables x kMaxSlots entries
  // Gather intake (slots hold datagrams): per slot max_segs descriptors and
  // their message positions, pinned; the kernel reads them in place.
  bool gather = false;
  uint32_t max_segs = 0;
  bt_sha1_seg *h_segs = nullptr;
  uint64_t *h_pos = nullptr;
  bt_sha1_seg *segs(const ISlot &s) const { return h_segs + (size_t)(&s - slot) * max_segs; }
  uint64_t *pos(const ISlot &s) const { return h_pos + (size_t)(&s - slot) * max_segs; }
  hipStream_t streams[kStreams] = {};
  ISlot slot[kMaxSlots];
  uint32_t order[kMaxSlots];  // committed slots, oldest first
  uint32_t norder = 0, ndue = 0;
  uint32_t empty_polls = 0;
  Flight flight[kTables];
  uint64_t head = 0, tail = 0;  // launches queued / retired; table of launch k is k % kTables
  std::deque<Done> done;
  int64_t queued = 0;  // committed, verdict not yet returned
  bt_sha1_intake_stats stats = {};
  BtSha1TableEntry *table(uint64_t k) const { return h_tables + (k % kTables) * kMaxSlots; }
};

Intake *impl(bt_sha1_intake *r) { return reinterpret_cast<Intake *>(r); }

void set_due(Intake *r, ISlot &s, bool due) {
  if (s.due != due) r->ndue += due ? 1u : -1u;
  s.due = due;
}

// Has entry e's workgroup published?  A slot's sequence numbers only grow and a
// later entry is queued only after this one finished, so "at or past" it is.
bool published(const Intake *r, const BtSha1TableEntry &e) {
  return (int32_t)(__atomic_load_n(r->slot[e.slot].done(), __ATOMIC_ACQUIRE) - e.seq) >= 0;
}

bool launch_finished(const Intake *r, uint64_t k) {
  const BtSha1TableEntry *t = r->table(k);
  for (uint32_t j = 0; j < r->flight[k % kTables].n; ++j)
    if (!published(r, t[j])) return false;
  return true;
}

// Spin until `ready` holds, watching stream st as the receiver's wait_slot
// does: a failed launch or a kernel that ended without its completion words
// returns -1 instead of spinning forever; after 1 ms the wait blocks on the
// stream.
template <class Ready>
int wait_on(hipStream_t st, Ready ready) {
  if (ready()) return 0;
  const double t0 = now_s();
  for (uint32_t it = 0;; ++it) {
    if (ready()) return 0;
    const bool late = (it & 1023u) == 1023u && now_s() - t0 > 1e-3;
    if (late || (it & 63u) == 63u) {
      const hipError_t q = late ? hipStreamSynchronize(st) : hipStreamQuery(st);
      if (q == hipSuccess) {
        if (ready()) return 0;
        set_err("intake: resume kernel finished without its completion word");
        return -1;
      }
      if (q != hipErrorNotReady) {
        set_err("intake: resume kernel: %s", hipGetErrorString(q));
        return -1;
      }
    }
  }
}

int wait_launch(Intake *r, uint64_t k) {
  return wait_on(r->flight[k % kTables].st, [&] { return launch_finished(r, k); });
}

int wait_slot(Intake *r, ISlot &s) {
  if (s.idle()) return 0;
  return wait_on(r->flight[s.table].st, [&] { return s.idle(); });
}

// Retire finished launches from the old end of the ring (their tables are free again).
void retire(Intake *r) {
  while (r->tail < r->head && launch_finished(r, r->tail)) ++r->tail;
}

int set_device(Intake *r) {
  if (hipSetDevice(r->dev) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", r->dev);
    return -1;
  }
  return 0;
}

// One table of every due slot with no launch in flight, one launch.  The
// slots' bookkeeping moves only once the launch is queued.
int kick(Intake *r) {
  ++r->stats.kicks;
  if (r->ndue == 0) return 0;
  uint32_t ready = 0;
  for (uint32_t k = 0; k < r->nslots; ++k) {
    const ISlot &s = r->slot[k];
    if (!s.due) continue;
    if (s.idle()) ++ready;
    else ++r->stats.deferred;
  }
  if (ready == 0) return 0;
  KeepDevice keep_dev;
  if (set_device(r)) return -1;
  retire(r);
  if (r->head - r->tail == kTables) {  // the ring is full: the oldest launch's table is needed
    if (wait_launch(r, r->tail)) return -1;
    retire(r);
  }
  BtSha1TableEntry *t = r->table(r->head);
  uint32_t n = 0;
  for (uint32_t k = 0; k < r->nslots && n < ready; ++k) {
    ISlot &s = r->slot[k];
    if (!s.due || !s.idle()) continue;
    BtSha1TableEntry &e = t[n++];
    e.slot = k;
    e.from = s.hashed;
    e.seq = s.seq + 1u;
    if (s.status == kCommitted) {  // whatever is left and the padding, in one finishing entry
      if (s.expected_held) memcpy(s.expected(), s.held, 20);
      e.len = s.len - s.hashed;
      e.total = s.len;
    } else {
      e.len = (s.filled & ~63u) - s.hashed;
      e.total = 0;
    }
    e.pad[0] = e.pad[1] = e.pad[2] = 0;
    if (r->gather) {  // the same 32 bytes as a BtSha1GatherEntry: what is listed now, and where `from` lies
      BtSha1GatherEntry &g = reinterpret_cast<BtSha1GatherEntry &>(e);
      g.nseg = s.nseg;
      g.seg_hint = s.hint;
    }
  }
  hipStream_t &st = r->streams[r->head % kStreams];
  if (!st) BT_CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  const hipError_t err =
      r->gather ? btsha1_launch_gather_resume_table(reinterpret_cast<const BtSha1GatherEntry *>(t), n, r->h_data,
                                                    r->pitch, r->h_segs, r->h_pos, r->max_segs, r->h_ctl, true, st)
                : btsha1_launch_resume_table(t, n, r->h_data, r->pitch, r->h_ctl, true, st);
  if (err != hipSuccess) {
    set_err("intake: resume kernel launch: %s", hipGetErrorString(err));
    return -1;
  }
  const uint32_t ring = (uint32_t)(r->head % kTables);
  r->flight[ring].n = n;
  r->flight[ring].st = st;
  ++r->head;
  for (uint32_t j = 0; j < n; ++j) {
    ISlot &s = r->slot[t[j].slot];
    s.seq = t[j].seq;
    s.table = ring;
    if (s.status == kCommitted) {
      s.finishing = true;
      s.expected_held = false;
    } else {
      r->stats.advanced_bytes += t[j].len;
    }
    s.hashed += t[j].len;
    if (r->gather) {  // the segment that holds the next entry's first byte
      const uint64_t *pos = r->pos(s);
      while (s.hint + 1u < s.nseg && pos[s.hint + 1u] <= s.hashed) ++s.hint;
    }
    set_due(r, s, false);
  }
  ++r->stats.launches;
  r->stats.entries += n;
  if (n > r->stats.max_entries) r->stats.max_entries = n;
  return (int)n;
}

// Wait for every queued launch; launches nothing.
int sync_all(Intake *r) {
  if (r->tail == r->head) return 0;
  KeepDevice keep_dev;
  if (set_device(r)) return -1;
  while (r->tail < r->head) {
    if (wait_launch(r, r->tail)) return -1;
    ++r->tail;
  }
  return 0;
}

void harvest(Intake *r, uint32_t k) {
  ISlot &s = r->slot[k];
  Done d;
  d.v.tag = s.tag;
  d.v.ok = *s.ok() ? 1 : 0;
  memcpy(d.v.digest, s.digest(), 20);
  r->done.push_back(d);
  s.status = kFree;
}

// Committed slots whose finishing entry has stored its completion word.
int harvest_ready(Intake *r) {
  uint32_t keep = 0, got = 0;
  for (uint32_t j = 0; j < r->norder; ++j) {
    const uint32_t k = r->order[j];
    if (r->slot[k].finishing && r->slot[k].idle()) {
      harvest(r, k);
      ++got;
    } else {
      r->order[keep++] = k;
    }
  }
  r->norder = keep;
  return (int)got;
}

int take(Intake *r, bt_sha1_verdict *out, int max) {
  int n = 0;
  while (n < max && !r->done.empty()) {
    out[n++] = r->done.front().v;
    r->done.pop_front();
  }
  r->queued -= n;
  return n;
}

// Slot pointer -> outstanding slot; NULL with a message otherwise.
ISlot *locate(Intake *r, const uint8_t *p) {
  if (p >= r->h_data && p < r->h_data + r->pitch * r->nslots && (size_t)(p - r->h_data) % r->pitch == 0) {
    ISlot &s = r->slot[(size_t)(p - r->h_data) / r->pitch];
    if (s.status == kOut) return &s;
  }
  set_err("intake: pointer is not an outstanding slot");
  return nullptr;
}

// The object behind both kinds, arguments already checked; max_segs != 0: a gather intake.
bt_sha1_intake *make_intake(int device, uint32_t chunk_len, size_t pitch, uint32_t nslots, uint32_t stride,
                            uint32_t max_segs) {
  if (!ctx_for(device)) return nullptr;
  KeepDevice keep_dev;
  if (hipSetDevice(device) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", device);
    return nullptr;
  }
  auto *r = new Intake;
  r->dev = device;
  r->chunk_len = chunk_len;
  r->nslots = nslots;
  r->stride = stride ? stride : kDefaultStride;
  r->pitch = pitch;
  r->gather = max_segs != 0;
  r->max_segs = max_segs;
  const size_t nsegs = (size_t)nslots * max_segs;
  if (hipHostMalloc((void **)&r->h_data, r->pitch * nslots, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&r->h_ctl, kCtl * nslots, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&r->h_tables, sizeof(BtSha1TableEntry) * kTables * kMaxSlots, hipHostMallocDefault) !=
          hipSuccess ||
      (r->gather && (hipHostMalloc((void **)&r->h_segs, sizeof(bt_sha1_seg) * nsegs, hipHostMallocDefault) != hipSuccess ||
                     hipHostMalloc((void **)&r->h_pos, sizeof(uint64_t) * nsegs, hipHostMallocDefault) != hipSuccess))) {
    set_err("intake: allocation of %u pinned slots of %u bytes failed", nslots, chunk_len);
    bt_sha1_intake_destroy(reinterpret_cast<bt_sha1_intake *>(r));
    return nullptr;
  }
  memset(r->h_ctl, 0, kCtl * nslots);
  for (uint32_t k = 0; k < nslots; ++k) {
    r->slot[k].data = r->h_data + k * r->pitch;
    r->slot[k].ctl = r->h_ctl + k * kCtl;
    r->slot[k].restart();
  }
  return reinterpret_cast<bt_sha1_intake *>(r);
}

// What commit and commit_gather share: the slot is complete at len bytes.
void commit_slot(Intake *r, ISlot *s, uint32_t len, const uint8_t expected[20], uint64_t tag) {
  if (s->idle()) {
    memcpy(s->expected(), expected, 20);
  } else {  // line 0 of the control block belongs to the launch in flight
    memcpy(s->held, expected, 20);
    s->expected_held = true;
  }
  s->tag = tag;
  s->filled = s->len = len;
  s->status = kCommitted;
  set_due(r, *s, true);
  r->order[r->norder++] = (uint32_t)(s - r->slot);
  ++r->queued;
  ++r->stats.committed;
}

// advance / commit belong to assembled slots, append / commit_gather to datagram slots.
int wrong_kind(const Intake *r, bool want_gather, const char *call) {
  if (r->gather == want_gather) return 0;
  set_err(want_gather ? "intake: %s needs a gather intake (bt_sha1_intake_create_gather)"
                      : "intake: %s is refused on a gather intake: use append / commit_gather",
          call);
  return -1;
}

}  // namespace
}  // namespace btsha1

using namespace btsha1;

extern "C" {

bt_sha1_intake *bt_sha1_intake_create(int device, uint32_t chunk_len, uint32_t nslots, uint32_t stride) {
  if (chunk_len == 0 || chunk_len > kMaxChunk) {
    set_err("intake: chunk_len must be in [1, 32 MiB]");
    return nullptr;
  }
  if (nslots == 0 || nslots > kMaxSlots) {
    set_err("intake: nslots must be in [1, %u]", kMaxSlots);
    return nullptr;
  }
  const size_t pitch = ((size_t)chunk_len + 63) & ~(size_t)63;
  if ((uint64_t)pitch * nslots > kMaxPinned) {
    set_err("intake: %u slots of %u bytes exceed the 2 GiB of pinned memory an intake may hold", nslots, chunk_len);
    return nullptr;
  }
  return make_intake(device, chunk_len, pitch, nslots, stride, 0);
}

bt_sha1_intake *bt_sha1_dgram_slots_create(int device, uint32_t slot_len, uint32_t max_segs, uint32_t nslots,
                                           uint32_t stride) {
  if (slot_len == 0 || slot_len > kMaxGatherSlot) {
    set_err("gather intake: slot_len must be in [1, 33 MiB]");
    return nullptr;
  }
  if (max_segs == 0) {
    set_err("gather intake: max_segs must be at least 1");
    return nullptr;
  }
  if (nslots == 0 || nslots > kMaxSlots) {
    set_err("gather intake: nslots must be in [1, %u]", kMaxSlots);
    return nullptr;
  }
  const size_t pitch = ((size_t)slot_len + 15) & ~(size_t)15;
  if ((uint64_t)pitch * nslots > kMaxPinned) {
    set_err("gather intake: %u slots of %u bytes exceed the 2 GiB of pinned memory an intake may hold", nslots,
            slot_len);
    return nullptr;
  }
  if ((uint64_t)nslots * max_segs * (sizeof(bt_sha1_seg) + sizeof(uint64_t)) > kMaxSegTables) {
    set_err("gather intake: nslots x max_segs x 24 bytes of segment tables exceed 256 MiB");
    return nullptr;
  }
  return make_intake(device, slot_len, pitch, nslots, stride, max_segs);
}

void bt_sha1_intake_destroy(bt_sha1_intake *rr) {
  Intake *r = impl(rr);
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
  if (r->h_tables) (void)hipHostFree(r->h_tables);
  if (r->h_segs) (void)hipHostFree(r->h_segs);
  if (r->h_pos) (void)hipHostFree(r->h_pos);
  delete r;
}

uint8_t *bt_sha1_intake_slot(bt_sha1_intake *rr) {
  Intake *r = impl(rr);
  if (!r) {
    set_err("null pointer");
    return nullptr;
  }
  for (int pass = 0; pass < 2; ++pass) {
    for (uint32_t k = 0; k < r->nslots; ++k) {
      ISlot &s = r->slot[k];
      if (s.status != kFree) continue;
      s.restart();  // nothing of the slot is in flight: it was harvested, released or never used
      s.status = kOut;
      return s.data;
    }
    if (pass || !harvest_ready(r)) break;  // a finished chunk's slot is free again
  }
  set_err("intake: all %u slots are outstanding (commit or release one, or take its verdict)", r->nslots);
  return nullptr;
}

int bt_sha1_intake_advance(bt_sha1_intake *rr, uint8_t *slot, uint32_t filled) {
  Intake *r = impl(rr);
  if (!r || !slot) {
    set_err("null pointer");
    return -1;
  }
  if (wrong_kind(r, false, "advance")) return -1;
  ISlot *s = locate(r, slot);
  if (!s) return -1;
  if (filled < s->filled || filled > r->chunk_len) {
    set_err("intake: filled = %u must not decrease (was %u) or exceed chunk_len %u", filled, s->filled, r->chunk_len);
    return -1;
  }
  s->filled = filled;
  const uint32_t whole = filled & ~63u;
  if (whole > s->hashed && whole - s->hashed >= r->stride) set_due(r, *s, true);
  return 0;
}

int bt_sha1_intake_commit(bt_sha1_intake *rr, uint8_t *slot, uint32_t len, const uint8_t expected[20], uint64_t tag) {
  Intake *r = impl(rr);
  if (!r || !slot || !expected) {
    set_err("null pointer");
    return -1;
  }
  if (wrong_kind(r, false, "commit")) return -1;
  ISlot *s = locate(r, slot);
  if (!s) return -1;
  if (len == 0 || len < s->hashed || len > r->chunk_len) {
    set_err("intake: commit of %u bytes: must be in [max(1, %u already hashed), chunk_len %u]", len, s->hashed,
            r->chunk_len);
    return -1;
  }
  commit_slot(r, s, len, expected, tag);
  return 0;
}

int bt_sha1_dgram_slots_append(bt_sha1_intake *rr, uint8_t *slot, const bt_sha1_seg *segs, uint32_t nseg) {
  Intake *r = impl(rr);
  if (!r || !slot || (!segs && nseg)) {
    set_err("null pointer");
    return -1;
  }
  if (wrong_kind(r, true, "append")) return -1;
  ISlot *s = locate(r, slot);
  if (!s) return -1;
  // Everything is checked before anything is recorded.
  if (nseg > r->max_segs - s->nseg) {
    set_err("gather intake: %u more segments after %u exceed max_segs %u", nseg, s->nseg, r->max_segs);
    return -1;
  }
  uint64_t total = s->filled;
  for (uint32_t k = 0; k < nseg; ++k) {
    if (segs[k].off > r->chunk_len || segs[k].len > r->chunk_len - segs[k].off) {
      set_err("gather intake: segment %u (off %llu, len %u) reaches past slot_len %u", k,
              (unsigned long long)segs[k].off, segs[k].len, r->chunk_len);
      return -1;
    }
    total += segs[k].len;
    if (total > kMaxChunk) {
      set_err("gather intake: the listed segments exceed 32 MiB");
      return -1;
    }
  }
  // Descriptors and positions at and past the slot's nseg: a launch in flight
  // on the slot reads only those below the nseg of its kick.
  bt_sha1_seg *d = r->segs(*s) + s->nseg;
  uint64_t *pos = r->pos(*s) + s->nseg;
  uint64_t at = s->filled;
  for (uint32_t k = 0; k < nseg; ++k) {
    d[k].off = segs[k].off;
    d[k].len = segs[k].len;
    d[k].reserved = 0;
    pos[k] = at;
    at += segs[k].len;
  }
  s->nseg += nseg;
  s->filled = (uint32_t)total;
  const uint32_t whole = s->filled & ~63u;
  if (whole > s->hashed && whole - s->hashed >= r->stride) set_due(r, *s, true);
  return 0;
}

int bt_sha1_dgram_slots_commit(bt_sha1_intake *rr, uint8_t *slot, const uint8_t expected[20], uint64_t tag) {
  Intake *r = impl(rr);
  if (!r || !slot || !expected) {
    set_err("null pointer");
    return -1;
  }
  if (wrong_kind(r, true, "commit_gather")) return -1;
  ISlot *s = locate(r, slot);
  if (!s) return -1;
  if (s->filled == 0) {
    set_err("gather intake: commit of a slot with no bytes listed");
    return -1;
  }
  commit_slot(r, s, s->filled, expected, tag);
  return 0;
}

int bt_sha1_intake_release(bt_sha1_intake *rr, uint8_t *slot) {
  Intake *r = impl(rr);
  if (!r || !slot) {
    set_err("null pointer");
    return -1;
  }
  ISlot *s = locate(r, slot);
  if (!s) return -1;
  if (!s->idle()) {  // an advance is in flight on the slot: it is handed out again only after it
    KeepDevice keep_dev;
    if (set_device(r) || wait_slot(r, *s)) return -1;
  }
  set_due(r, *s, false);  // a span that was due but never launched is dropped
  s->restart();
  s->status = kFree;
  ++r->stats.released;
  return 0;
}

int bt_sha1_intake_kick(bt_sha1_intake *rr) {
  Intake *r = impl(rr);
  if (!r) {
    set_err("null pointer");
    return -1;
  }
  return kick(r);
}

int bt_sha1_intake_sync(bt_sha1_intake *rr) {
  Intake *r = impl(rr);
  if (!r) {
    set_err("null pointer");
    return -1;
  }
  return sync_all(r);
}

int bt_sha1_intake_poll(bt_sha1_intake *rr, bt_sha1_verdict *out, int max) {
  Intake *r = impl(rr);
  if (!r || (!out && max > 0)) {
    set_err("null pointer");
    return -1;
  }
  const int got = harvest_ready(r);
  if (kick(r) < 0) return -1;
  if (got || r->norder == 0 || !r->done.empty()) {
    r->empty_polls = 0;
    return take(r, out, max);
  }
  // Nothing finished.  Every 64th such poll in a row looks at the oldest
  // launch's stream (a query, not a wait), so a failed launch surfaces here too.
  if ((++r->empty_polls & 63u) == 0 && r->tail < r->head) {
    const hipError_t q = hipStreamQuery(r->flight[r->tail % kTables].st);
    if (q == hipSuccess && !launch_finished(r, r->tail)) {
      set_err("intake: resume kernel finished without its completion word");
      return -1;
    }
    if (q != hipSuccess && q != hipErrorNotReady) {
      set_err("intake: resume kernel: %s", hipGetErrorString(q));
      return -1;
    }
    retire(r);
  }
  return 0;
}

int bt_sha1_intake_drain(bt_sha1_intake *rr, bt_sha1_verdict *out, int max) {
  Intake *r = impl(rr);
  if (!r || (!out && max > 0)) {
    set_err("null pointer");
    return -1;
  }
  // After a sync every slot is idle, so the next kick takes every committed
  // slot: two rounds at the most (an advance in flight, then the finish).
  for (int round = 0; r->norder; ++round) {
    harvest_ready(r);
    if (r->norder == 0) break;
    if (round == 3) {
      set_err("intake: committed chunks did not finish");
      return -1;
    }
    if (kick(r) < 0 || sync_all(r)) return -1;
  }
  return take(r, out, max);
}

int64_t bt_sha1_intake_pending(bt_sha1_intake *r) {
  if (!r) {
    set_err("null pointer");
    return -1;
  }
  return impl(r)->queued;
}

int bt_sha1_intake_get_stats(bt_sha1_intake *r, bt_sha1_intake_stats *out) {
  if (!r || !out) {
    set_err("null pointer");
    return -1;
  }
  *out = impl(r)->stats;
  return 0;
}

}  // extern "C"
