// bt_verifier.cpp -- the batched asynchronous verifier (bt_sha1_verifier_*,
// include/bt_sha1.h).
//
// Reference interface replaced (yunfanye/Bittorrent-with-Congestion-Control):
//   hash + memcmp of save_chunk    util.c:304-337, without the synchronous hash
//
// A ring of `nstreams` batches of `batch` pinned chunk slots.  Slots are handed
// out in ring order and may be committed (or released) in any order -- a peer
// assembles up to max_conn chunks at once (util.c:250-277).  A batch launches
// (one H2D of its slots, one hot-kernel launch with the fused verify epilogue)
// once it is closed -- every slot handed out, or flushed -- and each of its
// handed-out slots has been committed or released.
//
// A ragged verifier (bt_sha1_verifier_create_ragged) takes chunks of any
// length up to max_chunk_len -- a file's short last chunk, the last fread of
// make_chunks (chunk.c:20).  Its slots lie at a pitch of max_chunk_len rounded
// up to 16 bytes.  A batch whose committed slots are all max_chunk_len long,
// with max_chunk_len a 16-byte multiple, launches exactly what a classic
// verifier launches; any other batch is copied the same way and hashed by ONE
// btsha1_launch_ragged_verify over (i * pitch, length i), both read by the
// kernel in place from per-batch pinned arrays, released slots with length 0.
//
// A gather verifier (bt_sha1_verifier_create_gather) holds DATAGRAMS in its
// slots: packets stay where recvfrom put them, header and payload, in arrival
// order, and commit_gather lists the payloads in sequence order.  Every batch
// is one copy of its slots as they are and ONE btsha1_launch_gather over the
// batch's pinned segment table; slot i's segments stand at i * max_segs, so
// commits in any order need no compaction.  Released slots have count 0.
#include "bt_columns.h"
#include "bt_runtime.h"

#include <deque>
#include <vector>

using namespace btsha1;

struct VBatch {
  hipStream_t s = nullptr;
  hipEvent_t ev = nullptr;
  // column-split batches (v_launch): the columns' hashes run on hs, each after
  // its copy's event on s; the chunks' chaining state between columns
  hipStream_t hs = nullptr;
  hipEvent_t cev[kMaxColumns] = {};
  uint32_t *d_state = nullptr;
  StageBuf slots;  // the received chunks: written by the caller, read by the H2D copy
  uint8_t *h_in = nullptr, *h_exp = nullptr, *h_ok = nullptr, *h_dig = nullptr;
  // ragged verifiers only (pinned, read by the kernel in place): slot i's offset i * pitch and its
  // committed length (0: released, or not handed out)
  uint64_t *h_off = nullptr;
  uint32_t *h_len = nullptr;
  // gather verifiers only (pinned, read by the kernel in place): slot i's segments at h_segs[i * max_segs ..]
  // with offsets from d_in, h_first[i] = i * max_segs, and their count (0: released, or not handed out)
  bt_sha1_seg *h_segs = nullptr;
  uint64_t *h_first = nullptr;
  uint32_t *h_count = nullptr;
  uint8_t *d_in = nullptr;
  std::vector<uint64_t> tags;
  std::vector<uint8_t> state;  // per slot: 0 free, 1 handed out, 2 committed, 3 released
  uint32_t reserved = 0, settled = 0;
  bool closed = false, inflight = false;
};

struct bt_sha1_verifier {
  int dev = 0;
  uint32_t chunk_len = 0, batch = 0;  // chunk_len: every chunk's length, or a ragged verifier's max_chunk_len
  uint32_t pitch = 0;                 // slot i of a batch at i * pitch: chunk_len, rounded up to 16 bytes when ragged
  bool ragged = false;
  bool gather = false;    // chunk_len is then the slot length
  uint32_t max_segs = 0;  // gather: segments per chunk at most
  bt_sha1_verifier_stats st = {};
  bt_sha1_verifier_gather_stats gs = {};
  std::vector<VBatch> b;
  uint32_t fill = 0;             // batch handing out slots
  std::deque<uint32_t> order;    // batches in flight, oldest first
  std::deque<bt_sha1_verdict> done;
  int64_t queued = 0;            // committed, verdict not yet returned
};

namespace {

int v_harvest(bt_sha1_verifier *v, VBatch &b) {
  BT_CK(hipEventSynchronize(b.ev));
  for (uint32_t i = 0; i < b.reserved; ++i) {
    if (b.state[i] != 2) continue;  // released slots produce no verdict
    bt_sha1_verdict r;
    r.tag = b.tags[i];
    r.ok = b.h_ok[i] ? 1 : 0;
    memcpy(r.digest, b.h_dig + 20 * i, 20);
    v->done.push_back(r);
  }
  std::fill(b.state.begin(), b.state.end(), 0);
  b.reserved = b.settled = 0;
  b.closed = b.inflight = false;
  return 0;
}

// Columns a batch of `rows` chunks is split into (0: one copy, one launch):
// as the host pipelines' tail (HostFeed), a batch of at least
// column_min_bytes() of chunks of at least 64 KiB is copied in columns and
// each column hashed as soon as it has arrived, so its verdicts come one
// column's hash (~0.9 ms), not one whole chunk's (~6.7 ms), after its last
// byte crossed PCIe.
uint32_t v_columns(uint64_t chunk_len, uint64_t rows) {
  const uint32_t parts = split_columns(chunk_len);
  return parts && rows >= 2 && rows * chunk_len >= column_min_bytes() ? parts : 0;
}

int v_launch_columns(bt_sha1_verifier *v, VBatch &b, uint32_t parts) {
  const uint64_t cl = v->chunk_len, rows = b.reserved, w = cl / parts;
  if (!b.hs) BT_CK(hipStreamCreateWithFlags(&b.hs, hipStreamNonBlocking));
  if (!b.d_state) BT_CK(hipMalloc((void **)&b.d_state, 20 * (size_t)v->batch));
  const ColumnRun run{b.s, b.hs, b.cev, parts, rows, w, cl, b.d_in, b.d_state};
  for (uint32_t j = 0; j < parts; ++j) {
    BT_CK(hipMemcpy2DAsync(b.d_in + j * rows * w, (size_t)w, b.h_in + j * w, (size_t)cl, (size_t)w, (size_t)rows,
                           hipMemcpyHostToDevice, b.s));
    const bool last = j + 1 == parts;
    if (hash_column(run, j, last ? b.h_dig : nullptr, last ? b.h_exp : nullptr, last ? b.h_ok : nullptr)) return -1;
  }
  BT_CK(hipEventRecord(b.ev, b.hs));
  return 0;
}

// A ragged verifier's batch that needs the ragged launch: a committed slot
// shorter than max_chunk_len, or slots that are not at a pitch of chunk_len.
bool v_needs_ragged(const bt_sha1_verifier *v, const VBatch &b) {
  if (!v->ragged) return false;
  if (v->pitch != v->chunk_len) return true;
  for (uint32_t i = 0; i < b.reserved; ++i)
    if (b.state[i] == 2 && b.h_len[i] != v->chunk_len) return true;
  return false;
}

int v_launch(bt_sha1_verifier *v, uint32_t idx) {
  VBatch &b = v->b[idx];
  if (b.reserved == 0) {  // closed while empty: nothing to do
    b.closed = false;
    return 0;
  }
  ++v->st.batches;
  if (v->gather) {  // the slots as they are, one launch over the segment table
    const size_t bytes = (size_t)b.reserved * v->pitch;
    ++v->gs.gather_batches;
    v->gs.copied_bytes += bytes;
    BT_CK(hipMemcpyAsync(b.d_in, b.h_in, bytes, hipMemcpyHostToDevice, b.s));
    BT_CK(btsha1_launch_gather(b.d_in, b.h_segs, b.h_first, b.h_count, b.reserved, b.h_dig, b.h_exp, b.h_ok, b.s));
    BT_CK(hipEventRecord(b.ev, b.s));
    b.inflight = true;
    v->order.push_back(idx);
    return 0;
  }
  if (v_needs_ragged(v, b)) {  // one copy, one launch, no column split
    ++v->st.ragged_batches;
    BT_CK(hipMemcpyAsync(b.d_in, b.h_in, (size_t)b.reserved * v->pitch, hipMemcpyHostToDevice, b.s));
    BT_CK(btsha1_launch_ragged_verify(b.d_in, b.h_off, b.h_len, 0, 0, b.reserved, b.h_dig, b.h_exp, b.h_ok, b.s));
    BT_CK(hipEventRecord(b.ev, b.s));
    b.inflight = true;
    v->order.push_back(idx);
    return 0;
  }
  if (const uint32_t parts = v_columns(v->chunk_len, b.reserved)) {
    if (v_launch_columns(v, b, parts)) {  // leave nothing of the batch in flight behind the error
      if (b.s) (void)hipStreamSynchronize(b.s);
      if (b.hs) (void)hipStreamSynchronize(b.hs);
      return -1;
    }
    b.inflight = true;
    v->order.push_back(idx);
    return 0;
  }
  const size_t bytes = (size_t)b.reserved * v->chunk_len;
  BT_CK(hipMemcpyAsync(b.d_in, b.h_in, bytes, hipMemcpyHostToDevice, b.s));
  // Expected hashes are read, verdicts and digests written, by the kernel in
  // pinned host memory: the chunk bytes are the only copy (see run_pipeline).
  BT_CK(btsha1_launch_fixed(b.d_in, b.reserved, v->chunk_len, v->chunk_len, b.h_dig, b.h_exp, b.h_ok, b.s,
                            g_variant.load()));
  BT_CK(hipEventRecord(b.ev, b.s));
  b.inflight = true;
  v->order.push_back(idx);
  return 0;
}

int v_maybe_launch(bt_sha1_verifier *v, uint32_t idx) {
  VBatch &b = v->b[idx];
  if (b.closed && !b.inflight && b.settled == b.reserved) return v_launch(v, idx);
  return 0;
}

// The filling batch is closed: move the fill pointer on, waiting for the next
// batch of the ring if it is still in flight.
int v_advance(bt_sha1_verifier *v) {
  const uint32_t nxt = (v->fill + 1) % (uint32_t)v->b.size();
  VBatch &n = v->b[nxt];
  if (n.inflight) {  // ring wrapped: harvest up to and including it
    while (!v->order.empty()) {
      const uint32_t o = v->order.front();
      v->order.pop_front();
      if (v_harvest(v, v->b[o])) return -1;
      if (o == nxt) break;
    }
  } else if (n.closed) {
    set_err("verifier: every batch holds slots that were handed out but never committed");
    return -1;
  }
  v->fill = nxt;
  return 0;
}

// Slot pointer -> (batch, index); -1 if it is not a handed-out slot.
int v_locate(bt_sha1_verifier *v, const uint8_t *slot, uint32_t *bi, uint32_t *si) {
  for (uint32_t k = 0; k < v->b.size(); ++k) {
    VBatch &b = v->b[k];
    if (slot >= b.h_in && slot < b.h_in + (size_t)v->batch * v->pitch) {
      const size_t off = (size_t)(slot - b.h_in);
      if (off % v->pitch || b.state[off / v->pitch] != 1) break;
      *bi = k;
      *si = (uint32_t)(off / v->pitch);
      return 0;
    }
  }
  set_err("verifier: pointer is not an outstanding slot");
  return -1;
}

// The chunk length a commit or a submit brings: exactly chunk_len, or for a
// ragged verifier anything from 1 to max_chunk_len.
int v_check_len(const bt_sha1_verifier *v, uint32_t len) {
  if (v->gather) {
    if (len == 0 || len > v->chunk_len) {
      set_err("verifier: chunk of %u bytes, gather verifier's slots take 1 .. %u", len, v->chunk_len);
      return -1;
    }
  } else if (v->ragged) {
    if (len == 0 || len > v->chunk_len) {
      set_err("verifier: chunk of %u bytes, ragged verifier takes 1 .. %u", len, v->chunk_len);
      return -1;
    }
  } else if (len != v->chunk_len) {
    set_err("verifier: chunk of %u bytes, verifier built for %u", len, v->chunk_len);
    return -1;
  }
  return 0;
}

bt_sha1_verifier *v_create(int device, uint32_t chunk_len, uint32_t batch, uint32_t nstreams, bool ragged,
                           uint32_t max_segs = 0) {
  const bool gather = max_segs != 0;
  DevCtx *c = ctx_for(device);
  if (!c) return nullptr;
  KeepDevice keep_dev;
  if (hipSetDevice(device) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", device);
    return nullptr;
  }
  // The receive slots are written by the caller's receive path and read by
  // the DMA engine: on the GPU's NUMA node, like the pipelines' lanes.
  int node = -1;
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (c->numa_node == -2) c->numa_node = gpu_numa_node(device);
    node = placement_for(c->numa_node).node;
  }
  auto *v = new bt_sha1_verifier;
  v->dev = device;
  v->chunk_len = chunk_len;
  v->pitch = ragged || gather ? (chunk_len + 15u) & ~15u : chunk_len;
  v->ragged = ragged;
  v->gather = gather;
  v->max_segs = max_segs;
  v->batch = batch;
  v->b.resize(std::max<uint32_t>(nstreams, 2));
  const size_t bytes = (size_t)batch * v->pitch;
  t_err.clear();
  for (auto &b : v->b) {
    b.tags.resize(batch);
    b.state.assign(batch, 0);
    if (hipStreamCreateWithFlags(&b.s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess ||
        b.slots.ensure(bytes, node) != 0 ||
        hipHostMalloc((void **)&b.h_exp, 20 * (size_t)batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&b.h_ok, batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&b.h_dig, 20 * (size_t)batch, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&b.d_in, bytes) != hipSuccess ||
        (ragged && (hipHostMalloc((void **)&b.h_off, 8 * (size_t)batch, hipHostMallocDefault) != hipSuccess ||
                    hipHostMalloc((void **)&b.h_len, 4 * (size_t)batch, hipHostMallocDefault) != hipSuccess)) ||
        (gather &&
         (hipHostMalloc((void **)&b.h_segs, sizeof(bt_sha1_seg) * (size_t)batch * max_segs, hipHostMallocDefault) !=
              hipSuccess ||
          hipHostMalloc((void **)&b.h_first, 8 * (size_t)batch, hipHostMallocDefault) != hipSuccess ||
          hipHostMalloc((void **)&b.h_count, 4 * (size_t)batch, hipHostMallocDefault) != hipSuccess))) {
      if (t_err.empty()) set_err("verifier: allocation failed");
      bt_sha1_verifier_destroy(v);
      return nullptr;
    }
    b.h_in = b.slots.as<uint8_t>();
    for (uint32_t i = 0; ragged && i < batch; ++i) {
      b.h_off[i] = (uint64_t)i * v->pitch;
      b.h_len[i] = 0;
    }
    for (uint32_t i = 0; gather && i < batch; ++i) {
      b.h_first[i] = (uint64_t)i * max_segs;
      b.h_count[i] = 0;
    }
  }
  return v;
}

}  // namespace

extern "C" {

bt_sha1_verifier *bt_sha1_verifier_create(int device, uint32_t chunk_len, uint32_t batch, uint32_t nstreams) {
  if (chunk_len == 0 || (chunk_len & 15) || chunk_len > (32u << 20) || batch == 0) {
    set_err("verifier: chunk_len must be a 16-byte multiple <= 32 MiB and batch > 0");
    return nullptr;
  }
  return v_create(device, chunk_len, batch, nstreams, false);
}

bt_sha1_verifier *bt_sha1_verifier_create_ragged(int device, uint32_t max_chunk_len, uint32_t batch,
                                                 uint32_t nstreams) {
  if (max_chunk_len == 0 || max_chunk_len > (32u << 20) || batch == 0) {
    set_err("verifier: max_chunk_len must be in [1, 32 MiB] and batch > 0");
    return nullptr;
  }
  return v_create(device, max_chunk_len, batch, nstreams, true);
}

bt_sha1_verifier *bt_sha1_verifier_create_gather(int device, uint32_t slot_len, uint32_t max_segs, uint32_t batch,
                                                 uint32_t nstreams) {
  if (slot_len == 0 || slot_len > (33u << 20) || max_segs == 0 || batch == 0 ||
      (uint64_t)batch * max_segs * sizeof(bt_sha1_seg) > (256ull << 20)) {
    set_err("verifier: slot_len must be in [1, 33 MiB], max_segs > 0, batch > 0 and batch x max_segs x 16 <= 256 MiB");
    return nullptr;
  }
  return v_create(device, slot_len, batch, nstreams, false, max_segs);
}

int bt_sha1_verifier_commit_gather(bt_sha1_verifier *v, uint8_t *slot, const bt_sha1_seg *segs, uint32_t nseg,
                                   const uint8_t expected[20], uint64_t tag) {
  if (!v || !slot || !expected || (nseg && !segs)) {
    set_err("null pointer");
    return -1;
  }
  if (!v->gather) {
    set_err("verifier: commit_gather needs a verifier from bt_sha1_verifier_create_gather");
    return -1;
  }
  if (nseg > v->max_segs) {
    set_err("verifier: %u segments, gather verifier built for %u per chunk", nseg, v->max_segs);
    return -1;
  }
  uint64_t payload = 0;
  for (uint32_t k = 0; k < nseg; ++k) {
    if (segs[k].off > v->chunk_len || segs[k].len > v->chunk_len - segs[k].off) {
      set_err("verifier: segment %u (offset %llu, %u bytes) ends past the slot's %u bytes", k,
              (unsigned long long)segs[k].off, segs[k].len, v->chunk_len);
      return -1;
    }
    payload += segs[k].len;
  }
  KeepDevice keep_dev;
  if (hipSetDevice(v->dev) != hipSuccess) return -1;
  uint32_t bi, si;
  if (v_locate(v, slot, &bi, &si)) return -1;
  VBatch &b = v->b[bi];
  memcpy(b.h_exp + 20 * (size_t)si, expected, 20);
  bt_sha1_seg *t = b.h_segs + (size_t)si * v->max_segs;
  for (uint32_t k = 0; k < nseg; ++k) t[k] = bt_sha1_seg{(uint64_t)si * v->pitch + segs[k].off, segs[k].len, 0};
  b.h_count[si] = nseg;
  ++v->gs.gather_chunks;
  v->gs.segments += nseg;
  v->gs.payload_bytes += payload;
  ++v->st.chunks;
  b.tags[si] = tag;
  b.state[si] = 2;
  ++b.settled;
  ++v->queued;
  return v_maybe_launch(v, bi);
}

int bt_sha1_verifier_get_gather_stats(bt_sha1_verifier *v, bt_sha1_verifier_gather_stats *out) {
  if (!v || !out) {
    set_err("null pointer");
    return -1;
  }
  *out = v->gs;
  return 0;
}

void bt_sha1_verifier_destroy(bt_sha1_verifier *v) {
  if (!v) return;
  KeepDevice keep_dev;
  (void)hipSetDevice(v->dev);
  for (auto &b : v->b) {
    if (b.s) (void)hipStreamSynchronize(b.s);
    if (b.hs) (void)hipStreamSynchronize(b.hs);
    if (b.ev) (void)hipEventDestroy(b.ev);
    for (hipEvent_t e : b.cev)
      if (e) (void)hipEventDestroy(e);
    if (b.s) (void)hipStreamDestroy(b.s);
    if (b.hs) (void)hipStreamDestroy(b.hs);
    if (b.d_state) (void)hipFree(b.d_state);
    b.slots.release();
    if (b.h_exp) (void)hipHostFree(b.h_exp);
    if (b.h_ok) (void)hipHostFree(b.h_ok);
    if (b.h_dig) (void)hipHostFree(b.h_dig);
    if (b.h_off) (void)hipHostFree(b.h_off);
    if (b.h_len) (void)hipHostFree(b.h_len);
    if (b.h_segs) (void)hipHostFree(b.h_segs);
    if (b.h_first) (void)hipHostFree(b.h_first);
    if (b.h_count) (void)hipHostFree(b.h_count);
    if (b.d_in) (void)hipFree(b.d_in);
  }
  delete v;
}

uint8_t *bt_sha1_verifier_slot(bt_sha1_verifier *v) {
  if (!v) return nullptr;
  KeepDevice keep_dev;
  if (hipSetDevice(v->dev) != hipSuccess) return nullptr;
  if (v->b[v->fill].closed && v_advance(v)) return nullptr;
  VBatch &b = v->b[v->fill];
  const uint32_t j = b.reserved++;
  b.state[j] = 1;
  if (b.reserved == v->batch) b.closed = true;  // launches when its last slot settles
  return b.h_in + (size_t)j * v->pitch;
}

int bt_sha1_verifier_commit(bt_sha1_verifier *v, uint8_t *slot, uint32_t len, const uint8_t expected[20],
                            uint64_t tag) {
  if (!v || !slot || !expected) {
    set_err("null pointer");
    return -1;
  }
  if (v_check_len(v, len)) return -1;
  KeepDevice keep_dev;
  if (hipSetDevice(v->dev) != hipSuccess) return -1;
  uint32_t bi, si;
  if (v_locate(v, slot, &bi, &si)) return -1;
  VBatch &b = v->b[bi];
  memcpy(b.h_exp + 20 * (size_t)si, expected, 20);
  if (v->ragged) b.h_len[si] = len;
  if (v->gather) {  // the one-segment message (0, len)
    b.h_segs[(size_t)si * v->max_segs] = bt_sha1_seg{(uint64_t)si * v->pitch, len, 0};
    b.h_count[si] = 1;
    ++v->gs.gather_chunks;
    ++v->gs.segments;
    v->gs.payload_bytes += len;
  }
  ++v->st.chunks;
  if (!v->gather && len < v->chunk_len) ++v->st.short_chunks;
  b.tags[si] = tag;
  b.state[si] = 2;
  ++b.settled;
  ++v->queued;
  return v_maybe_launch(v, bi);
}

int bt_sha1_verifier_release(bt_sha1_verifier *v, uint8_t *slot) {
  if (!v || !slot) {
    set_err("null pointer");
    return -1;
  }
  KeepDevice keep_dev;
  if (hipSetDevice(v->dev) != hipSuccess) return -1;
  uint32_t bi, si;
  if (v_locate(v, slot, &bi, &si)) return -1;
  VBatch &b = v->b[bi];
  memset(b.h_exp + 20 * (size_t)si, 0, 20);
  if (v->ragged) b.h_len[si] = 0;  // hashed as an empty message; no verdict (v_harvest)
  if (v->gather) b.h_count[si] = 0;
  ++v->st.released;
  b.state[si] = 3;
  ++b.settled;
  return v_maybe_launch(v, bi);
}

int bt_sha1_verifier_submit(bt_sha1_verifier *v, const void *h_chunk, uint32_t len, const uint8_t expected[20],
                            uint64_t tag) {
  if (!v || !h_chunk) {
    set_err("null pointer");
    return -1;
  }
  if (v_check_len(v, len)) return -1;
  uint8_t *slot = bt_sha1_verifier_slot(v);
  if (!slot) return -1;
  memcpy(slot, h_chunk, len);
  return bt_sha1_verifier_commit(v, slot, len, expected, tag);
}

int bt_sha1_verifier_flush(bt_sha1_verifier *v) {
  if (!v) return -1;
  KeepDevice keep_dev;
  if (hipSetDevice(v->dev) != hipSuccess) return -1;
  VBatch &b = v->b[v->fill];
  if (b.reserved == 0 || b.closed) return 0;
  b.closed = true;
  return v_maybe_launch(v, v->fill);
}

static int v_take(bt_sha1_verifier *v, bt_sha1_verdict *out, int max) {
  int n = 0;
  while (n < max && !v->done.empty()) {
    out[n++] = v->done.front();
    v->done.pop_front();
  }
  v->queued -= n;
  return n;
}

int bt_sha1_verifier_poll(bt_sha1_verifier *v, bt_sha1_verdict *out, int max) {
  if (!v) return -1;
  KeepDevice keep_dev;
  if (hipSetDevice(v->dev) != hipSuccess) return -1;
  while (!v->order.empty()) {
    VBatch &b = v->b[v->order.front()];
    hipError_t q = hipEventQuery(b.ev);
    if (q == hipErrorNotReady) break;
    if (q != hipSuccess) {
      set_err("verifier: %s", hipGetErrorString(q));
      return -1;
    }
    v->order.pop_front();
    if (v_harvest(v, b)) return -1;
  }
  return v_take(v, out, max);
}

int bt_sha1_verifier_drain(bt_sha1_verifier *v, bt_sha1_verdict *out, int max) {
  if (!v) return -1;
  if (bt_sha1_verifier_flush(v)) return -1;
  while (!v->order.empty()) {
    const uint32_t o = v->order.front();
    v->order.pop_front();
    if (v_harvest(v, v->b[o])) return -1;
  }
  return v_take(v, out, max);
}

int64_t bt_sha1_verifier_pending(bt_sha1_verifier *v) { return v ? v->queued : -1; }

int bt_sha1_verifier_get_stats(bt_sha1_verifier *v, bt_sha1_verifier_stats *out) {
  if (!v || !out) {
    set_err("null pointer");
    return -1;
  }
  *out = v->st;
  return 0;
}

}  // extern "C"
