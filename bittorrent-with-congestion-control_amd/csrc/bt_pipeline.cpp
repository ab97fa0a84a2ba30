// bt_pipeline.cpp -- the host pipelines: an image in host memory or a file
// goes through two double-buffered staging lanes to the hot kernel, digests
// come back in chunk order.  Three feeds (staged, direct DMA from pinned
// memory, pageable memory page-locked batch by batch), the column-split last
// batch, and the split of one image over several devices.
//
// Reference interface replaced (yunfanye/Bittorrent-with-Congestion-Control):
//   make_chunks' read + hash loop  chunk.c:13-25 (chunk.h:25), a chunk at a
//   time on one core there; bt_sha1_chunks_host* / bt_sha1_chunks_file here.
//
// Host-side work here is bookkeeping only (staging, page locking); every
// compression runs in a HIP kernel.  No CPU hashing path.
#include "bt_columns.h"
#include "bt_runtime.h"

#include <memory>
#include <thread>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>
#include <cerrno>

namespace btsha1 {

namespace {

// Staging batch: ~1 GiB per lane keeps >= 2048 chunks in flight per launch,
// enough that the per-chunk hash latency (~10 ms, 8193 dependent blocks at one
// wave per SIMD) still outruns PCIe; capped by the input size when known.  An
// input of 64 MiB - 2 GiB is cut in two batches so both lanes work (the second
// lane's pinning overlaps the first batch, see run_pipeline).
// Direct-DMA input (pinned / registered) uses the same 1 GiB batches, DMA'd
// straight from the caller's memory into the kept lanes.  Round 2 chose 4 GiB
// batches under overlapping copies (40.2 / 45.9 / 48.9 GiB/s with 1 / 2 / 4
// GiB); with round 3's serial copy order bigger batches gain nothing, and
// because they exceed the kept lanes they were allocated and freed on every
// call -- and a re-allocated 4 GiB batch ran the copies at 41.1-41.4 GiB/s call
// after call on three of three boxes (tools/dma_repeat.py;
// profiles/r04/dma_batch.md) where 1 GiB kept lanes hold 48.9-50.7 (8 GiB
// image) and 52.4-52.5 (32 GiB) against a ~53.6 raw copy.  BT_SHA1_DMA_BATCH_MB overrides the 1024 MiB
// default; batches above 1 GiB are freed after the call.
uint64_t dma_batch_target() {
  static const uint64_t v = [] {
    const char *e = getenv("BT_SHA1_DMA_BATCH_MB");
    const long mb = e ? atol(e) : 1024;
    return (uint64_t)(mb < 64 ? 64 : (mb > 16384 ? 16384 : mb)) << 20;
  }();
  return v;
}

uint64_t batch_bytes_for(uint64_t chunk_len, uint64_t size_hint, bool staged = true) {
  const uint64_t target = staged ? 1ull << 30 : dma_batch_target();
  uint64_t per = std::max<uint64_t>(1, target / chunk_len);
  if (size_hint != UINT64_MAX) {
    const uint64_t n = (size_hint + chunk_len - 1) / chunk_len;
    per = std::max<uint64_t>(1, std::min<uint64_t>(per, size_hint >= (64ull << 20) ? (n + 1) / 2 : n));
  }
  return per * chunk_len;
}

// Host memory the DMA engine can read directly (hipHostMalloc'd or
// registered with bt_sha1_host_register): no staging copy needed.
bool is_pinned(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
// An input is DMA'd in place only when both its ends are pinned (a lock
// around its first bytes alone -- a neighbour's page -- does not make it so).
bool is_pinned_range(const uint8_t *p, uint64_t n) { return n && is_pinned(p) && is_pinned(p + n - 1); }

// Workers of one bt_sha1_chunks_host_devices call (each a host thread with two
// staging lanes of up to 1 GiB pinned + 1 GiB HBM while the call runs).
constexpr int kMaxWorkers = 64;

// Staging -> H2D granule inside a batch: 128 MiB (BT_SHA1_PIECE_MB overrides,
// 16 .. 1024).
uint64_t piece_bytes() {
  static const uint64_t v = [] {
    const char *e = getenv("BT_SHA1_PIECE_MB");
    const long mb = e ? atol(e) : 128;
    return (uint64_t)(mb < 16 ? 16 : (mb > 1024 ? 1024 : mb)) << 20;
  }();
  return v;
}

// Copy order of the two lanes.  "serial": a batch's first H2D waits for the
// previous batch's last one, so one copy runs at a time (hashing still
// overlaps the next copy).  "overlap": a batch's H2D may run beside the
// previous batch's (two DMA engines at once).  Default: serial for direct DMA
// from pinned / registered memory, overlap for the staged lanes.  Measured
// (tools/numa_probe.py 8, profiles/r03/numa_probe.md): an 8 GiB registered
// image on the GPU's socket 50.6 (overlap) / 50.1 (serial) GiB/s, on the other
// socket 42.2 (overlap) / 49.7 (serial) -- two concurrent DMA streams out of
// the other socket's memory lose ~8 GiB/s; the staged lanes (whose pages the
// copy threads place) lose ~1 with serial copies.  BT_SHA1_COPY_ORDER=
// serial|overlap forces one order.
bool serial_copies(bool staged) {
  static const int forced = [] {
    const char *e = getenv("BT_SHA1_COPY_ORDER");
    return e ? (!strcmp(e, "serial") ? 1 : !strcmp(e, "overlap") ? 0 : -1) : -1;
  }();
  return forced >= 0 ? forced == 1 : !staged;
}

// bt_sha1_get_pipeline_stats: the calling thread's last pipeline run.
thread_local bt_sha1_pipeline_stats t_stats;
thread_local bool t_stats_valid = false;

// How a pipeline's input reaches the DMA engine.
enum class Feed {
  kStaged,     // copied (memcpy / pread) into the pinned staging lanes
  kDirect,     // the caller's memory is pinned already: DMA'd in place
  kRegistered  // pageable caller memory page-locked batch by batch (HostFeed)
};

// tail.queue(idle_lane, last_copied): called once every batch is queued, with
// the lane that is not carrying the last batch and the event after the last
// batch's copy (NULL when copies may overlap) -- HostFeed's column-split
// tail; tail.wait() after the lanes are drained, before any lane buffer is
// resized.  Both return 0 or -1.
template <class Q, class W>
struct TailOps {
  Q queue;
  W wait;
};
template <class Q, class W>
TailOps<Q, W> tail_ops(Q q, W w) {
  return TailOps<Q, W>{q, w};
}
inline auto no_tail() {
  return tail_ops([](Lane &, hipEvent_t) { return 0; }, [] { return 0; });
}

// Generic double-buffered pipeline over two streams: batch k+1's H2D overlaps
// batch k's hashing, and inside a batch each 128 MiB piece is copied to the
// device as soon as it is staged, so host reads overlap the H2D.
// fill(lane, off, max_bytes, &src, &eof) provides up to max_bytes of the
// image at byte `off` of the lane's batch (staged at lane.h_in + off, or in
// place when the DMA engine can read it) and returns the byte count -- fewer
// than max_bytes at a piece boundary of its own -- setting eof when no input
// follows (a return of 0 is the end too); sink(first_chunk, count, digests)
// receives digests in chunk order.
// BT_SHA1_TRACE=1: per-phase wall times of each pipeline run on stderr.
template <class Fill, class Sink, class Tail>
int64_t run_pipeline(DevCtx *c, uint64_t chunk_len, uint64_t size_hint, Feed feed, Fill fill, Sink sink, Tail tail) {
  if (chunk_len == 0 || chunk_len >= (1ull << 32)) {
    set_err("chunk_len must be in [1, 4 GiB)");
    return -1;
  }
  const bool staged = feed == Feed::kStaged;
  const double t_start = now_s();
  double t_fill = 0, t_wait = 0;
  if (ensure_streams(c)) return -1;
  const uint64_t bytes_per = batch_bytes_for(chunk_len, size_hint, staged);
  const uint64_t per = bytes_per / chunk_len;
  double t_alloc = 0;
  // NUMA: staged lanes on the GPU's node, staging threads on its CPUs.
  if (c->numa_node == -2) c->numa_node = gpu_numa_node(c->dev);
  const Placement place = staged ? placement_for(c->numa_node) : Placement{};
  std::atomic<int32_t> piece_nodes[BT_SHA1_STATS_NODES];
  for (auto &x : piece_nodes) x.store(0);
  struct PlaceScope {  // the staging helpers of this thread see the placement for this call only
    const Placement *prev_place;
    std::atomic<int32_t> *prev_nodes;
    PlaceScope(const Placement *p, std::atomic<int32_t> *n) : prev_place(t_place), prev_nodes(t_piece_nodes) {
      t_place = p;
      t_piece_nodes = n;
    }
    ~PlaceScope() {
      t_place = prev_place;
      t_piece_nodes = prev_nodes;
    }
  } place_scope(&place, piece_nodes);
  t_stats_valid = false;
  // Buffers are sized (grow-only, kept across calls) when a lane is first
  // used: an input that fits one batch never pins the second lane's memory.
  auto prepare = [&](Lane &l) -> int {
    const double t0 = now_s();
    if ((staged && l.h_in.ensure(bytes_per, place.node)) || l.d_in.ensure(bytes_per) || l.h_dig.ensure(20 * per) ||
        (feed == Feed::kRegistered && l.h_edge.ensure(2 * kPage)))
      return -1;
    t_alloc += now_s() - t0;
    return 0;
  };
  for (auto &l : c->lane) l.busy = false;
  const size_t kept_cap[2] = {c->lane[0].d_in.cap, c->lane[1].d_in.cap};
  // When a second batch will be needed, size lane 1 on a helper thread while
  // lane 0 is filled and copied: pinning ~1 GiB costs ~0.2-0.5 s per process.
  std::thread pre;
  int pre_rc = 0;
  std::string pre_err;
  if (size_hint > bytes_per) {
    pre = std::thread([&] {
      if (hipSetDevice(c->dev) != hipSuccess) {
        pre_rc = -1;
        pre_err = "hipSetDevice failed on the staging thread";
        return;
      }
      Lane &l = c->lane[1];
      pre_rc = (staged && l.h_in.ensure(bytes_per, place.node)) || l.d_in.ensure(bytes_per) || l.h_dig.ensure(20 * per)
                   ? -1
                   : 0;
      if (pre_rc) pre_err = t_err;
    });
  }
  struct JoinAtExit {  // every return path, including the error ones
    std::thread &t;
    ~JoinAtExit() {
      if (t.joinable()) t.join();
    }
  } join_at_exit{pre};
  auto join_pre = [&]() -> int {
    if (!pre.joinable()) return 0;
    const double t0 = now_s();
    pre.join();
    t_alloc += now_s() - t0;
    if (pre_rc) set_err("%s", pre_err.c_str());
    return pre_rc;
  };
  auto drain = [&](Lane &l) -> int {
    if (!l.busy) return 0;
    const double t0 = now_s();
    BT_CK(hipEventSynchronize(l.ev));
    t_wait += now_s() - t0;
    sink(l.first, l.count, l.h_dig.as<uint8_t>());
    l.busy = false;
    return 0;
  };
  uint64_t next = 0;
  int k = 0;
  for (;;) {
    Lane &l = c->lane[k & 1];
    if ((k == 1 && join_pre()) || drain(l) || prepare(l)) return -1;
    if (k > 0 && serial_copies(staged)) BT_CK(hipStreamWaitEvent(l.s, c->lane[(k + 1) & 1].copied, 0));
    uint64_t got = 0;
    bool eof = false;
    while (got < bytes_per && !eof) {
      // Staged input moves in pieces (host reads overlap the H2D); pinned
      // input goes as one copy per batch -- 128 MiB copies straight from
      // registered memory measured 36.5 GiB/s against 50 for 1 GiB ones.
      const uint64_t want = std::min<uint64_t>(staged ? piece_bytes() : bytes_per, bytes_per - got);
      const uint8_t *src = nullptr;
      const double t0 = now_s();
      const int64_t r = fill(l, got, want, &src, &eof);
      t_fill += now_s() - t0;
      if (r < 0) return -1;
      if (r) {
        const hipError_t ce = hipMemcpyAsync(l.d_in.as<uint8_t>() + got, src, (size_t)r, hipMemcpyHostToDevice, l.s);
        if (ce != hipSuccess) {
          set_err("hipMemcpyAsync of %llu bytes from host %p (batch %d, byte %llu of it) failed: %s",
                  (unsigned long long)r, (const void *)src, k, (unsigned long long)got, hipGetErrorString(ce));
          return -1;
        }
      }
      got += (uint64_t)r;
      if (r == 0) eof = true;
    }
    if (got == 0) break;
    if (serial_copies(staged)) BT_CK(hipEventRecord(l.copied, l.s));
    const uint64_t cnt = (got + chunk_len - 1) / chunk_len;
    if (launch_image(l.d_in.as<uint8_t>(), got, chunk_len, l.h_dig.as<uint8_t>(), l.s)) return -1;
    BT_CK(hipEventRecord(l.ev, l.s));
    l.busy = true;
    l.first = next;
    l.count = cnt;
    next += cnt;
    ++k;
    if (eof) break;
  }
  if (join_pre()) return -1;  // input shorter than the size hint
  if (tail.queue(c->lane[k & 1], k > 0 && serial_copies(staged) ? c->lane[(k + 1) & 1].copied : nullptr)) return -1;
  // Older lane first so digests arrive in order.
  if (drain(c->lane[k & 1]) || drain(c->lane[(k + 1) & 1])) return -1;
  {
    const double t0 = now_s();
    if (tail.wait()) return -1;
    t_wait += now_s() - t0;
  }
  // Direct-DMA batches bigger than a staged batch (BT_SHA1_DMA_BATCH_MB >
  // 1024) are not kept past the call: the lanes keep at most 1 GiB of HBM
  // each, so a process that shares the GPU does not lose more for good.  An
  // oversized lane goes back to what it held before the call (capped at the
  // staged size), so the next staged call finds its kept lane in place.
  if (!staged) {
    const uint64_t keep = batch_bytes_for(chunk_len, UINT64_MAX, true);
    for (int i = 0; i < 2; ++i) {
      DevBuf &d = c->lane[i].d_in;
      if (d.cap <= keep) continue;
      d.release();
      // Every digest has gone through the sink: the kept lane is only a
      // cache, so a failed re-allocation leaves it released (the next
      // call's prepare() grows it again) and the call still succeeds.
      if (kept_cap[i] && d.ensure(std::min<uint64_t>(kept_cap[i], keep))) {
        (void)hipGetLastError();
        t_err.clear();
      }
    }
  }
  const double total = now_s() - t_start;
  bt_sha1_pipeline_stats &s = t_stats;
  memset(&s, 0, sizeof s);
  s.chunks = next;
  s.bytes = 0;
  s.batch_bytes = bytes_per;
  s.batches = (uint32_t)k;
  s.staged = feed == Feed::kStaged ? 1 : feed == Feed::kRegistered ? 2 : 0;
  s.device = c->dev;
  s.copy_threads = copy_threads();
  s.numa_nodes = numa_nodes();
  s.gpu_numa_node = c->numa_node;
  s.numa_policy = place.mode();
  s.total_s = total;
  s.alloc_s = t_alloc;
  s.fill_s = t_fill;
  s.wait_s = t_wait;
  if (staged)
    for (auto &l : c->lane) page_nodes(l.h_in.p, l.h_in.cap, 64, s.lane_pages, BT_SHA1_STATS_NODES);
  for (int i = 0; i < BT_SHA1_STATS_NODES; ++i) s.copy_pieces[i] = piece_nodes[i].load();
  t_stats_valid = true;
  if (trace_on())
    fprintf(stderr, "libbtsha1 pipeline dev %d: %llu chunks, batch %llu B, %s: total %.4f s = alloc %.4f + fill %.4f "
                    "+ wait %.4f + other\n",
            c->dev, (unsigned long long)next, (unsigned long long)bytes_per,
            staged ? "staged" : feed == Feed::kRegistered ? "registered batch by batch" : "direct DMA", total, t_alloc,
            t_fill, t_wait);
  return (int64_t)next;
}

// Pageable input to bt_sha1_chunks_host: page-lock it batch by batch and DMA
// it in place (default), or copy it into the staging lanes
// (BT_SHA1_PAGEABLE=stage).  The staging copy is host memory bandwidth and
// CPU time -- 8 threads moving every byte once more -- so its rate follows
// whatever else the host's cores and memory are doing (profiles/r06: 34-50
// GiB/s on shared hosts); registering a 1 GiB batch's pages costs well under
// its 20 ms DMA and hides behind the previous batch's copy, so the pageable
// path runs at the registered-image rate.  Inputs under kRegisterMin stay
// staged (a few ms of copying at most).
constexpr uint64_t kRegisterMin = 64ull << 20;
std::atomic<int> g_pageable_feed{-1};  // BT_SHA1_PAGEABLE_REGISTER / _STAGE; -1: not read yet
int pageable_feed() {
  int v = g_pageable_feed.load();
  if (v < 0) {
    const char *e = getenv("BT_SHA1_PAGEABLE");
    const int env = (e && !strcmp(e, "stage")) ? BT_SHA1_PAGEABLE_STAGE : BT_SHA1_PAGEABLE_REGISTER;
    g_pageable_feed.compare_exchange_strong(v, env);
    v = g_pageable_feed.load();
  }
  return v;
}
bool register_pageable() { return pageable_feed() == BT_SHA1_PAGEABLE_REGISTER; }

constexpr uintptr_t page_down(uintptr_t a) { return a & ~(uintptr_t)(kPage - 1); }
constexpr uintptr_t page_up(uintptr_t a) { return page_down(a + kPage - 1); }

// One bt_sha1_chunks_host run on one device: the state its pipeline callbacks
// share, and the steps in the order chunks_host_on takes them.
//
// Registered feed, per batch [b0, b1) of the input: the whole pages inside
// it, [p0, p1), are page-locked and DMA'd in place; the head [b0, p0) and
// tail [p1, b1) -- under a page each, shared with the neighbouring batch's
// pages -- go through the lane's small pinned edge buffer.  Pages that
// cannot be registered (read-only, registered by the caller elsewhere) are
// staged through the lane instead.  Every batch is locked before the first
// copy is queued (pages locked before: ~0.1 ms per 8 GiB; never locked:
// 14-22 ms per 8 GiB under the ROCm 7.2 runtime, 69-92 ms under the 7.0
// runtime torch bundles, however the locking is placed -- per batch ahead
// of its DMA, on a helper thread, or all up front; profiles/r06).
//
// Column-split last batch (registered and direct feeds).  A pipeline's last
// chunks can only be hashed once copied, and a chunk's hash is one serial
// chain (~6.8 ms per 512 KiB in k_sha1_lat), so an unsplit pipeline ends a
// chain latency after its last byte crossed PCIe (profiles/r06: 6.8 of the
// 158 ms an 8 GiB image takes).  The last ~batch of chunks is therefore
// copied COLUMN by column: columns() 2D copies (rows = the chunks, W =
// chunk_len / columns() bytes of each; the DMA engine runs them at the 1D
// rate, tools/copy2d_probe.py) into the idle lane's device buffer, column-
// major, each hashed by k_sha1_lat's column form (chaining state in HBM) as
// soon as it has arrived, on a stream of its own, while the next column
// crosses PCIe.  After the last byte only one column's W/64 blocks remain
// (~0.9 ms for 512 KiB chunks in 8 columns).  The copies read every byte of
// their rows, so with the registered feed those rows' pages are locked too
// -- but never a page reaching past the input (the page holding its end or
// start may belong to a neighbour: another worker's slice, another call's
// buffer); the one to three chunks touching such a page, and a short last
// chunk, are copied into a pinned buffer on the host and hashed from there
// by the chain kernel on a third stream, beside the columns.
struct HostFeed {
  DevCtx *const c;
  const uint8_t *const h_in;
  const uint64_t total, chunk_len;
  uint8_t *const h_dig;
  const Feed feed;
  const uint64_t nchunks, nfull, rem;

  // plan_split
  struct Split {
    uint64_t t0 = 0, c0 = 0, c1 = 0;  // the split tail: chunks [t0, nchunks); by columns: [c0, c1)
    uint32_t parts = 0, width = 0;    // columns and their width
    bool head = false;                // chunk t0 is a leftover (c0 == t0 + 1)
    void *lock = nullptr;             // registered feed: the columns' locked pages
  } sp;
  uint64_t dma_total = 0;  // the part the lane batches carry
  // lock_batches: the registered feed's batches of lock_batch bytes; batch k's
  // whole pages are [bp0[k], bp1[k]) of the input, locked where blocked[k]
  uint64_t lock_batch = 0;
  std::vector<uint64_t> bp0, bp1;
  std::vector<char> blocked;
  // Locked ranges stay locked until the whole call is done: hipHostUnregister
  // waits for the device's outstanding work, so releasing a batch's pages
  // while the next batch's copy and hash are in flight stalled the pipeline
  // (40.5 GiB/s instead of 50.7 on 8 GiB, profiles/r06).  At the end nothing
  // is in flight and each release is quick; on an error path the streams are
  // drained first.
  std::vector<void *> regs;
  double lock_s = 0;
  // fill: the input byte the next piece starts at; registered feed: the
  // current batch's end, whole pages and whether they are locked
  uint64_t off = 0, b1 = 0, p0 = 0, p1 = 0;
  bool locked = false;
  // the tail: queued and not yet waited for; staged feed: host time gathering the columns
  bool tail_queued = false;
  double t_gather = 0;

  HostFeed(DevCtx *ctx, const uint8_t *in, uint64_t bytes, uint64_t clen, uint8_t *dig, Feed f)
      : c(ctx), h_in(in), total(bytes), chunk_len(clen), h_dig(dig), feed(f),
        nchunks((bytes + clen - 1) / clen), nfull(bytes / clen), rem(bytes % clen) {}
  HostFeed(const HostFeed &) = delete;
  HostFeed &operator=(const HostFeed &) = delete;
  // Error paths: nothing may still read the locked pages, or the caller's
  // memory, when the call returns.  After finish() there is nothing to do.
  ~HostFeed() {
    if (regs.empty() && !tail_queued) return;
    for (auto &l : c->lane)
      if (l.s) (void)hipStreamSynchronize(l.s);
    for (hipStream_t t : {c->cs, c->xs})
      if (t) (void)hipStreamSynchronize(t);
    for (void *p : regs) (void)hipHostUnregister(p);
  }

  uint64_t ntail() const { return nchunks - sp.t0; }
  uint64_t rows() const { return sp.c1 - sp.c0; }
  uint64_t nleft_full() const { return (sp.head ? 1 : 0) + (nfull - sp.c1); }

  // Page-lock [p, p + len); it stays in regs until finish() or the destructor.
  bool lock_pages(void *p, size_t len) {
    if (hipHostRegister(p, len, hipHostRegisterPortable) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    regs.push_back(p);
    return true;
  }

  // Whether the last ~batch goes by columns, which chunks, and (registered
  // feed) its pages locked.
  void plan_split() {
    const double t_lock0 = now_s();
    const uint32_t parts = split_columns(chunk_len);
    // about one batch of this feed, never more than a kept lane holds
    // (1 GiB: the idle lane carries the columns, and a staged lane is never
    // shrunk after the call)
    const uint64_t per = std::min<uint64_t>(batch_bytes_for(chunk_len, total, feed == Feed::kStaged),
                                            batch_bytes_for(chunk_len, UINT64_MAX, true)) /
                         chunk_len;
    const uint64_t t0 = nchunks - std::min<uint64_t>(nchunks, per);
    uint64_t c0 = t0, c1 = nfull;
    const uintptr_t base = (uintptr_t)h_in;
    uintptr_t lo = 0, hi = 0;
    if (feed == Feed::kRegistered) {
      const uint64_t bound = page_down(base + total) - base;  // the input's last page boundary
      c1 = std::min<uint64_t>(nfull, bound / chunk_len);      // chunks [0, c1) end at or before it
      if (page_down(base + c0 * chunk_len) < base) ++c0;      // t0 == 0, unaligned start
      lo = page_down(base + c0 * chunk_len);
      hi = page_up(base + c1 * chunk_len);
    }
    if (parts && c1 > c0 + 1 && (c1 - c0) * chunk_len >= column_min_bytes() &&
        !c->h_cdig.ensure(20 * (nchunks - t0 + 3)) && !c->h_cleft.ensure(3 * chunk_len) &&
        !c->d_cstate.ensure(20 * (c1 - c0))) {
      bool ok = true;
      if (feed == Feed::kRegistered) {
        ok = lock_pages((void *)lo, (size_t)(hi - lo));  // not locked: copied with the rest
        if (ok) {
          sp.lock = (void *)lo;
          if (trace_on())
            fprintf(stderr, "libbtsha1 lock column tail: [%p, %p)\n", (void *)lo, (void *)hi);
        }
      }
      if (ok) {
        sp.t0 = t0;
        sp.c0 = c0;
        sp.c1 = c1;
        sp.parts = parts;
        sp.width = (uint32_t)(chunk_len / parts);
        sp.head = c0 > t0;
      }
    }
    t_err.clear();
    dma_total = sp.parts ? sp.t0 * chunk_len : total;
    lock_s = now_s() - t_lock0;
  }

  // Registered feed: every batch's whole pages, locked up front.  lock_batch
  // is the direct-DMA batch (what run_pipeline cuts for this feed).
  void lock_batches() {
    lock_batch = batch_bytes_for(chunk_len, dma_total, false);
    const size_t nbatch = feed == Feed::kRegistered ? (size_t)((dma_total + lock_batch - 1) / lock_batch) : 0;
    if (!nbatch) return;
    bp0 = std::vector<uint64_t>(nbatch);
    bp1 = std::vector<uint64_t>(nbatch);
    blocked = std::vector<char>(nbatch, 0);
    const double t0 = now_s();
    const uintptr_t base = (uintptr_t)h_in;
    for (size_t k = 0; k < nbatch; ++k) {
      const uint64_t lo = k * lock_batch, hi = std::min<uint64_t>(lo + lock_batch, dma_total);
      bp0[k] = page_up(base + lo) - base;
      bp1[k] = page_down(base + hi) - base;
      if (bp1[k] <= bp0[k]) {
        bp0[k] = bp1[k] = hi;  // no whole page: the batch (< 2 pages) rides in the edge buffer
        continue;
      }
      if (lock_pages((void *)(h_in + bp0[k]), (size_t)(bp1[k] - bp0[k]))) {  // not locked: that batch is staged
        blocked[k] = 1;
        if (trace_on())
          fprintf(stderr, "libbtsha1 lock batch %zu: [%p, %p)\n", k, (const void *)(h_in + bp0[k]),
                  (const void *)(h_in + bp1[k]));
      }
    }
    lock_s += now_s() - t0;
  }

  // The columns land in the lane that is idle once the last batch is queued
  // (its previous batch's hash precedes them on its stream): sized for them
  // up front, never grown while a batch may still read it -- its device
  // buffer, and for the staged feed its staging (on the GPU's node, as the
  // pipeline places it), where the copy threads gather the columns.
  // lane_batch is the batch run_pipeline cuts for this feed (staged or not).
  int size_idle_lane() {
    if (!sp.parts) return 0;
    const bool staged = feed == Feed::kStaged;
    const uint64_t lane_batch = batch_bytes_for(chunk_len, dma_total, staged);
    const int k_last = dma_total ? (int)((dma_total + lane_batch - 1) / lane_batch) : 0;
    const uint64_t need = std::max<uint64_t>(rows() * chunk_len, dma_total ? lane_batch : 0);
    Lane &idle = c->lane[k_last & 1];
    if (idle.d_in.ensure(need)) return -1;
    if (staged) {
      if (c->numa_node == -2) c->numa_node = gpu_numa_node(c->dev);
      if (idle.h_in.ensure(need, placement_for(c->numa_node).node)) return -1;
    }
    return 0;
  }

  // run_pipeline's fill: the next piece of [0, dma_total), by feed.
  int64_t fill(Lane &l, uint64_t at, uint64_t max, const uint8_t **src, bool *eof) {
    uint64_t n = std::min<uint64_t>(max, dma_total - off);
    if (feed == Feed::kDirect) {
      *src = h_in + off;  // DMA straight from the caller's pinned image
    } else if (feed == Feed::kStaged) {
      *src = stage(l, at, n);
    } else if (fill_registered(l, at, &n, src)) {
      return -1;
    }
    off += n;
    *eof = off == dma_total;
    return (int64_t)n;
  }
  const uint8_t *stage(Lane &l, uint64_t at, uint64_t n) {
    parallel_copy(l.h_in.as<uint8_t>() + at, h_in + off, n);
    return l.h_in.as<uint8_t>() + at;
  }
  int fill_registered(Lane &l, uint64_t at, uint64_t *n, const uint8_t **src) {
    if (at == 0) {  // a new batch
      const size_t k = (size_t)(off / lock_batch);
      p0 = bp0[k];
      p1 = bp1[k];
      b1 = std::min<uint64_t>((k + 1) * lock_batch, dma_total);
      locked = blocked[k] != 0;
    }
    uint8_t *edge = l.h_edge.as<uint8_t>();
    if (off < p0) {  // head, or a batch without a whole page
      *n = std::min<uint64_t>(*n, p0 - off);
      memcpy(edge, h_in + off, *n);
      *src = edge;
    } else if (off < p1) {
      *n = std::min<uint64_t>(*n, p1 - off);
      if (locked) {
        *src = h_in + off;
      } else {
        if (l.h_in.ensure(batch_bytes_for(chunk_len, total, false), -1)) return -1;
        *src = stage(l, at, *n);
      }
    } else {  // tail
      *n = std::min<uint64_t>(*n, b1 - off);
      memcpy(edge + kPage, h_in + off, *n);
      *src = edge + kPage;
    }
    return 0;
  }

  void sink(uint64_t first, uint64_t count, const uint8_t *d) { memcpy(h_dig + 20 * first, d, 20 * count); }

  // The split tail: leftovers first (their chain runs beside the columns),
  // then each column's copy on the idle lane's stream and its hash on the
  // column stream once that copy is done.  Digest j of the tail (chunk t0 + j)
  // goes to h_cdig + 20*j; the leftovers' own launch writes theirs after the
  // tail's (h_cdig + 20*(nchunks - t0) ..) and they are moved into place.
  int queue_tail(Lane &idle, hipEvent_t last_copied) {
    if (!sp.parts) return 0;
    if (!c->cs) {
      BT_CK(hipStreamCreateWithFlags(&c->cs, hipStreamNonBlocking));
      BT_CK(hipStreamCreateWithFlags(&c->xs, hipStreamNonBlocking));
      BT_CK(hipEventCreateWithFlags(&c->cdone, hipEventDisableTiming));
      BT_CK(hipEventCreateWithFlags(&c->xdone, hipEventDisableTiming));
    }
    tail_queued = true;
    uint8_t *left = c->h_cleft.as<uint8_t>(), *tdig = c->h_cdig.as<uint8_t>();
    if (nleft_full() || rem) {
      uint64_t at = 0;
      if (sp.head) {
        memcpy(left, h_in + sp.t0 * chunk_len, chunk_len);
        at = chunk_len;
      }
      memcpy(left + at, h_in + sp.c1 * chunk_len, total - sp.c1 * chunk_len);
      BT_CK(btsha1_launch_chain(left, nullptr, nullptr, chunk_len, chunk_len, nleft_full(), tdig + 20 * ntail(), c->xs,
                                rem));
    }
    BT_CK(hipEventRecord(c->xdone, c->xs));
    if (last_copied) BT_CK(hipStreamWaitEvent(idle.s, last_copied, 0));
    // Staged feed: the copy threads gather each column into the idle lane's
    // staging (free once its previous batch is done) while the previous
    // column crosses PCIe; pinned / locked input: one strided copy per column.
    const bool staged = feed == Feed::kStaged;
    if (staged && idle.busy) BT_CK(hipEventSynchronize(idle.ev));
    uint8_t *stage = staged ? idle.h_in.as<uint8_t>() : nullptr;
    const uint64_t w = sp.width, nrows = rows();
    const ColumnRun run{idle.s, c->cs, c->cev, sp.parts, nrows, w, chunk_len, idle.d_in.as<uint8_t>(),
                        c->d_cstate.as<uint32_t>()};
    for (uint32_t j = 0; j < sp.parts; ++j) {
      const uint8_t *src = h_in + sp.c0 * chunk_len + j * w;
      uint8_t *col = run.d_cols + j * nrows * w;
      hipError_t ce;
      if (staged) {
        const double g0 = now_s();
        parallel_gather(stage + j * nrows * w, src, nrows, w, chunk_len);
        t_gather += now_s() - g0;
        ce = hipMemcpyAsync(col, stage + j * nrows * w, (size_t)(nrows * w), hipMemcpyHostToDevice, idle.s);
      } else {
        ce = hipMemcpy2DAsync(col, (size_t)w, src, (size_t)chunk_len, (size_t)w, (size_t)nrows, hipMemcpyHostToDevice,
                              idle.s);
      }
      if (ce != hipSuccess) {
        set_err("copy of column %u (%llu x %llu bytes, pitch %llu) from host %p failed: %s", j,
                (unsigned long long)nrows, (unsigned long long)w, (unsigned long long)chunk_len, (const void *)src,
                hipGetErrorString(ce));
        return -1;
      }
      if (hash_column(run, j, tdig + 20 * (sp.c0 - sp.t0))) return -1;
    }
    BT_CK(hipEventRecord(c->cdone, c->cs));
    return 0;
  }
  int wait_tail() {
    if (!tail_queued) return 0;
    BT_CK(hipEventSynchronize(c->cdone));
    BT_CK(hipEventSynchronize(c->xdone));
    tail_queued = false;
    return 0;
  }

  // n: run_pipeline's result.  Puts the tail's digests in place, completes
  // the stats and releases the locked pages (timed); returns the call's result.
  int64_t finish(int64_t n) {
    if (n >= 0 && sp.parts) {  // the tail's digests follow the batches'
      if ((uint64_t)n != sp.t0) {
        set_err("internal: %lld chunks before the split tail, expected %llu", (long long)n,
                (unsigned long long)sp.t0);
        n = -1;
      } else {
        const uint8_t *tdig = c->h_cdig.as<uint8_t>();
        uint8_t *out = h_dig + 20 * sp.t0;
        memcpy(out + 20 * (sp.c0 - sp.t0), tdig + 20 * (sp.c0 - sp.t0), 20 * rows());
        const uint8_t *ld = tdig + 20 * ntail();  // leftovers: [head] [c1, nchunks)
        if (sp.head) {
          memcpy(out, ld, 20);
          ld += 20;
        }
        memcpy(out + 20 * (sp.c1 - sp.t0), ld, 20 * (nchunks - sp.c1));
        n = (int64_t)nchunks;
        if (t_stats_valid) {
          t_stats.chunks = nchunks;
          t_stats.column_chunks = (uint32_t)rows();
          t_stats.fill_s += t_gather;
        }
      }
    }
    if (n >= 0 && t_stats_valid) {
      t_stats.bytes = total;
      page_nodes(h_in, total, 64, t_stats.src_pages, BT_SHA1_STATS_NODES);
    }
    if (n >= 0 && !regs.empty()) {  // every batch is done: release the pages (timed)
      const double t0 = now_s();
      for (void *p : regs)
        if (hipHostUnregister(p) != hipSuccess) (void)hipGetLastError();
      const double dt = now_s() - t0;
      if (t_stats_valid) {
        t_stats.registered_batches = (int32_t)(regs.size() - (sp.lock ? 1 : 0));
        t_stats.register_s = lock_s;
        t_stats.unregister_s = dt;
        t_stats.total_s += lock_s + dt;
      }
      regs.clear();
    }
    return n;
  }
};

// own: a worker context of this call (repeated device ids); NULL = the
// device's shared context.
int64_t chunks_host_on(int dev, const uint8_t *h_in, uint64_t total, uint64_t chunk_len, uint8_t *h_dig,
                       DevCtx *own = nullptr) {
  if (chunk_len == 0 || chunk_len >= (1ull << 32)) {  // before any chunk arithmetic
    set_err("chunk_len must be in [1, 4 GiB)");
    return -1;
  }
  KeepDevice keep_dev;
  DevCtx *c = own ? own : ctx_for(dev);
  if (!c) return -1;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(dev) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", dev);
    return -1;
  }
  const bool pinned = is_pinned_range(h_in, total);
  const Feed feed = pinned ? Feed::kDirect
                    : (register_pageable() && total >= kRegisterMin) ? Feed::kRegistered
                                                                      : Feed::kStaged;
  HostFeed f(c, h_in, total, chunk_len, h_dig, feed);
  f.plan_split();
  f.lock_batches();
  if (f.size_idle_lane()) return -1;
  const int64_t n = run_pipeline(
      c, chunk_len, f.dma_total, feed,
      [&f](Lane &l, uint64_t at, uint64_t max, const uint8_t **src, bool *eof) { return f.fill(l, at, max, src, eof); },
      [&f](uint64_t first, uint64_t count, const uint8_t *d) { f.sink(first, count, d); },
      tail_ops([&f](Lane &idle, hipEvent_t last_copied) { return f.queue_tail(idle, last_copied); },
               [&f] { return f.wait_tail(); }));
  return f.finish(n);
}

}  // namespace

int64_t chunks_file_on(int dev, FILE *fp, uint64_t chunk_len, const DigestSink &sink) {
  KeepDevice keep_dev;
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(dev) != hipSuccess) {
    set_err("hipSetDevice(%d) failed", dev);
    return -1;
  }
  uint64_t hint = UINT64_MAX;
  struct stat st;
  const off_t pos = ftello(fp);
  const bool regular = fstat(fileno(fp), &st) == 0 && S_ISREG(st.st_mode) && pos >= 0 && st.st_size >= pos;
  if (regular) hint = (uint64_t)(st.st_size - pos);
  uint64_t fpos = regular ? (uint64_t)pos : 0, bytes_in = 0;
  auto read_some = [&](uint8_t *dst, uint64_t max, bool *eof) -> int64_t {
    if (regular) {
      // Regular file: several threads pread the batch straight into pinned
      // memory at the FILE's logical position; short only at EOF.
      const int64_t got = parallel_pread(fileno(fp), dst, max, fpos);
      if (got < 0) {
        set_err("pread failed: %s", strerror(errno));
        return -1;
      }
      fpos += (uint64_t)got;
      *eof = (uint64_t)got < max;
      return got;
    }
    // Pipe or device: fread to EOF as chunk.c:20 does.
    size_t got = 0;
    while (got < max) {
      size_t r = fread(dst + got, 1, (size_t)(max - got), fp);
      if (r == 0) break;
      got += r;
    }
    if (ferror(fp)) {
      set_err("fread failed");
      return -1;
    }
    *eof = got < max;
    return (int64_t)got;
  };
  auto fill = [&](Lane &l, uint64_t at, uint64_t max, const uint8_t **src, bool *eof) -> int64_t {
    uint8_t *dst = l.h_in.as<uint8_t>() + at;
    *src = dst;
    const int64_t r = read_some(dst, max, eof);
    if (r > 0) bytes_in += (uint64_t)r;
    return r;
  };
  const int64_t n = run_pipeline(c, chunk_len, hint, Feed::kStaged, fill, std::cref(sink), no_tail());
  if (n >= 0 && t_stats_valid) t_stats.bytes = bytes_in;
  if (regular) {
    // Leave the stream where the reference's fread loop leaves it: at EOF,
    // with the end-of-file indicator set.
    if (fseeko(fp, (off_t)fpos, SEEK_SET) == 0) {
      const int ch = fgetc(fp);
      if (ch != EOF) ungetc(ch, fp);
    }
  }
  return n;
}

}  // namespace btsha1

using namespace btsha1;

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int64_t bt_sha1_chunks_host(const void *h_in, uint64_t total_len, uint64_t chunk_len, uint8_t *h_digests) {
  if (total_len && (!h_in || !h_digests)) {
    set_err("null pointer");
    return -1;
  }
  if (total_len == 0) return 0;
  return chunks_host_on(t_dev, (const uint8_t *)h_in, total_len, chunk_len, h_digests);
}

int64_t bt_sha1_chunks_host_devices(const void *h_in, uint64_t total_len, uint64_t chunk_len, uint8_t *h_digests,
                                    const int *devs, int nworkers) {
  if (chunk_len == 0 || chunk_len >= (1ull << 32)) {
    set_err("chunk_len must be in [1, 4 GiB)");
    return -1;
  }
  if (nworkers <= 0 || !devs) {
    set_err("empty device list");
    return -1;
  }
  if (nworkers > kMaxWorkers) {
    set_err("%d workers: at most %d (one host thread and two staging lanes each)", nworkers, kMaxWorkers);
    return -1;
  }
  if (total_len == 0) return 0;
  if (!h_in || !h_digests) {
    set_err("null pointer");
    return -1;
  }
  const int avail = device_count();
  if (avail <= 0) {
    set_err("no HIP device visible");
    return -1;
  }
  for (int g = 0; g < nworkers; ++g)
    if (devs[g] < 0 || devs[g] >= avail) {
      set_err("device %d out of range (%d visible)", devs[g], avail);
      return -1;
    }
  const uint64_t n = (total_len + chunk_len - 1) / chunk_len;
  // Contiguous block split of the chunk index: worker g gets
  // [g*n/G, (g+1)*n/G) -- possibly empty when G > n; only the globally last
  // chunk can be short.  One host thread per worker; a device listed k times
  // gets k independent contexts (streams + staging lanes), so the split,
  // staging and ordered gather run exactly as on k distinct GPUs.  The first
  // use of a device takes its shared context; the repeats get contexts of
  // their own that are released (buffers, streams) before the call returns.
  std::vector<int64_t> rc(nworkers, 0);
  std::vector<std::string> errs(nworkers);
  std::vector<std::unique_ptr<DevCtx>> own(nworkers);
  for (int g = 0; g < nworkers; ++g)
    for (int h = 0; h < g; ++h)
      if (devs[h] == devs[g]) {
        own[g] = std::make_unique<DevCtx>();
        own[g]->dev = devs[g];
        break;
      }
  struct ReleaseAtExit {
    std::vector<std::unique_ptr<DevCtx>> &v;
    ~ReleaseAtExit() {
      for (auto &c : v) release_ctx(c.get());
    }
  } release_at_exit{own};
  std::vector<std::thread> th;
  for (int g = 0; g < nworkers; ++g) {
    th.emplace_back([&, g] {
      const uint64_t lo = n * g / nworkers, hi = n * (g + 1) / nworkers;
      if (lo == hi) return;
      const uint64_t off = lo * chunk_len;
      const uint64_t bytes = std::min<uint64_t>(hi * chunk_len, total_len) - off;
      rc[g] = chunks_host_on(devs[g], (const uint8_t *)h_in + off, bytes, chunk_len, h_digests + 20 * lo, own[g].get());
      if (rc[g] >= 0 && (uint64_t)rc[g] != hi - lo) {
        rc[g] = -1;
        t_err = "short digest count";
      }
      errs[g] = t_err;
    });
  }
  for (auto &t : th) t.join();
  for (int g = 0; g < nworkers; ++g)
    if (rc[g] < 0) {
      t_err = "worker " + std::to_string(g) + " (device " + std::to_string(devs[g]) + "): " + errs[g];
      return -1;
    }
  return (int64_t)n;
}

int64_t bt_sha1_chunks_host_multi(const void *h_in, uint64_t total_len, uint64_t chunk_len, uint8_t *h_digests,
                                  int ndev) {
  const int avail = device_count();
  if (avail <= 0) {
    set_err("no HIP device visible");
    return -1;
  }
  if (ndev <= 0 || ndev > avail) ndev = avail;
  std::vector<int> devs(ndev);
  for (int g = 0; g < ndev; ++g) devs[g] = g;
  return bt_sha1_chunks_host_devices(h_in, total_len, chunk_len, h_digests, devs.data(), ndev);
}

int bt_sha1_set_pageable_feed(int feed) {
  if (feed != BT_SHA1_PAGEABLE_REGISTER && feed != BT_SHA1_PAGEABLE_STAGE) {
    set_err("pageable feed %d: BT_SHA1_PAGEABLE_REGISTER (0) or BT_SHA1_PAGEABLE_STAGE (1)", feed);
    return -1;
  }
  const int prev = pageable_feed();
  g_pageable_feed.store(feed);
  return prev;
}

int bt_sha1_get_pipeline_stats(bt_sha1_pipeline_stats *out) {
  if (!out) {
    set_err("null pointer");
    return -1;
  }
  if (!t_stats_valid) {
    set_err("no host pipeline has run on this thread");
    return -1;
  }
  *out = t_stats;
  return 0;
}

int64_t bt_sha1_chunks_file(void *fp, uint64_t chunk_len, uint8_t *h_digests, uint64_t max_chunks) {
  if (!fp || !h_digests) {
    set_err("null pointer");
    return -1;
  }
  bool overflow = false;
  int64_t n = chunks_file_on(t_dev, (FILE *)fp, chunk_len, [&](uint64_t first, uint64_t count, const uint8_t *d) {
    for (uint64_t i = 0; i < count; ++i) {
      if (first + i >= max_chunks) {
        overflow = true;
        return;
      }
      memcpy(h_digests + 20 * (first + i), d + 20 * i, 20);
    }
  });
  if (n >= 0 && overflow) {
    set_err("file has more than max_chunks chunks");
    return -1;
  }
  return n;
}

}  // extern "C"
