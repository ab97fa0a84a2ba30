// bt_runtime.cpp -- the base of libbtsha1.so's host runtime (include/bt_sha1.h):
// the thread's error text and device, the per-device contexts with their
// streams, the whole-chunk launches, and the small and device-resident entry
// points -- device count / selection, build info and source id, variant and
// batch setters, bt_sha1_*_dev, the synthetic fill, host registration, the
// digest lookup and the debug hooks.
//
// The reference has no counterpart for most of this; the device-resident
// entry points batch what it does a chunk at a time:
//   shahash over a chunk           chunk.c:33-49  (bt_sha1_chunks_dev)
//   hash + memcmp of save_chunk    util.c:304-337 (bt_sha1_verify_dev)
//
// Host-side work here is bookkeeping only; every compression runs in a HIP
// kernel.  No CPU hashing path.
#include "bt_runtime.h"

#include <cstdarg>
#include <memory>
#include <vector>

namespace btsha1 {

thread_local std::string t_err;
__thread int t_dev = 0;
std::atomic<int> g_variant{310};  // ring 3 x 128-byte slots, default cache policy

void set_err(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  t_err = buf;
}

[[noreturn]] void die(const char *where) {
  fprintf(stderr, "libbtsha1: %s: %s\n", where, t_err.c_str());
  fflush(stderr);
  abort();
}

bool trace_on() {
  static const bool on = [] {
    const char *e = getenv("BT_SHA1_TRACE");
    return e && *e && *e != '0';
  }();
  return on;
}

namespace {
std::mutex g_ctx_mu;
std::vector<std::unique_ptr<DevCtx>> g_ctx;
}  // namespace

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

DevCtx *ctx_for(int dev) {
  std::lock_guard<std::mutex> g(g_ctx_mu);
  int n = device_count();
  if (n <= 0) {
    set_err("no HIP device visible (hipGetDeviceCount = 0)");
    return nullptr;
  }
  if (dev < 0 || dev >= n) {
    set_err("device %d out of range (%d visible)", dev, n);
    return nullptr;
  }
  if ((int)g_ctx.size() < n) g_ctx.resize(n);
  if (!g_ctx[dev]) {
    auto c = std::make_unique<DevCtx>();
    c->dev = dev;
    KeepDevice keep_dev;
    if (hipSetDevice(dev) != hipSuccess) {
      set_err("cannot initialise HIP device %d", dev);
      return nullptr;
    }
    g_ctx[dev] = std::move(c);
  }
  return g_ctx[dev].get();
}

// Everything a context holds: its streams (drained first), staging lanes and
// drop-in buffers.  Used for the per-call worker contexts of repeated device
// ids in bt_sha1_chunks_host_devices, which must not outlive the call.
void release_ctx(DevCtx *c) {
  if (!c) return;
  KeepDevice keep_dev;
  if (hipSetDevice(c->dev) != hipSuccess) return;
  for (auto &l : c->lane) {
    if (l.s) {
      (void)hipStreamSynchronize(l.s);
      (void)hipStreamDestroy(l.s);
    }
    if (l.ev) (void)hipEventDestroy(l.ev);
    if (l.copied) (void)hipEventDestroy(l.copied);
    l.copied = nullptr;
    l.s = nullptr;
    l.ev = nullptr;
    l.h_in.release();
    l.h_dig.release();
    l.h_edge.release();
    l.d_in.release();
  }
  c->s = nullptr;
  c->h_msg.release();
  c->h_state.release();
  c->h_cdig.release();
  c->h_cleft.release();
  c->d_cstate.release();
  for (hipEvent_t &e : c->cev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  for (hipEvent_t *e : {&c->cdone, &c->xdone}) {
    if (*e) (void)hipEventDestroy(*e);
    *e = nullptr;
  }
  for (hipStream_t *t : {&c->cs, &c->xs}) {
    if (*t) (void)hipStreamDestroy(*t);
    *t = nullptr;
  }
}

// Streams are created on first use and kept few: HIP multiplexes streams onto
// GPU_MAX_HW_QUEUES (4) hardware queues, and two streams that share a queue
// serialise -- which silently kills the H2D/hash overlap of the pipelines.
int ensure_streams(DevCtx *c) {
  std::lock_guard<std::mutex> g(g_ctx_mu);
  if (c->s) return 0;
  for (auto &l : c->lane) {
    BT_CK(hipStreamCreateWithFlags(&l.s, hipStreamNonBlocking));
    BT_CK(hipEventCreateWithFlags(&l.ev, hipEventDisableTiming));
    BT_CK(hipEventCreateWithFlags(&l.copied, hipEventDisableTiming));
  }
  c->s = c->lane[0].s;
  return 0;
}

namespace {

// Caller streams of the device-resident entry points.  NULL is the device's
// null (default) stream, exactly as for a hipLaunchKernelGGL(..., 0, ...) of the
// caller's own: ordered after the caller's earlier default-stream work (e.g.
// torch's default stream, whose handle is 0) and before its later work.  The
// library's own non-blocking streams serve only its host pipelines.
hipStream_t pick_stream(void *stream) { return (hipStream_t)stream; }

bool fast_layout(const void *d_in, uint64_t chunk_len, uint64_t pitch, const void *d_dig) {
  return ((uintptr_t)d_in & 15) == 0 && (pitch & 15) == 0 && ((uintptr_t)d_dig & 3) == 0 &&
         chunk_len <= pitch && 64 * pitch + 4096 <= (1ull << 32);  // 32-bit buffer offsets incl. prefetch overrun
}

// Launch the right kernel(s) for n equal chunks of len bytes at pitch.
int launch_chunks(const void *d_in, uint64_t n, uint64_t len, uint64_t pitch, uint8_t *d_dig, hipStream_t s) {
  if (n == 0) return 0;
  if (fast_layout(d_in, len, pitch, d_dig)) {
    BT_CK(btsha1_launch_fixed(d_in, n, (uint32_t)pitch, (uint32_t)len, d_dig, nullptr, nullptr, s, g_variant.load()));
  } else {
    if (len >= (1ull << 32)) {
      set_err("chunk_len %llu exceeds 4 GiB", (unsigned long long)len);
      return -1;
    }
    BT_CK(btsha1_launch_ragged(d_in, nullptr, nullptr, pitch, (uint32_t)len, n, d_dig, s));
  }
  return 0;
}

}  // namespace

// A contiguous image: full chunks through the hot kernel, a short last chunk
// (make_chunks' final fread, chunk.c:20) in the same launch as its tail wave
// when the layout allows, else through the ragged kernel after it.
int launch_image(const uint8_t *d_img, uint64_t bytes, uint64_t chunk_len, uint8_t *d_dig, hipStream_t s) {
  const uint64_t nfull = bytes / chunk_len, rem = bytes % chunk_len;
  if (fast_layout(d_img, chunk_len, chunk_len, d_dig)) {
    BT_CK(btsha1_launch_fixed(d_img, nfull, (uint32_t)chunk_len, (uint32_t)chunk_len, d_dig, nullptr, nullptr, s,
                              g_variant.load(), (uint32_t)rem));
    return 0;
  }
  if (launch_chunks(d_img, nfull, chunk_len, chunk_len, d_dig, s)) return -1;
  if (rem) BT_CK(btsha1_launch_ragged(d_img + nfull * chunk_len, nullptr, nullptr, 0, (uint32_t)rem, 1,
                                      d_dig + 20 * nfull, s));
  return 0;
}

}  // namespace btsha1

using namespace btsha1;

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int bt_sha1_device_count(void) { return device_count(); }

int bt_sha1_set_device(int device) {
  int n = device_count();
  if (device < 0 || device >= n) {
    set_err("device %d out of range (%d visible)", device, n);
    return -1;
  }
  t_dev = device;
  return 0;
}

const char *bt_sha1_last_error(void) { return t_err.c_str(); }

#ifndef BT_SHA1_SRC_ID
#define BT_SHA1_SRC_ID "unknown"
#endif

const char *bt_sha1_build_info(void) {
  static thread_local char info[192];
  const uint64_t lat = btsha1_latency_batch_setting();
  char latbuf[48];
  if (lat == BT_SHA1_LATENCY_AUTO)
    snprintf(latbuf, sizeof latbuf, "auto");
  else
    snprintf(latbuf, sizeof latbuf, "%llu", (unsigned long long)lat);
  snprintf(info, sizeof info, "libbtsha1 gfx950 hip%d.%d ring=%d latency_batch=%s src=%s", HIP_VERSION_MAJOR,
           HIP_VERSION_MINOR, g_variant.load(), latbuf, BT_SHA1_SRC_ID);
  return info;
}

const char *bt_sha1_source_id(void) { return BT_SHA1_SRC_ID; }

int bt_sha1_set_ring_depth(int nbuf) { return bt_sha1_set_variant(nbuf, 1, 0); }

uint64_t bt_sha1_set_latency_batch(uint64_t max_chunks) {
  const uint64_t prev = btsha1_latency_batch_setting();
  btsha1_set_latency_batch(max_chunks);
  return prev;
}

uint64_t bt_sha1_set_chain_batch(uint64_t max_messages) {
  const uint64_t prev = btsha1_chain_batch_setting();
  btsha1_set_chain_batch(max_messages);
  return prev;
}

uint64_t bt_sha1_set_seglist_latency_batch(uint64_t max_messages) {
  const uint64_t prev = btsha1_seglist_latency_batch_setting();
  btsha1_set_seglist_latency_batch(max_messages);
  return prev;
}

uint64_t bt_sha1_set_segchain_batch(uint64_t max_messages) {
  const uint64_t prev = btsha1_segchain_batch_setting();
  btsha1_set_segchain_batch(max_messages);
  return prev;
}

const char *bt_sha1_seglist_kernel_name(uint64_t n) { return btsha1_seglist_kernel_name(n); }

const char *bt_sha1_kernel_name(uint64_t n_chunks) {
  if (device_count() <= 0) {
    set_err("no HIP device visible");
    return nullptr;
  }
  return btsha1_fixed_kernel_name(n_chunks, g_variant.load());
}

int bt_sha1_clock_probe(const void *d_in, uint64_t n, uint64_t chunk_len, uint64_t pitch, uint8_t *d_digests,
                        uint64_t *d_stamps, void *stream) {
  if (n == 0) return 0;
  if (!d_in || !d_digests || !d_stamps) {
    set_err("null pointer");
    return -1;
  }
  if (!fast_layout(d_in, chunk_len, pitch, d_digests)) {
    set_err("clock probe needs the hot kernel's layout");
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  if (!ctx_for(dev)) return -1;
  BT_CK(btsha1_launch_fixed_stamped(d_in, n, (uint32_t)pitch, (uint32_t)chunk_len, d_digests, d_stamps,
                                    pick_stream(stream), g_variant.load()));
  return 0;
}

int64_t bt_sha1_wallclock_khz(void) {
  int dev = 0, khz = 0;
  BT_CK(hipGetDevice(&dev));
  BT_CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
  return khz;
}

int bt_sha1_debug_barrier_stats(uint64_t out[3], int reset) {
  if (!out) {
    set_err("null pointer");
    return -1;
  }
  const hipError_t e = btsha1_debug_barrier_stats(out, reset);
  if (e == hipErrorNotSupported) {
    set_err("barrier tallies exist only in the -DBT_SHA1_DEBUG_BARRIERS build (make dbgbar)");
    return -1;
  }
  BT_CK(e);
  return 0;
}

int64_t bt_sha1_debug_dropin_residue(int device) {
  DevCtx *c = nullptr;
  {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    if (device < 0) {
      set_err("device %d out of range", device);
      return -1;
    }
    if (device < (int)g_ctx.size()) c = g_ctx[device].get();
  }
  if (!c) return 0;  // no drop-in call has run on this device: nothing staged
  std::lock_guard<std::mutex> g(c->mu);
  int64_t nz = 0;
  const uint8_t *m = c->h_msg.as<uint8_t>();
  for (size_t i = 0; m && i < c->h_msg.cap; ++i) nz += m[i] != 0;
  const uint8_t *st = c->h_state.as<uint8_t>();
  for (size_t i = 0; st && i < kStateBytes; ++i) nz += st[i] != 0;
  return nz;
}

int bt_sha1_set_variant(int nbuf, int lines, int nt) {
  const int code = nbuf * 100 + lines * 10 + (nt ? 1 : 0);
  if (!btsha1_fixed_variant_ok(code)) {
    if (btsha1_experiments_build())
      set_err("no hot-kernel variant ring=%d lines=%d nt=%d", nbuf, lines, nt);
    else
      set_err("no hot-kernel variant ring=%d lines=%d nt=%d in the product library: it carries only the default "
              "(3, 1, 0); the rejected variants are in build_variants/experiments/libbtsha1.so (make experiments)",
              nbuf, lines, nt);
    return -1;
  }
  g_variant.store(code);
  return 0;
}

int bt_sha1_chunks_dev(const void *d_in, uint64_t n, uint64_t chunk_len, uint64_t pitch, uint8_t *d_digests,
                       void *stream) {
  if (n && (!d_in || !d_digests)) {
    set_err("null pointer");
    return -1;
  }
  if (n > 1 && pitch < chunk_len) {
    set_err("pitch < chunk_len");
    return -1;
  }
  if (n == 1 && pitch < chunk_len) pitch = (chunk_len + 15) & ~15ull;
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  return launch_chunks(d_in, n, chunk_len, pitch, d_digests, st);
}

int bt_sha1_verify_dev(const void *d_in, uint64_t n, uint64_t chunk_len, uint64_t pitch, const uint8_t *d_expected,
                       uint8_t *d_ok, uint8_t *d_digests, void *stream) {
  if (n == 0) return 0;
  if (!d_in || !d_expected || !d_ok) {
    set_err("null pointer");
    return -1;
  }
  if (!fast_layout(d_in, chunk_len, pitch, d_digests)) {
    set_err("verify needs a 16-byte aligned layout with 64*pitch + 4096 <= 4 GiB");
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  BT_CK(btsha1_launch_fixed(d_in, n, (uint32_t)pitch, (uint32_t)chunk_len, d_digests, d_expected, d_ok, st,
                            g_variant.load()));
  return 0;
}

int bt_sha1_column_dev(const void *d_col, uint64_t n, uint64_t pitch, uint64_t width, int part, uint32_t *d_state,
                       uint64_t msg_len, uint8_t *d_digests, const uint8_t *d_expected, uint8_t *d_ok, void *stream) {
  if (n == 0) return 0;
  if (!d_col || !d_state) {
    set_err("null pointer");
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  // The launcher takes 32-bit pitch and width: what does not fit is refused
  // here, like its own 64*pitch < 4 GiB, not truncated into something valid.
  const hipError_t e = pitch >> 32 || width >> 32
                           ? hipErrorInvalidValue
                           : btsha1_launch_column(d_col, n, (uint32_t)pitch, (uint32_t)width, part, d_state, msg_len,
                                                  d_digests, st, d_expected, d_ok);
  if (e != hipSuccess) {
    set_err("column launch (part %d, n %llu, width %llu, pitch %llu) refused: %s", part, (unsigned long long)n,
            (unsigned long long)width, (unsigned long long)pitch, hipGetErrorString(e));
    return -1;
  }
  return 0;
}

int bt_sha1_ragged_dev(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
                       uint8_t *d_digests, void *stream) {
  if (n == 0) return 0;
  if (!d_base || !d_offsets || !d_lens || !d_digests) {
    set_err("null pointer");
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  BT_CK(btsha1_launch_ragged(d_base, d_offsets, d_lens, 0, 0, n, d_digests, st));
  return 0;
}

int bt_sha1_ragged_verify_dev(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
                              const uint8_t *d_expected, uint8_t *d_ok, uint8_t *d_digests, void *stream) {
  if (n == 0) return 0;
  if (!d_base || !d_offsets || !d_lens || !d_expected || !d_ok) {
    set_err("null pointer");
    return -1;
  }
  if (n > BTSHA1_RAGGED_VERIFY_MAX) {  // one workgroup per message in the chain form
    set_err("ragged verify: %llu messages exceed the grid limit of %llu per launch", (unsigned long long)n,
            (unsigned long long)BTSHA1_RAGGED_VERIFY_MAX);
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  BT_CK(btsha1_launch_ragged_verify(d_base, d_offsets, d_lens, 0, 0, n, d_digests, d_expected, d_ok, st));
  return 0;
}

static int gather_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_first,
                      const uint32_t *d_seg_count, uint64_t n, uint8_t *d_digests, const uint8_t *d_expected,
                      uint8_t *d_ok, bool verify, void *stream) {
  if (n == 0) return 0;
  if (!d_base || !d_segs || !d_seg_first || !d_seg_count || (verify ? !d_expected || !d_ok : !d_digests)) {
    set_err("null pointer");
    return -1;
  }
  if (n > BTSHA1_GATHER_MAX) {  // one message per lane of 64-thread workgroups
    set_err("gather: %llu messages exceed the grid limit of %llu per launch", (unsigned long long)n,
            (unsigned long long)BTSHA1_GATHER_MAX);
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  BT_CK(btsha1_launch_gather(d_base, d_segs, d_seg_first, d_seg_count, n, d_digests, d_expected, d_ok, st));
  return 0;
}

int bt_sha1_gather_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_first,
                       const uint32_t *d_seg_count, uint64_t n, uint8_t *d_digests, void *stream) {
  return gather_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_digests, nullptr, nullptr, false, stream);
}

int bt_sha1_gather_verify_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_first,
                              const uint32_t *d_seg_count, uint64_t n, const uint8_t *d_expected, uint8_t *d_ok,
                              uint8_t *d_digests, void *stream) {
  return gather_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_digests, d_expected, d_ok, true, stream);
}

// Fixed-size packet buffers (k_sha1_pkts).  Everything the launcher would
// refuse is refused here with a message, before any device call.
__attribute__((noinline)) static int pkts_dev(const void *d_base, const bt_sha1_pkt_geom *geom, const uint64_t *d_slot_off,
                    const uint32_t *d_len, const uint32_t *d_order, const uint64_t *d_order_first, uint64_t n,
                    uint8_t *d_digests, const uint8_t *d_expected, uint8_t *d_ok, bool verify, void *stream) {
  if (!d_base || !geom || !d_slot_off || !d_len || !d_order || !d_order_first ||
      (verify ? !d_expected || !d_ok : !d_digests)) {
    set_err("null pointer");
    return -1;
  }
  if (((geom->stride | geom->header | geom->payload) & 3u) || geom->payload < 64u ||
      (uint64_t)geom->header + geom->payload > geom->stride || geom->slot_pkts == 0 ||
      (uint64_t)geom->slot_pkts * geom->stride > (1ull << 32)) {
    set_err("pkts: geometry %u/%u/%u x %u outside the rule (bt_sha1.h)", geom->stride, geom->header, geom->payload,
            geom->slot_pkts);
    return -1;
  }
  if (n > BTSHA1_PKTS_MAX) {
    set_err("pkts: %llu messages exceed the grid limit", (unsigned long long)n);
    return -1;
  }
  if (n == 0) return 0;
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  BT_CK(btsha1_launch_pkts(d_base, &geom->stride, d_slot_off, d_len, d_order, d_order_first, n, d_digests, d_expected,
                           d_ok, pick_stream(stream)));
  return 0;
}

int bt_sha1_pkts_dev(const void *d_base, const bt_sha1_pkt_geom *geom, const uint64_t *d_slot_off,
                     const uint32_t *d_len, const uint32_t *d_order, const uint64_t *d_order_first, uint64_t n,
                     uint8_t *d_digests, void *stream) {
  return pkts_dev(d_base, geom, d_slot_off, d_len, d_order, d_order_first, n, d_digests, nullptr, nullptr, false,
                  stream);
}

int bt_sha1_pkts_verify_dev(const void *d_base, const bt_sha1_pkt_geom *geom, const uint64_t *d_slot_off,
                            const uint32_t *d_len, const uint32_t *d_order, const uint64_t *d_order_first, uint64_t n,
                            const uint8_t *d_expected, uint8_t *d_ok, uint8_t *d_digests, void *stream) {
  return pkts_dev(d_base, geom, d_slot_off, d_len, d_order, d_order_first, n, d_digests, d_expected, d_ok, true,
                  stream);
}

// Diagnostic, like bt_sha1_column_dev: ONE launch of the chain form of the
// segment-list kernels whatever bt_sha1_set_segchain_batch says.  What the
// launcher would refuse is refused here with a message, before any device call.
int bt_sha1_segchain_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_first,
                         const uint32_t *d_seg_count, uint64_t n, const uint8_t *d_expected, uint8_t *d_ok,
                         uint8_t *d_digests, uint32_t piece_bytes, void *stream) {
  if (n == 0) return 0;
  if (!d_base || !d_segs || !d_seg_first || !d_seg_count) {
    set_err("null pointer");
    return -1;
  }
  if (!d_expected != !d_ok) {
    set_err("segchain: d_expected and d_ok come together or not at all");
    return -1;
  }
  if (!d_ok && !d_digests) {
    set_err("segchain: neither d_digests nor d_ok: nothing to write");
    return -1;
  }
  const uint32_t piece = piece_bytes ? piece_bytes : BTSHA1_SEGCHAIN_PIECE;
  if ((piece & 63u) || piece > BTSHA1_SEGCHAIN_PIECE) {
    set_err("segchain: piece_bytes %u must be 0 or a 64-byte multiple of at most %u", piece_bytes,
            BTSHA1_SEGCHAIN_PIECE);
    return -1;
  }
  if (n > BTSHA1_RESUME_MAX) {  // one workgroup per message
    set_err("segchain: %llu messages exceed the grid limit of %llu per launch", (unsigned long long)n,
            (unsigned long long)BTSHA1_RESUME_MAX);
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  BT_CK(btsha1_launch_gather_chain(d_base, d_segs, d_seg_first, d_seg_count, n, d_digests, d_expected, d_ok, piece,
                                   st));
  return 0;
}

int bt_sha1_states_init_dev(uint32_t *d_states, uint64_t n, void *stream) {
  if (n == 0) return 0;
  if (!d_states) {
    set_err("null pointer");
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  if (!ctx_for(dev)) return -1;
  BT_CK(btsha1_launch_states_init(d_states, n, pick_stream(stream)));
  return 0;
}

int bt_sha1_resume_dev(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens, const uint64_t *d_totals,
                       uint64_t n, uint32_t *d_states, uint8_t *d_digests, const uint8_t *d_expected, uint8_t *d_ok,
                       void *stream) {
  if (n == 0) return 0;
  if (!d_base || !d_offsets || !d_lens || !d_totals || !d_states) {
    set_err("null pointer");
    return -1;
  }
  if (d_ok && !d_expected) {
    set_err("null pointer: d_ok needs d_expected");
    return -1;
  }
  if (n > BTSHA1_RESUME_MAX) {  // one workgroup per message
    set_err("resume: %llu messages exceed the grid limit of %llu per launch", (unsigned long long)n,
            (unsigned long long)BTSHA1_RESUME_MAX);
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  if (!ctx_for(dev)) return -1;
  BT_CK(btsha1_launch_resume(d_base, d_offsets, d_lens, d_totals, n, d_states, d_digests, d_expected, d_ok,
                             pick_stream(stream)));
  return 0;
}

int bt_sha1_dgram_chain_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_pos,
                            const uint64_t *d_seg_first, const uint32_t *d_seg_count, const uint64_t *d_from,
                            const uint32_t *d_lens, const uint64_t *d_totals, uint64_t n, uint32_t *d_states,
                            uint8_t *d_digests, const uint8_t *d_expected, uint8_t *d_ok, void *stream) {
  if (n == 0) return 0;
  if (!d_base || !d_segs || !d_seg_pos || !d_seg_first || !d_seg_count || !d_from || !d_lens || !d_totals ||
      !d_states) {
    set_err("null pointer");
    return -1;
  }
  if (d_ok && !d_expected) {
    set_err("null pointer: d_ok needs d_expected");
    return -1;
  }
  if (n > BTSHA1_RESUME_MAX) {  // one workgroup per message
    set_err("gather resume: %llu messages exceed the grid limit of %llu per launch", (unsigned long long)n,
            (unsigned long long)BTSHA1_RESUME_MAX);
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  if (!ctx_for(dev)) return -1;
  BT_CK(btsha1_launch_gather_resume(d_base, d_segs, d_seg_pos, d_seg_first, d_seg_count, d_from, d_lens, d_totals, n,
                                    d_states, d_digests, d_expected, d_ok, pick_stream(stream)));
  return 0;
}

int bt_sha1_fill_synthetic(void *d_buf, uint64_t nbytes, uint64_t first_word, uint64_t seed, void *stream) {
  if (nbytes && (!d_buf || ((uintptr_t)d_buf & 15))) {
    set_err("fill needs a non-null 16-byte aligned buffer");
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  BT_CK(btsha1_launch_fill(d_buf, nbytes, first_word, seed, st));
  return 0;
}

int bt_sha1_host_register(void *h_ptr, uint64_t len) {
  if (!h_ptr || !len) {
    set_err("null pointer or zero length");
    return -1;
  }
  if (!ctx_for(t_dev)) return -1;
  BT_CK(hipHostRegister(h_ptr, (size_t)len, hipHostRegisterPortable));
  return 0;
}

int bt_sha1_host_unregister(void *h_ptr) {
  BT_CK(hipHostUnregister(h_ptr));
  return 0;
}

int bt_sha1_lookup_dev(const uint8_t *d_table, uint64_t n_table, const uint8_t *d_queries, uint64_t n_queries,
                       int64_t *d_index, void *stream) {
  if (n_queries == 0) return 0;
  // cap below is a uint32_t of at least 2 * n_table: past 2^30 entries it
  // would have to be 2^32, and the doubling loop would wrap to 0 and never end.
  if (n_table > (1ull << 30)) {
    set_err("lookup table too large");
    return -1;
  }
  if ((n_table && !d_table) || !d_queries || !d_index || ((uintptr_t)d_table & 3) || ((uintptr_t)d_queries & 3)) {
    set_err("lookup needs non-null, 4-byte aligned digest arrays");
    return -1;
  }
  int dev = 0;
  BT_CK(hipGetDevice(&dev));
  DevCtx *c = ctx_for(dev);
  if (!c) return -1;
  hipStream_t st = pick_stream(stream);
  uint32_t cap = 1024;
  while (cap < 2 * n_table) cap <<= 1;  // load factor <= 1/2
  void *slots = nullptr;
  BT_CK(hipMallocAsync(&slots, (size_t)cap * 4, st));
  BT_CK(btsha1_launch_lookup(d_table, n_table, d_queries, n_queries, (uint32_t *)slots, cap, d_index, st));
  BT_CK(hipFreeAsync(slots, st));
  return 0;
}

}  // extern "C"
