// bt_runtime.h -- internals the host runtime's components share (not installed):
// error and buffer plumbing, the per-device context with its two staging
// lanes, and what crosses a file boundary between
//   bt_runtime.cpp   contexts, whole-chunk launches, small and device-resident entry points
//   bt_hostmem.cpp   NUMA placement, staging memory, the threaded host copies
//   bt_columns.cpp   the column split's plan and its per-column step
//   bt_pipeline.cpp  the two-lane host pipelines and their feeds (chunk.c:13-25)
//   bt_dropin.cpp    sha.h / chunk.h (sha.c:149-163, 453-558; chunk.c:13-83)
//   bt_verifier.cpp  the batched verifier (util.c:304-337)
//   bt_receiver.cpp  the progressive receiver (util.c:250-337, hashed while received)
//   bt_intake.cpp    the same for up to 512 chunks at once, one launch per kick
// Everything here is in one namespace with hidden visibility: shared between
// the library's objects, absent from its dynamic symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>

#include <sched.h>

#include "bt_sha1.h"
#include "sha1_launch.h"

namespace btsha1 __attribute__((visibility("hidden"))) {

// The thread-locals with a trivial initialiser are __thread, not thread_local:
// for an extern thread_local the compiler tests a weak reference to the
// variable's dynamic-init function, and under hidden visibility that test is
// resolved wrongly when no such function exists (the call then jumps into the
// library's ELF header).  t_err has one, so thread_local is right for it.
extern thread_local std::string t_err;
extern __thread int t_dev;
extern std::atomic<int> g_variant;  // ring 3 x 128-byte slots, default cache policy

void set_err(const char *fmt, ...);

#define BT_CK(expr)                                                                  \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) {                                                          \
      set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -1;                                                                     \
    }                                                                                \
  } while (0)

[[noreturn]] void die(const char *where);

// Entry points that must switch devices (host pipelines, drop-in calls, the
// verifier) give the caller's thread its current device back on return, so
// a caller that drives its own HIP work (torch on cuda:N) is not moved.
struct KeepDevice {
  int prev = -1;
  KeepDevice() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~KeepDevice() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
  KeepDevice(const KeepDevice &) = delete;
  KeepDevice &operator=(const KeepDevice &) = delete;
};

// Grow-only device / pinned scratch.
constexpr uint32_t kMaxColumns = 16;  // column-split tail: most columns per chunk (HostFeed)

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t need) {
    if (need <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t sz = std::max<size_t>(need, 4096);
    BT_CK(hipMalloc(&p, sz));
    cap = sz;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};
struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t need) {
    if (need <= cap) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t sz = std::max<size_t>(need, 4096);
    BT_CK(hipHostMalloc(&p, sz, hipHostMallocDefault));
    cap = sz;
    return 0;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};

// Grow-only staging buffer of the host pipelines, read only by the DMA engine
// (hipMemcpyAsync): anonymous memory on transparent huge pages, first-touched
// by several threads, then page-locked with hipHostRegister.  Per GiB on
// MI355X boxes (tools/ubench/pin_cost.hip): ~3 ms to register + the touch
// (65 ms on one thread), against 222-251 ms for hipHostMalloc -- the pinning
// was most of a make-chunks run on a 1 GiB file.  Same H2D rate (~57 GB/s).
struct StageBuf {  // bt_hostmem.cpp
  void *p = nullptr;
  size_t cap = 0;
  void release();
  // node >= 0: the pages prefer that NUMA node (placed at first touch).
  int ensure(size_t need, int node = -1);
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};

// One double-buffered staging lane of the host pipelines.
struct Lane {
  hipStream_t s = nullptr;
  hipEvent_t ev = nullptr;
  hipEvent_t copied = nullptr;  // after the batch's last H2D (serial copy order)
  StageBuf h_in;  // staged input pieces, DMA'd to d_in
  PinBuf h_dig;   // the kernel stores digests straight into it
  PinBuf h_edge;  // registered-batch mode: the batch's unaligned head / tail bytes
  DevBuf d_in;
  bool busy = false;
  uint64_t first = 0, count = 0;  // chunk range in flight
};

struct DevCtx {
  int dev = 0;
  int numa_node = -2;  // the GPU's NUMA node (-1 unknown; -2 not read yet)
  std::mutex mu;
  hipStream_t s = nullptr;  // drop-in calls and NULL-stream launches (= lane[0].s)
  Lane lane[2];
  PinBuf h_msg, h_state;  // drop-in calls: message / chaining state, read and written by the chain kernel
  // Host pipelines' column-split last batch (HostFeed): its digests, its
  // few chunks that are not split (hashed from a pinned copy), the chunks'
  // chaining state between columns, the column and leftover streams, an event
  // per column copy and one after each stream's work.
  PinBuf h_cdig, h_cleft;
  DevBuf d_cstate;
  hipStream_t cs = nullptr, xs = nullptr;
  hipEvent_t cev[kMaxColumns] = {}, cdone = nullptr, xdone = nullptr;
  uint32_t seq = 0;       // drop-in calls: completion word the chain kernel stores at h_state + 32
};

// ---- bt_runtime.cpp ----------------------------------------------------------
int device_count();
DevCtx *ctx_for(int dev);
void release_ctx(DevCtx *c);
int ensure_streams(DevCtx *c);
int launch_image(const uint8_t *d_img, uint64_t bytes, uint64_t chunk_len, uint8_t *d_dig, hipStream_t s);
bool trace_on();  // BT_SHA1_TRACE=1: per-phase wall times of each pipeline run on stderr
inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
constexpr uint64_t kPage = 4096;     // host page (registration granule)
constexpr size_t kStateBytes = 32;   // drop-in calls: bytes of h_state that hold data (bt_dropin.cpp)

// ---- bt_hostmem.cpp ----------------------------------------------------------
enum NumaMode { kNumaOff = 0, kNumaLanes = 1, kNumaGpu = 2 };
// Staging placement of one call: the node to bind the lanes to and the CPUs
// (within the calling thread's affinity mask) the copy threads run on.
struct Placement {
  int node = -1;      // -1: no placement
  int ncpus = 0;      // 0: threads unpinned
  cpu_set_t cpus;
  int mode() const { return node < 0 ? kNumaOff : ncpus > 0 ? kNumaGpu : kNumaLanes; }
};
Placement placement_for(int gpu_node);
int gpu_numa_node(int dev);
int numa_nodes();
void page_nodes(const void *p, uint64_t len, int samples, int32_t *counts, int ncounts);
// The calling thread's current placement (set by run_pipeline for the
// duration of one call; read by the staging helpers on that thread).
extern __thread const Placement *t_place;
extern __thread std::atomic<int32_t> *t_piece_nodes;  // per-node piece tally of the call
int copy_threads();
void parallel_copy(uint8_t *dst, const uint8_t *src, uint64_t n);
void parallel_gather(uint8_t *dst, const uint8_t *src, uint64_t rows, uint64_t width, uint64_t pitch);
int64_t parallel_pread(int fd, uint8_t *dst, uint64_t want, uint64_t pos);

// ---- bt_pipeline.cpp ---------------------------------------------------------
// The staged file pipeline on device dev: fp to EOF in chunks of chunk_len;
// sink(first_chunk, count, digests) receives digests in chunk order, once per
// batch.  Returns the chunk count or -1.
using DigestSink = std::function<void(uint64_t, uint64_t, const uint8_t *)>;
int64_t chunks_file_on(int dev, FILE *fp, uint64_t chunk_len, const DigestSink &sink);

}  // namespace btsha1
