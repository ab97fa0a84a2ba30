// bt_hostmem.cpp -- host memory of the pipelines: NUMA topology and the
// placement of the staging lanes, the staging buffer itself, and the threaded
// copy helpers (memcpy, column gather, pread) that fill it.
//
// Stands in for the reference's single-threaded fread into a stack buffer
// (make_chunks, chunk.c:18-22): the same bytes, moved by several threads into
// memory the DMA engine reads.
#include "bt_runtime.h"

#include <thread>
#include <vector>

#include <pthread.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <cerrno>

namespace btsha1 {

namespace {

// ---- NUMA placement of the host pipelines' staging ---------------------------
// The GPU hangs off one socket's PCIe root.  The staging lanes are written by
// the copy threads and read by the DMA engine; placing their pages on the
// GPU's node and running the copy threads on that node's CPUs keeps both
// local (the caller's pageable input is wherever the caller touched it).
// Topology from sysfs, no libnuma: node N's CPUs from
// /sys/devices/system/node/nodeN/cpulist, the GPU's node from
// /sys/bus/pci/devices/<bdf>/numa_node.
struct NumaTopo {
  int nodes = 1;
  std::vector<int> cpu_node;               // cpu -> node
  std::vector<std::vector<int>> node_cpus;  // node -> cpus
};

std::vector<int> parse_cpulist(const char *s) {
  std::vector<int> out;
  while (*s) {
    char *end = nullptr;
    const long a = strtol(s, &end, 10);
    if (end == s) break;
    long b = a;
    s = end;
    if (*s == '-') {
      b = strtol(s + 1, &end, 10);
      s = end;
    }
    for (long c = a; c <= b && c < 65536; ++c) out.push_back((int)c);
    while (*s == ',' || *s == '\n' || *s == ' ') ++s;
  }
  return out;
}

const NumaTopo &numa_topo() {
  static const NumaTopo t = [] {
    NumaTopo r;
    int present = 0;
    for (int n = 0; n < 256; ++n) {
      char path[96], buf[4096];
      snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", n);
      FILE *f = fopen(path, "r");
      if (!f) continue;
      const size_t got = fread(buf, 1, sizeof buf - 1, f);
      fclose(f);
      buf[got] = 0;
      ++present;
      r.node_cpus.resize(n + 1);
      r.node_cpus[n] = parse_cpulist(buf);
      for (int c : r.node_cpus[n]) {
        if ((int)r.cpu_node.size() <= c) r.cpu_node.resize(c + 1, -1);
        r.cpu_node[c] = n;
      }
    }
    r.nodes = std::max(1, present);
    return r;
  }();
  return t;
}

int node_of_cpu(int cpu) {
  const NumaTopo &t = numa_topo();
  return cpu >= 0 && cpu < (int)t.cpu_node.size() ? t.cpu_node[cpu] : -1;
}

// Staging placement (BT_SHA1_NUMA): "off" = none (pages wherever the kernel
// puts them, copy threads unpinned); "lanes" (default) = the lanes' pages
// prefer the GPU's node, so the DMA engine reads local memory; "gpu" = that,
// and the copy threads run on the node's CPUs.  Applies only when the machine
// has more than one node and the GPU's node is known.  Measured on MI355X
// boxes (tools/numa_probe.py, profiles/r06/numa_place.md), 8 GiB images on
// either node: off 49.0-50.4, lanes 50.1-50.5 GiB/s; pinning the copy
// threads to the GPU node's cores cost 15-30 % on hosts whose cores other
// jobs share (34.5-40.7 GiB/s), so it is not the default.
constexpr int kNumaDefault = kNumaLanes;
int numa_mode() {
  static const int m = [] {
    const char *e = getenv("BT_SHA1_NUMA");
    if (!e || !*e) return (int)kNumaDefault;
    if (!strcmp(e, "off") || !strcmp(e, "0")) return (int)kNumaOff;
    if (!strcmp(e, "lanes")) return (int)kNumaLanes;
    return (int)kNumaGpu;
  }();
  return m;
}

// Preferred (not strict) policy: pages go to `node` while it has memory.
void prefer_node(void *p, size_t len, int node) {
  if (node < 0 || node >= 256) return;
  unsigned long mask[4] = {0, 0, 0, 0};
  mask[node / 64] = 1ul << (node % 64);
  const int kMpolPreferred = 1;
  (void)syscall(SYS_mbind, p, (unsigned long)len, kMpolPreferred, mask, 256ul, 0u);
}

}  // namespace

int numa_nodes() { return numa_topo().nodes; }

// The NUMA node the device's PCI function reports (-1: unknown).
int gpu_numa_node(int dev) {
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, sizeof bdf, dev) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  for (char *p = bdf; *p; ++p)
    if (*p >= 'A' && *p <= 'F') *p = (char)(*p + 32);
  char path[160];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE *f = fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  return node;
}

// Pages of [p, p+len) sampled evenly (at most `samples`), counted per node
// (move_pages with no target nodes only queries).  Pages not yet faulted in
// count nowhere.
void page_nodes(const void *p, uint64_t len, int samples, int32_t *counts, int ncounts) {
  if (!p || !len || samples <= 0) return;
  const uint64_t pg = 4096, first = (uintptr_t)p & ~(pg - 1), last = ((uintptr_t)p + len - 1) & ~(pg - 1);
  const uint64_t npages = (last - first) / pg + 1;
  const int n = (int)std::min<uint64_t>((uint64_t)samples, npages);
  std::vector<void *> pages(n);
  std::vector<int> status(n, -1);
  for (int i = 0; i < n; ++i) pages[i] = (void *)(first + pg * (npages * (uint64_t)i / (uint64_t)n));
  if (syscall(SYS_move_pages, 0, (unsigned long)n, pages.data(), nullptr, status.data(), 0) != 0) return;
  for (int s : status)
    if (s >= 0 && s < ncounts) ++counts[s];
}

Placement placement_for(int gpu_node) {
  Placement pl;
  CPU_ZERO(&pl.cpus);
  const NumaTopo &t = numa_topo();
  const int mode = numa_mode();
  if (mode == kNumaOff || gpu_node < 0 || t.nodes < 2 || gpu_node >= (int)t.node_cpus.size()) return pl;
  if (mode == kNumaLanes) {
    pl.node = gpu_node;
    return pl;
  }
  cpu_set_t aff;
  CPU_ZERO(&aff);
  if (sched_getaffinity(0, sizeof aff, &aff) != 0) return pl;
  for (int c : t.node_cpus[gpu_node])
    if (c < CPU_SETSIZE && CPU_ISSET(c, &aff)) {
      CPU_SET(c, &pl.cpus);
      ++pl.ncpus;
    }
  if (pl.ncpus == 0) return pl;  // none of the GPU's CPUs usable: leave placement to the kernel
  pl.node = gpu_node;
  return pl;
}

__thread const Placement *t_place = nullptr;
__thread std::atomic<int32_t> *t_piece_nodes = nullptr;

// Host staging threads for the pipelines' CPU side (memcpy into pinned memory,
// file reads): one core moves ~8 GB/s, PCIe takes ~53.  BT_SHA1_COPY_THREADS
// overrides the default of 8.
int copy_threads() {
  static const int n = [] {
    const char *e = getenv("BT_SHA1_COPY_THREADS");
    const int v = e ? atoi(e) : 8;
    return v < 1 ? 1 : (v > 64 ? 64 : v);
  }();
  return n;
}

namespace {

// Split [0, n) into page-aligned pieces of at least 16 MiB, one per thread
// (the caller's thread takes the first), and run body(off, len, piece) on each.
// Under a pipeline call's NUMA placement (t_place) every piece runs on a
// helper thread pinned to the GPU node's CPUs (the caller's own affinity is
// left alone); staging pieces (tally) are counted by the node of the CPU
// they started on.
template <class Body>
void parallel_pieces(uint64_t n, Body body, bool tally = false) {
  const uint64_t min_piece = 16ull << 20;
  int t = copy_threads();
  if ((uint64_t)t > n / min_piece) t = (int)std::max<uint64_t>(1, n / min_piece);
  uint64_t piece = (n + t - 1) / t;
  piece = (piece + 4095) & ~4095ull;
  const Placement *pl = t_place;
  std::atomic<int32_t> *counts = tally ? t_piece_nodes : nullptr;
  const bool pin = pl && pl->ncpus > 0;
  auto run = [&, pl, counts, pin](int i) {
    if (pin) (void)pthread_setaffinity_np(pthread_self(), sizeof pl->cpus, &pl->cpus);
    if (counts) {
      const int nd = node_of_cpu(sched_getcpu());
      if (nd >= 0 && nd < BT_SHA1_STATS_NODES) counts[nd].fetch_add(1, std::memory_order_relaxed);
    }
    body((uint64_t)i * piece, std::min<uint64_t>(piece, n - (uint64_t)i * piece), i);
  };
  std::vector<std::thread> th;
  for (int i = pin ? 0 : 1; i < t && (uint64_t)i * piece < n; ++i) th.emplace_back(run, i);
  if (!pin) run(0);
  for (auto &x : th) x.join();
}

void touch_parallel(uint8_t *p, uint64_t n) {
  parallel_pieces(n, [&](uint64_t off, uint64_t len, int) {
    for (uint64_t o = 0; o < len; o += 4096) p[off + o] = 0;
  });
}

}  // namespace

void StageBuf::release() {
  if (!p) return;
  (void)hipHostUnregister(p);
  munmap(p, cap);
  p = nullptr;
  cap = 0;
}

int StageBuf::ensure(size_t need, int node) {
  if (need <= cap) return 0;
  release();
  const size_t sz = (std::max<size_t>(need, 4096) + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
  void *q = mmap(nullptr, sz, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (q == MAP_FAILED) {
    set_err("staging mmap of %zu bytes failed: %s", sz, strerror(errno));
    return -1;
  }
  (void)madvise(q, sz, MADV_HUGEPAGE);  // a hint: 4 KiB pages still work
  // Not inherited by fork(): a child (e.g. a subprocess about to exec) would
  // otherwise get a copy of every page-locked page at fork time.
  (void)madvise(q, sz, MADV_DONTFORK);
  prefer_node(q, sz, node);
  touch_parallel((uint8_t *)q, sz);
  const hipError_t e = hipHostRegister(q, sz, hipHostRegisterPortable);
  if (e != hipSuccess) {
    munmap(q, sz);
    set_err("hipHostRegister of the staging buffer failed: %s", hipGetErrorString(e));
    return -1;
  }
  p = q;
  cap = sz;
  return 0;
}

void parallel_copy(uint8_t *dst, const uint8_t *src, uint64_t n) {
  if (n < (32ull << 20) && !(t_place && t_place->ncpus > 0)) {
    if (t_piece_nodes) {
      const int nd = node_of_cpu(sched_getcpu());
      if (nd >= 0 && nd < BT_SHA1_STATS_NODES) t_piece_nodes[nd].fetch_add(1, std::memory_order_relaxed);
    }
    memcpy(dst, src, n);
    return;
  }
  parallel_pieces(n, [&](uint64_t off, uint64_t len, int) { memcpy(dst + off, src + off, len); }, true);
}

// Gather one column of `rows` strided rows into a dense buffer with the copy
// threads: dst[r*width ..] = src[r*pitch ..] (width bytes per row).
void parallel_gather(uint8_t *dst, const uint8_t *src, uint64_t rows, uint64_t width, uint64_t pitch) {
  parallel_pieces(
      rows * width,
      [&](uint64_t off, uint64_t len, int) {
        for (uint64_t o = off, end = off + len; o < end;) {
          const uint64_t r = o / width, in = o % width, k = std::min<uint64_t>(width - in, end - o);
          memcpy(dst + o, src + r * pitch + in, k);
          o += k;
        }
      },
      true);
}

// pread `want` bytes at file offset `pos` into dst with several threads.
// Returns the length of the contiguous prefix read (short only at EOF), or -1.
int64_t parallel_pread(int fd, uint8_t *dst, uint64_t want, uint64_t pos) {
  std::vector<int64_t> got(64, 0);
  std::vector<uint64_t> asked(64, 0);
  std::atomic<bool> err{false};
  parallel_pieces(want, [&](uint64_t off, uint64_t len, int i) {
    asked[i] = len;
    uint64_t done = 0;
    while (done < len) {
      const ssize_t r = pread(fd, dst + off + done, (size_t)(len - done), (off_t)(pos + off + done));
      if (r < 0) {
        if (errno == EINTR) continue;
        err = true;
        break;
      }
      if (r == 0) break;  // EOF
      done += (uint64_t)r;
    }
    got[i] = (int64_t)done;
  }, true);
  if (err) return -1;
  int64_t total = 0;
  for (int i = 0; i < 64 && asked[i]; ++i) {
    total += got[i];
    if ((uint64_t)got[i] < asked[i]) break;  // EOF inside piece i
  }
  return total;
}

}  // namespace btsha1
