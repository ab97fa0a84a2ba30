/*
 * bt_sha1.h -- C-ABI of the MI355X SHA-1 chunk-hashing path (libbtsha1.so).
 *
 * Drop-in surface (declared in sha.h / chunk.h of this directory, which keep
 * the reference's prototypes source-compatible):
 *   SHA1Init / SHA1Update / SHA1Final   replace reference sha.h:58-60
 *   make_chunks / shahash               replace reference chunk.h:25,28
 *   binary2hex / hex2binary             replace reference chunk.h:31,34
 * Every digest is computed by the HIP kernels of
 * bittorrent-with-congestion-control_amd/csrc/ on the GPU; there is no CPU
 * hashing path in this library.  If no GPU / HIP runtime is usable the
 * int-returning entry points return -1 (bt_sha1_last_error() says why) and
 * the void ones (shahash, SHA1Update, SHA1Final) print the error and abort().
 *
 * Additions with no reference counterpart (batching is what makes a GPU pay):
 * device-resident batches, ragged batches, a batched asynchronous verifier
 * that replaces the synchronous shahash + memcmp of util.c:311-313, a host
 * pipeline over pinned buffers, a multi-GPU host split, and the frozen
 * synthetic generator used by the bench and the tests.
 *
 * Conventions: plain pointers and sizes; `stream` is a hipStream_t passed as
 * void* (NULL = the current device's null/default stream, so a call is
 * ordered with the caller's default-stream work, e.g. torch's default stream,
 * exactly like a kernel the caller launches on stream 0); device
 * pointers are prefixed d_, host pointers h_.  Return 0 (or a count) on
 * success, -1 on error.
 */
#ifndef BT_SHA1_H
#define BT_SHA1_H

#include <stddef.h>
#include <stdint.h>

#include "sha.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BT_SHA1_DIGEST_SIZE 20

/* ---- runtime ---------------------------------------------------------- */
/* Number of visible GPUs (0 if none), without creating any context. */
int bt_sha1_device_count(void);
/* Select the device used by the drop-in calls on this thread (default 0). */
int bt_sha1_set_device(int device);
/* Human-readable description of the last error on this thread. */
const char *bt_sha1_last_error(void);
/* Library / kernel build description (arch, ring depth, latency threshold,
 * source id). */
const char *bt_sha1_build_info(void);
/* Id of the kernel sources this library was compiled from (first 16 hex
 * digits of the SHA-256 of sha1_kernels.hip + sha1_device.h, comments
 * stripped, so comment edits keep it): ties profiles
 * (PMC traffic, rocprof summaries) to the build that produced them. */
const char *bt_sha1_source_id(void);
/* Hot-kernel register-ring depth in 128-byte lines (default 3).  The product
 * library carries only the default hot kernel (3 slots of one line, plain
 * loads) and accepts only 3; the measured-and-rejected variants (2 or 4
 * slots, two-line slots, non-temporal loads, and 10 = the LDS-staged
 * k_sha1_lds) are compiled into build_variants/experiments/libbtsha1.so
 * (`make experiments`) alone. */
int bt_sha1_set_ring_depth(int nbuf);
/* Hot-kernel variant: nbuf ring slots of `lines` 128-byte lines each, nt = 1
 * for non-temporal loads.  Returns -1 (message names the experiments
 * library) for a combination this library does not carry: in the product
 * library, anything but (3, 1, 0). */
int bt_sha1_set_variant(int nbuf, int lines, int nt);
/* Batches of at most max_chunks chunks take the latency kernel (a loader /
 * schedule wave and a round wave per 64 chunks, meeting in LDS), which
 * shortens a lone chunk's serial chain; larger batches take the hot-kernel
 * variant above.  0 disables it; UINT64_MAX (the default) = 128 chunks per
 * compute unit of the launching device (32768 on a full MI355X).  Returns the
 * previous setting. */
uint64_t bt_sha1_set_latency_batch(uint64_t max_chunks);
/* Ragged batches (bt_sha1_ragged_dev, strided fallbacks) of at most
 * max_messages messages take the chain kernel -- one two-wave workgroup per
 * message, the lowest latency a single serial chain gets (shahash and the
 * SHA1Update/SHA1Final midstate always use it); larger batches the
 * one-message-per-lane ragged kernel.  0 disables it; UINT64_MAX (default) =
 * two per compute unit.  Returns the previous setting. */
uint64_t bt_sha1_set_chain_batch(uint64_t max_messages);
/* Segment-list batches (bt_sha1_gather_dev, bt_sha1_gather_verify_dev, a
 * gather verifier's batch launch) of at most max_messages messages take the
 * latency form k_sha1_gather_lat: a loader wave that walks the segment lists
 * and a round wave per 64 messages, as the latency kernel above; larger
 * batches the one-message-per-lane kernel.  0 (the default) disables it;
 * UINT64_MAX = 128 messages per compute unit of the launching device.
 * Returns the previous setting; needs no device. */
uint64_t bt_sha1_set_seglist_latency_batch(uint64_t max_messages);
/* The same batches of at most max_messages messages take the CHAIN form
 * k_sha1_gather_chain instead: one two-wave workgroup per message, the lowest
 * latency for the handful of chunks a peer has in flight (max_conn).  It is
 * asked before the latency form above.  0 (the default) disables it;
 * UINT64_MAX = two messages per compute unit of the launching device, as
 * bt_sha1_set_chain_batch's default.  Returns the previous setting; needs no
 * device. */
uint64_t bt_sha1_set_segchain_batch(uint64_t max_messages);
/* Name of the kernel a segment-list batch of n messages runs under the
 * current settings and device: "k_sha1_gather_chain", "k_sha1_gather_lat<2>"
 * (at most one workgroup per compute unit), "k_sha1_gather_lat<3>" or
 * "k_sha1_gather".  Needs no device (256 compute units are assumed without
 * one). */
const char *bt_sha1_seglist_kernel_name(uint64_t n);
/* Name of the kernel a fixed-layout batch of n_chunks chunks runs on the
 * current device ("k_sha1_chain" up to two chunks per CU, "k_sha1_lat" up to
 * the latency batch, else "k_sha1_fixed" -- or, in the experiments library
 * with variant 10, "k_sha1_lds");
 * NULL without a device. */
const char *bt_sha1_kernel_name(uint64_t n_chunks);
/* Diagnostic (bench clock measurement): hashes the batch like
 * bt_sha1_chunks_dev through a separately compiled build of the hot kernel
 * whose lane 0 of every wave stores {s_memtime, s_memrealtime} before and
 * after its main loop into d_stamps[4*w .. 4*w+3] (w = chunk index / 64;
 * d_stamps holds 4*ceil(n/64) uint64).  The in-kernel shader clock is
 * delta(memtime) / delta(realtime) * bt_sha1_wallclock_khz().  The production
 * kernel executes no stamp. */
int bt_sha1_clock_probe(const void *d_in, uint64_t n, uint64_t chunk_len, uint64_t pitch, uint8_t *d_digests,
                        uint64_t *d_stamps, void *stream);
/* Rate of s_memrealtime on the current device in kHz (100000 on MI355X). */
int64_t bt_sha1_wallclock_khz(void);
/* Diagnostic (barrier-accounting build, `make dbgbar`): the latency, chain
 * and ragged-latency kernels meet s_barrier from different call sites in
 * their two waves and are correct only while both waves execute the same
 * count.  That build tallies, over every such wave since the last reset,
 * out[0] = waves checked, out[1] = barriers executed, out[2] = waves whose
 * count broke the invariant.  Synchronises the current device first; reset
 * != 0 zeroes the tallies after reading.  Returns -1 in the production
 * library, which counts nothing. */
int bt_sha1_debug_barrier_stats(uint64_t out[3], int reset);

/* Diagnostic: bytes still nonzero in the pinned staging the drop-in calls
 * (shahash, SHA1Update, SHA1Final) copy the message and the chaining state
 * into on `device` -- every call zeroes what it staged before it returns, as
 * the reference leaves no copy behind (chunk.c:48; sha.c:165-174, 526), so
 * this is 0 between calls.  0 when no drop-in call has run on the device;
 * -1 for a negative device.  Scans the whole staging buffer: a test hook, not
 * for hot loops. */
int64_t bt_sha1_debug_dropin_residue(int device);
/* Diagnostic: ONE launch of the latency kernel's column form, which the host
 * pipelines' column-split tail and the verifier's split batches chain per
 * chunk (test hook: they reach it only with chunks of 64 KiB or more).
 * Column `part` (0 first, 1 middle, 2 last) of n chunks: chunk i's column is
 * `width` bytes (a 64-byte multiple) at d_col + i*pitch (16-byte aligned;
 * pitch >= width, a 16-byte multiple, 64*pitch < 4 GiB).  d_state (5*n
 * uint32, device memory) carries each chunk's chaining state from column to
 * column, word k of chunk i at d_state[k*n + i]: the first part starts from
 * the SHA-1 IV and writes it, a middle part advances it, the last part reads
 * it, appends the padding of a msg_len-byte message (the bytes of all the
 * parts) and writes digest i to d_digests + 20*i (4-byte aligned) -- and with
 * d_ok (last part only) d_ok[i] = digest i == d_expected[20*i ..], where
 * d_digests may be NULL.  Returns -1, with nothing launched, for arguments
 * the launcher refuses. */
int bt_sha1_column_dev(const void *d_col, uint64_t n, uint64_t pitch, uint64_t width, int part,
                       uint32_t *d_state, uint64_t msg_len, uint8_t *d_digests,
                       const uint8_t *d_expected, uint8_t *d_ok, void *stream);

/* ---- device-resident batches (the hot path) ---------------------------- */
/* n chunks of chunk_len bytes, chunk i at d_in + i*pitch (pitch >= chunk_len).
 * d_digests receives 20*n bytes, digest i = SHA-1(chunk i) as sha.c:545-556
 * serialises it.  Fast path when d_in and pitch are 16-byte aligned and
 * 64*pitch + 4096 <= 4 GiB; any other layout takes the generic kernel. */
int bt_sha1_chunks_dev(const void *d_in, uint64_t n, uint64_t chunk_len, uint64_t pitch,
                       uint8_t *d_digests, void *stream);
/* Same, then compares with d_expected (20*n): d_ok[i] = 1 iff equal
 * (util.c:311-313).  d_digests may be NULL. */
int bt_sha1_verify_dev(const void *d_in, uint64_t n, uint64_t chunk_len, uint64_t pitch,
                       const uint8_t *d_expected, uint8_t *d_ok, uint8_t *d_digests, void *stream);
/* n messages, message i = d_base[d_offsets[i] .. + d_lens[i]). */
int bt_sha1_ragged_dev(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
                       uint64_t n, uint8_t *d_digests, void *stream);
/* Same, then compares with d_expected (20*n): d_ok[i] = 1 iff digest i equals
 * d_expected[20*i .. 20*i+19], else 0 (util.c:311-313) -- the verify form for
 * chunks of any length at any offset, e.g. a file's short last chunk (the last
 * fread of make_chunks, chunk.c:20), which bt_sha1_verify_dev does not take.
 * d_expected, d_ok and d_digests take any alignment; d_digests may be NULL.
 * The batch size selects the kernel as for bt_sha1_ragged_dev, under
 * bt_sha1_set_chain_batch and bt_sha1_set_latency_batch.  n == 0 is no work;
 * a null d_base / d_offsets / d_lens / d_expected / d_ok, or n above 2^31 - 1
 * (the grid), are -1 before any device call. */
int bt_sha1_ragged_verify_dev(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
                              uint64_t n, const uint8_t *d_expected, uint8_t *d_ok,
                              uint8_t *d_digests /* may be NULL */, void *stream);
/* Scatter-gather: message i is the concatenation, in list order, of the
 * d_seg_count[i] segments d_segs[d_seg_first[i] ..], each d_base[off .. off +
 * len) -- a chunk hashed where its DATA datagrams landed, never assembled
 * (save_data_packet's memcpy, util.c:275).  Offsets and lengths take any
 * value (length 0 included), segments any address order; messages may share
 * or overlap segments; d_seg_count[i] == 0 is the empty message.  No byte
 * outside the listed segments is read.  Data and tables may be device or
 * pinned host memory.  n == 0 is no work; a null d_base / d_segs /
 * d_seg_first / d_seg_count (/ d_digests, or d_expected / d_ok), or n above
 * (2^31 - 1) * 64 (the grid), are -1 before any device call. */
typedef struct {
  uint64_t off;      /* from d_base (commit_gather: from the slot)            */
  uint32_t len;
  uint32_t reserved; /* not read                                              */
} bt_sha1_seg;
int bt_sha1_gather_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_first,
                       const uint32_t *d_seg_count, uint64_t n, uint8_t *d_digests, void *stream);
int bt_sha1_gather_verify_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_first,
                              const uint32_t *d_seg_count, uint64_t n, const uint8_t *d_expected,
                              uint8_t *d_ok, uint8_t *d_digests /* may be NULL */, void *stream);
/* Fixed-size packet buffers (k_sha1_pkts): a chunk hashed where recvmmsg put
 * its DATA datagrams, an array of equal buffers, with no segment list -- the
 * host writes one uint32_t per datagram.  A slot is slot_pkts packet buffers
 * `stride` bytes apart; every datagram of a message carries `payload` bytes
 * behind a `header`-byte header, its last one what is left.  Message i is
 * d_len[i] bytes (0: the empty message); with npkt = ceil(len / payload), its
 * byte m has sequence position k = m / payload, lies in packet buffer
 * j = d_order[d_order_first[i] + k], at
 *   d_base + d_slot_off[i] + j*stride + header + m % payload.
 * Arrival order is free and a duplicate datagram's buffer is simply never
 * named; positions may name one buffer twice.  d_slot_off[i] must be a
 * multiple of 4 (the caller's contract: other values give the right digest,
 * slowly).  Data and arrays may be device or pinned host memory; digests,
 * d_expected and d_ok take any alignment.
 * What is read: for message i no byte outside [d_slot_off[i], d_slot_off[i] +
 * slot_pkts*stride) whatever d_order holds (entries are clamped to
 * slot_pkts - 1), and no d_order entry at or past npkt; bytes of the slot
 * outside the listed payloads may be read and influence no result.
 * -1 with a message, before any device call: a null array (d_expected and
 * d_ok are both required by the verify form); n above (2^31 - 1) * 64 (the
 * grid); stride, header or payload not a multiple of 4; payload < 64;
 * header + payload > stride; slot_pkts == 0; slot_pkts * stride above 2^32.
 * n == 0 is no work.  Callers with other geometries (odd sizes, short
 * payloads, headers of varying size) use bt_sha1_gather_dev. */
typedef struct {
  uint32_t stride;    /* bytes from one packet buffer to the next             */
  uint32_t header;    /* bytes in front of the payload in every buffer        */
  uint32_t payload;   /* payload bytes of every datagram but a message's last */
  uint32_t slot_pkts; /* packet buffers per slot                              */
} bt_sha1_pkt_geom;
int bt_sha1_pkts_dev(const void *d_base, const bt_sha1_pkt_geom *geom /* host */, const uint64_t *d_slot_off,
                     const uint32_t *d_len, const uint32_t *d_order, const uint64_t *d_order_first, uint64_t n,
                     uint8_t *d_digests, void *stream);
int bt_sha1_pkts_verify_dev(const void *d_base, const bt_sha1_pkt_geom *geom /* host */, const uint64_t *d_slot_off,
                            const uint32_t *d_len, const uint32_t *d_order, const uint64_t *d_order_first,
                            uint64_t n, const uint8_t *d_expected, uint8_t *d_ok,
                            uint8_t *d_digests /* may be NULL */, void *stream);
/* Diagnostic, like bt_sha1_column_dev: ONE launch of the segment-list
 * kernels' chain form (k_sha1_gather_chain: one two-wave workgroup per
 * message, which needs no position table -- it builds one in LDS, a window of
 * 1024 non-empty segments at a time) whatever bt_sha1_set_segchain_batch
 * says.  Messages, tables and results as bt_sha1_gather_verify_dev's;
 * d_expected and d_ok come together or not at all (without them: digests
 * only), d_digests may be NULL with them.  piece_bytes caps the bytes hashed
 * per pass over a window: 0 is the production value (2^31), a test passes a
 * small 64-byte multiple to put piece boundaries inside its messages; the
 * results do not depend on it.  n == 0 is no work; a null d_base / d_segs /
 * d_seg_first / d_seg_count, one of d_expected / d_ok without the other,
 * neither d_ok nor d_digests, a piece_bytes that is no 64-byte multiple or
 * above 2^31, or n above 2^31 - 1 (the grid) are -1 before any device call. */
int bt_sha1_segchain_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_first,
                         const uint32_t *d_seg_count, uint64_t n, const uint8_t *d_expected, uint8_t *d_ok,
                         uint8_t *d_digests, uint32_t piece_bytes, void *stream);
/* Resumable hashing of messages that are still arriving (a peer appends a
 * chunk's payloads in order, util.c:275, and hashes it only when complete,
 * util.c:311-313; SHA-1 resumes at every 64-byte boundary).  This is the
 * LATENCY form: one two-wave workgroup per message, any n, meant for the
 * handful of chunks a peer has in flight -- batches of whole chunks belong to
 * bt_sha1_chunks_dev.
 * bt_sha1_states_init_dev: d_states[5*i ..] = the SHA-1 IV (sha.c:149-163)
 * for i < n.
 * bt_sha1_resume_dev: n messages, one launch.  Message i's next d_lens[i]
 * bytes are at d_base + d_offsets[i] (any alignment; device or pinned host
 * memory; no byte at or past d_offsets[i] + d_lens[i] is read, so the caller
 * may be writing there), its chaining state at d_states[5*i ..] in
 * SHA1Context.hash order (device or pinned host memory).
 *   d_totals[i] == 0: advance -- the d_lens[i] / 64 whole blocks are
 *     compressed into the state; d_lens[i] == 0 leaves it as it was.
 *   d_totals[i] != 0: finish -- d_lens[i] are the last bytes (any count, 0
 *     included) of a d_totals[i]-byte message whose first d_totals[i] -
 *     d_lens[i] bytes, a 64-byte multiple, were advanced before; the padding
 *     of sha.c:536-543 is appended and digest i written.  The state is not
 *     written back.
 * d_digests / d_expected / d_ok as in bt_sha1_verify_dev (d_digests may be
 * NULL, and any alignment is taken): d_ok needs d_expected; entries of
 * advancing messages are left untouched.  n == 0 is no work; null d_base /
 * d_offsets / d_lens / d_totals / d_states, d_ok without d_expected, or n
 * above 2^31 - 1 (the grid) are -1 before any device call. */
int bt_sha1_states_init_dev(uint32_t *d_states, uint64_t n, void *stream);
int bt_sha1_resume_dev(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
                       const uint64_t *d_totals, uint64_t n, uint32_t *d_states, uint8_t *d_digests,
                       const uint8_t *d_expected, uint8_t *d_ok, void *stream);
/* The two together: resumable hashing of messages given as SEGMENT LISTS that
 * are still growing -- a chunk received as datagrams, hashed where recvfrom put
 * them over the in-sequence prefix that has arrived (the chain-form gather
 * kernel: one two-wave workgroup per message, the latency form; with d_from =
 * 0 and d_lens = d_totals it is gather's latency form for a handful of whole
 * chunks).  Message i's segments listed so far are d_segs[d_seg_first[i] .. +
 * d_seg_count[i]); d_seg_pos is parallel to d_segs: the entry of message i's
 * segment k is the sum of the lengths of its segments before k.  The launch
 * hashes message bytes [d_from[i], d_from[i] + d_lens[i]) into d_states[5*i ..].
 * The caller keeps: d_from[i] a 64-byte multiple; the range inside the listed
 * bytes; for a finish (d_totals[i] != 0), d_from[i] + d_lens[i] == d_totals[i].
 * No byte outside the listed segments is read, and no entry of d_segs /
 * d_seg_pos past a message's listed ones, so the caller may be appending
 * there.  States, d_totals, d_digests / d_expected / d_ok, null handling and
 * the bound on n are exactly bt_sha1_resume_dev's; data and tables may be
 * device or pinned host memory.
 * The library exports this function as bt_sha1_dgram_chain_dev (its export
 * lists close the gather_ and resume_ name families at the functions above);
 * bt_sha1_gather_resume_dev is the same call under the name it is known by. */
int bt_sha1_dgram_chain_dev(const void *d_base, const bt_sha1_seg *d_segs, const uint64_t *d_seg_pos,
                            const uint64_t *d_seg_first, const uint32_t *d_seg_count,
                            const uint64_t *d_from, const uint32_t *d_lens, const uint64_t *d_totals,
                            uint64_t n, uint32_t *d_states, uint8_t *d_digests /* may be NULL */,
                            const uint8_t *d_expected, uint8_t *d_ok, void *stream);
static inline int bt_sha1_gather_resume_dev(const void *d_base, const bt_sha1_seg *d_segs,
                                            const uint64_t *d_seg_pos, const uint64_t *d_seg_first,
                                            const uint32_t *d_seg_count, const uint64_t *d_from,
                                            const uint32_t *d_lens, const uint64_t *d_totals, uint64_t n,
                                            uint32_t *d_states, uint8_t *d_digests /* may be NULL */,
                                            const uint8_t *d_expected, uint8_t *d_ok, void *stream) {
  return bt_sha1_dgram_chain_dev(d_base, d_segs, d_seg_pos, d_seg_first, d_seg_count, d_from, d_lens, d_totals, n,
                                 d_states, d_digests, d_expected, d_ok, stream);
}
/* Frozen generator: 64-bit word g of the stream = splitmix64(seed + g), LE.
 * Writes words first_word .. into d_buf (16-byte aligned), nbytes bytes. */
int bt_sha1_fill_synthetic(void *d_buf, uint64_t nbytes, uint64_t first_word, uint64_t seed,
                           void *stream);

/* ---- host batches (H2D -> kernel -> D2H, double-buffered pinned staging) - */
/* Page-lock a caller buffer (e.g. an mmap'ed file or a receive ring) so the
 * host batch calls DMA from it directly instead of copying into staging. */
int bt_sha1_host_register(void *h_ptr, uint64_t len);
int bt_sha1_host_unregister(void *h_ptr);
/* make_chunks over a memory image: chunk i = h_in[i*chunk_len ..], the last
 * one may be short.  Returns the chunk count (ceil(total_len/chunk_len)).
 * Memory kept between calls: each device's context keeps its two staging
 * lanes, grown on demand and reused by later calls -- up to 2 x 1 GiB of
 * page-locked host memory (pageable input) and 2 x 1 GiB of HBM.  Pinned or
 * registered input is DMA'd straight from the caller's memory into the same
 * HBM lanes (1 GiB batches).  With BT_SHA1_DMA_BATCH_MB above 1024 the
 * direct-DMA batches are bigger; before the call returns each oversized lane
 * is freed and re-allocated at the size it had before the call (at most the
 * 1 GiB kept lane), so the call leaves exactly the kept lanes allocated.
 * Freeing (hipFree) synchronises the whole device, so such a call returns
 * only after work other streams of this process queued on the GPU has
 * finished. */
int64_t bt_sha1_chunks_host(const void *h_in, uint64_t total_len, uint64_t chunk_len,
                            uint8_t *h_digests);
/* The same split over the first `ndev` GPUs (<=0: all), one host thread per
 * device, contiguous chunk ranges, digests gathered into h_digests in order. */
int64_t bt_sha1_chunks_host_multi(const void *h_in, uint64_t total_len, uint64_t chunk_len,
                                  uint8_t *h_digests, int ndev);
/* The same split over an explicit list of nworkers device ids (SURVEY.md §8e:
 * worker g takes chunks [g*n/G, (g+1)*n/G)).  An id may repeat: each repeat
 * is an independent worker (own host thread, streams and staging) on that
 * device, so the multi-GPU split / staging / ordered gather can be run with
 * any worker count on one GPU.  The first use of a device works in its shared
 * context (kept, as above); the repeats' contexts are freed before the call
 * returns.  At most 64 workers.  Returns the chunk count. */
int64_t bt_sha1_chunks_host_devices(const void *h_in, uint64_t total_len, uint64_t chunk_len,
                                    uint8_t *h_digests, const int *devs, int nworkers);
/* make_chunks over a FILE* with an explicit chunk size (make_chunks uses
 * BT_CHUNK_SIZE).  h_digests must hold 20*ceil(size/chunk_len) bytes. */
int64_t bt_sha1_chunks_file(void *fp /* FILE* */, uint64_t chunk_len, uint8_t *h_digests,
                            uint64_t max_chunks);

/* Where the time of the calling thread's last host pipeline run went
 * (bt_sha1_chunks_host, bt_sha1_chunks_file, make_chunks; for the multi-GPU
 * split, the last worker's run on its own thread), and where its memory sat.
 * The pipeline stages each batch on the host (fill: threaded memcpy / pread
 * into the page-locked staging lanes, or nothing for DMA straight from
 * pinned input), queues its H2D and hash on the lane's stream, and blocks
 * (wait) only when a lane is needed again or at the end.  fill_s close to
 * total_s means the host staging sets the rate; wait_s close to total_s
 * means PCIe / the GPU do.  NUMA fields (Linux sysfs + move_pages): the
 * GPU's node, sampled pages of the staging lanes and of the caller's input
 * per node, and the staging pieces by the node of the CPU their thread ran
 * on; -1 / zeros where unknown.  numa_policy (BT_SHA1_NUMA, applied only
 * when the machine has more than one node and the GPU's node is known):
 * 0 = "off" (pages where the kernel puts them), 1 = "lanes" (the default:
 * the staging lanes and the verifier's receive slots prefer the GPU's
 * node), 2 = "gpu" (that, and the staging threads run on the node's CPUs
 * within the caller's affinity mask -- measured 15-30 % slower on a shared
 * host, where the node's cores are busy with other work: DESIGN.md §6).
 * Pageable input of at least 64 MiB to bt_sha1_chunks_host is page-locked
 * batch by batch (the whole pages of each ~1 GiB batch, all locked before the
 * first copy and released when the call's last batch is done) and DMA'd in
 * place; the unaligned head
 * and tail bytes of each batch, and pages that cannot be locked, are staged
 * (BT_SHA1_PAGEABLE=stage: stage everything).  The last ~batch of chunks of
 * a bt_sha1_chunks_host input (at least 256 MiB of them, chunks of at least
 * 64 KiB; BT_SHA1_COLUMN_MIN_MB) is copied in columns -- 8 strided copies of
 * chunk_len/8 bytes of every chunk (BT_SHA1_COLUMNS: 2..16, 0 = off), for the
 * staged feed gathered into the staging lane by the copy threads -- each
 * hashed into the chunks' chaining state as soon as it has arrived, so the
 * call ends one column's hash, not one whole chunk's, after its last byte
 * crossed PCIe.
 * Returns 0, or -1 when this thread has run no pipeline. */
/* How bt_sha1_chunks_host feeds pageable input of at least 64 MiB to the
 * GPU: page-locked batch by batch and DMA'd in place (REGISTER, the default)
 * or copied into the pinned staging lanes (STAGE; also BT_SHA1_PAGEABLE=stage
 * in the environment).  Process-wide; returns the previous setting or -1. */
#define BT_SHA1_PAGEABLE_REGISTER 0
#define BT_SHA1_PAGEABLE_STAGE 1
int bt_sha1_set_pageable_feed(int feed);
#define BT_SHA1_STATS_NODES 8
typedef struct {
  uint64_t chunks;          /* digests produced                               */
  uint64_t bytes;           /* input bytes                                    */
  uint64_t batch_bytes;     /* bytes per lane batch                           */
  uint32_t batches;         /* lane batches launched                          */
  int32_t staged;           /* 1: copied into the lanes; 0: direct DMA from
                               pinned input; 2: pageable input page-locked
                               batch by batch and DMA'd in place             */
  int32_t device;           /* HIP device                                     */
  int32_t copy_threads;     /* staging threads per piece (BT_SHA1_COPY_THREADS) */
  int32_t numa_nodes;       /* NUMA nodes of the machine (sysfs)              */
  int32_t gpu_numa_node;    /* the GPU's node (-1: unknown)                   */
  int32_t numa_policy;      /* 0 none, 1 lanes, 2 lanes + threads (see above) */
  int32_t registered_batches; /* batches DMA'd from caller pages locked for them */
  uint32_t column_chunks;   /* last chunks copied and hashed column by column
                               (bt_sha1_chunks_host; see above)              */
  double total_s;           /* the whole call                                 */
  double alloc_s;           /* lane allocation / page-locking in the call     */
  double fill_s;            /* providing the input on the host: staging copies
                               / reads, or registering the batch's pages      */
  double wait_s;            /* blocked on a lane's H2D + hash                 */
  double register_s;        /* page-locking caller pages before the first copy
                               (in total_s)                                   */
  double unregister_s;      /* releasing them after the last batch (in total_s) */
  int32_t lane_pages[BT_SHA1_STATS_NODES];  /* sampled staging pages per node */
  int32_t src_pages[BT_SHA1_STATS_NODES];   /* sampled input pages per node   */
  int32_t copy_pieces[BT_SHA1_STATS_NODES]; /* staging pieces per CPU node    */
} bt_sha1_pipeline_stats;
int bt_sha1_get_pipeline_stats(bt_sha1_pipeline_stats *out);

/* ---- batched asynchronous verify (replaces util.c:304-337's hash+memcmp) -- */
typedef struct bt_sha1_verifier bt_sha1_verifier;
typedef struct {
  uint64_t tag;                       /* caller's tag (e.g. chunk id)        */
  int32_t ok;                         /* 1: digest == expected, 0: mismatch  */
  uint8_t digest[BT_SHA1_DIGEST_SIZE]; /* computed digest                    */
} bt_sha1_verdict;

/* batch: chunks per GPU launch; nstreams: batches in flight (>=2 overlaps
 * H2D of batch k+1 with hashing of batch k); chunk_len: BT_CHUNK_SIZE. */
bt_sha1_verifier *bt_sha1_verifier_create(int device, uint32_t chunk_len, uint32_t batch,
                                          uint32_t nstreams);
/* A verifier for chunks of ANY length from 1 to max_chunk_len (1 .. 32 MiB, any
 * value): a file's short last chunk (the last fread of make_chunks,
 * chunk.c:20) is committed at its own length, like the receiver and the intake
 * take it.  Slots lie at a pitch of max_chunk_len rounded up to 16 bytes.  A
 * batch whose committed chunks are all max_chunk_len long, with max_chunk_len a
 * 16-byte multiple, launches exactly what the verifier above launches (the hot
 * kernel, or the column split); any other batch is copied the same way and
 * hashed by one launch of the ragged kernels with the compare fused (as
 * bt_sha1_ragged_verify_dev; no column split).  NULL with a message for
 * arguments out of range, before any device call.  Everything below works on
 * both kinds; a verifier from bt_sha1_verifier_create still refuses any len
 * but chunk_len. */
bt_sha1_verifier *bt_sha1_verifier_create_ragged(int device, uint32_t max_chunk_len, uint32_t batch,
                                                 uint32_t nstreams);
void bt_sha1_verifier_destroy(bt_sha1_verifier *v);
/* Zero-copy: hand out a pinned chunk_len-byte slot to assemble one chunk in
 * (e.g. save_data_packet's memcpy target, util.c:275).  Several slots may be
 * outstanding (one per in-progress download); blocks only when the ring must
 * wrap onto a batch still in flight.  NULL on error. */
uint8_t *bt_sha1_verifier_slot(bt_sha1_verifier *v);
/* Queue an outstanding slot for verification against expected[20].  len is
 * chunk_len; for a ragged verifier, the chunk's own length, 1 .. max_chunk_len. */
int bt_sha1_verifier_commit(bt_sha1_verifier *v, uint8_t *slot, uint32_t len,
                            const uint8_t expected[20], uint64_t tag);
/* Give an outstanding slot back unverified (aborted download); no verdict. */
int bt_sha1_verifier_release(bt_sha1_verifier *v, uint8_t *slot);
/* Copying form: slot + memcpy + commit. */
int bt_sha1_verifier_submit(bt_sha1_verifier *v, const void *h_chunk, uint32_t len,
                            const uint8_t expected[20], uint64_t tag);
/* Close the batch being filled; it launches once its outstanding slots are settled. */
int bt_sha1_verifier_flush(bt_sha1_verifier *v);
/* Non-blocking: copy up to max finished verdicts out; returns the count. */
int bt_sha1_verifier_poll(bt_sha1_verifier *v, bt_sha1_verdict *out, int max);
/* Blocking: flush, wait for everything in flight, return up to max verdicts. */
int bt_sha1_verifier_drain(bt_sha1_verifier *v, bt_sha1_verdict *out, int max);
/* Verdicts not yet returned (in flight + finished-unpolled). */
int64_t bt_sha1_verifier_pending(bt_sha1_verifier *v);
typedef struct {
  uint64_t batches;         /* batches launched                               */
  uint64_t ragged_batches;  /* of them, through the ragged kernels: a short
                               chunk in the batch, or max_chunk_len not a
                               16-byte multiple (always 0 for a verifier from
                               bt_sha1_verifier_create)                       */
  uint64_t chunks;          /* chunks committed                               */
  uint64_t short_chunks;    /* of them, shorter than max_chunk_len            */
  uint64_t released;        /* slots released                                 */
} bt_sha1_verifier_stats;
int bt_sha1_verifier_get_stats(bt_sha1_verifier *v, bt_sha1_verifier_stats *out);
/* A verifier whose slots hold DATAGRAMS, not an assembled chunk: recvfrom /
 * recvmmsg land whole packets (header and payload) anywhere in the slot, in
 * arrival order, and commit_gather lists the payloads in sequence order; a
 * retransmitted duplicate is simply not listed.  slot_len: 1 .. 33 MiB (354 x
 * 1500 = 531,000 bytes for the reference's chunk; the pitch is slot_len
 * rounded up to 16); max_segs >= 1: segments per chunk at most, with batch x
 * max_segs x 16 bytes of pinned table at most 256 MiB.  NULL with a message
 * for arguments out of range, before any device call.  Every batch is one
 * copy of its slots as they are and ONE gather-verify launch (as
 * bt_sha1_gather_verify_dev; tables, expected hashes, verdicts and digests in
 * pinned memory in place; no column split).
 * commit_gather: segs[k].off is relative to the slot.  nseg > max_segs, or a
 * segment with off + len > slot_len, is -1 with a message: the slot stays
 * outstanding, nothing is recorded, the verifier stays usable.  Refused on
 * any other kind of verifier.
 * bt_sha1_verifier_commit on such a verifier is the one-segment message
 * (0, len), 1 <= len <= slot_len; everything else works unchanged. */
bt_sha1_verifier *bt_sha1_verifier_create_gather(int device, uint32_t slot_len, uint32_t max_segs,
                                                 uint32_t batch, uint32_t nstreams);
int bt_sha1_verifier_commit_gather(bt_sha1_verifier *v, uint8_t *slot, const bt_sha1_seg *segs,
                                   uint32_t nseg, const uint8_t expected[20], uint64_t tag);
typedef struct {
  uint64_t gather_batches;  /* batches launched through the gather kernel     */
  uint64_t gather_chunks;   /* chunks committed to them                       */
  uint64_t segments;        /* segments listed by those commits               */
  uint64_t payload_bytes;   /* bytes hashed: the sum of the segment lengths   */
  uint64_t copied_bytes;    /* bytes copied to the device: reserved x pitch   */
} bt_sha1_verifier_gather_stats;
int bt_sha1_verifier_get_gather_stats(bt_sha1_verifier *v, bt_sha1_verifier_gather_stats *out);

/* ---- progressive receive (util.c:250-337 for in-order delivery) ---------- */
/* The verifier above starts a chunk's serial chain when its last byte has
 * arrived (~6 ms per 512 KiB).  The receiver hashes a chunk WHILE it is
 * received: the GPU advances each in-progress chunk's chaining state over the
 * prefix that has arrived (the resumable chain kernel reads the pinned slot
 * in place over PCIe, no H2D copy), so commit leaves only the last stride and
 * the padding.  One thread per object, like the verifier.
 * nslots: chunks in flight (the peer's max_conn), 1..64; chunk_len: 1 .. 32
 * MiB; stride: bytes of new whole blocks that trigger a launch (0 = 64 KiB;
 * UINT32_MAX = never before commit).  NULL with a message for arguments out
 * of range, before any device call. */
typedef struct bt_sha1_receiver bt_sha1_receiver;
bt_sha1_receiver *bt_sha1_receiver_create(int device, uint32_t chunk_len, uint32_t nslots,
                                          uint32_t stride);
void bt_sha1_receiver_destroy(bt_sha1_receiver *r);
/* A pinned chunk_len-byte slot to receive one chunk into, in order
 * (save_data_packet's memcpy target, util.c:275); its chaining state starts
 * from the IV.  NULL with a message when all nslots are out. */
uint8_t *bt_sha1_receiver_slot(bt_sha1_receiver *r);
/* Bytes [0, filled) of the slot are final (received_byte_number): `filled`
 * never decreases and is at most chunk_len.  Once the whole blocks not yet
 * hashed reach `stride` bytes, ONE launch over them is queued; returns
 * without waiting. */
int bt_sha1_receiver_advance(bt_sha1_receiver *r, uint8_t *slot, uint32_t filled);
/* The chunk is complete at len bytes (hashed so far <= len <= chunk_len,
 * len > 0; a short last chunk is fine): queues the finishing launch over the
 * rest with the compare against expected[20] fused, and returns without
 * waiting.  The verdict arrives through poll / drain; the slot is free again
 * once its verdict has been returned. */
int bt_sha1_receiver_commit(bt_sha1_receiver *r, uint8_t *slot, uint32_t len,
                            const uint8_t expected[20], uint64_t tag);
/* Give an outstanding slot back (aborted download): waits for its queued
 * launches; no verdict.  The slot restarts from the IV when handed out again. */
int bt_sha1_receiver_release(bt_sha1_receiver *r, uint8_t *slot);
/* Non-blocking: reads the kernels' completion words (no stream wait) and
 * copies up to max finished verdicts out, in the order they were found
 * finished; returns the count. */
int bt_sha1_receiver_poll(bt_sha1_receiver *r, bt_sha1_verdict *out, int max);
/* Blocking: waits for everything committed, returns up to max verdicts; -1 if
 * a launch failed. */
int bt_sha1_receiver_drain(bt_sha1_receiver *r, bt_sha1_verdict *out, int max);
/* Verdicts not yet returned (in flight + finished-unpolled). */
int64_t bt_sha1_receiver_pending(bt_sha1_receiver *r);
typedef struct {
  uint64_t launches;          /* kernel launches queued (advances + commits)  */
  uint64_t advance_launches;  /* of them, queued by advance                   */
  uint64_t advanced_bytes;    /* bytes hashed before their chunk's commit     */
  uint64_t committed;         /* chunks committed                             */
  uint64_t released;          /* slots released                               */
} bt_sha1_receiver_stats;
int bt_sha1_receiver_get_stats(bt_sha1_receiver *r, bt_sha1_receiver_stats *out);

/* ---- progressive receive for many chunks at once --------------------------- */
/* The receiver above queues one single-workgroup launch per slot per stride,
 * so only a handful of chains advance at a time.  The intake has the same slot
 * life cycle for up to 512 chunks in flight, but advance and commit only
 * RECORD what has arrived: kick (or poll, which ends with a kick) advances
 * every slot that is due in ONE launch of the table-driven resumable chain
 * kernel, one two-wave workgroup per slot.  An event loop calls advance per
 * payload and poll once per turn.  One thread per object.
 * nslots: 1..512; chunk_len: 1 .. 32 MiB, and nslots x chunk_len (padded to 64
 * bytes) at most 2 GiB of pinned memory; stride as in the receiver (0 = 64
 * KiB; UINT32_MAX = nothing before commit).  NULL with a message for arguments
 * out of range, before any device call. */
typedef struct bt_sha1_intake bt_sha1_intake;
typedef struct {
  uint64_t kicks;           /* calls to kick (poll's and drain's included)    */
  uint64_t launches;        /* launches queued                                */
  uint64_t entries;         /* table entries queued in total                  */
  uint64_t max_entries;     /* largest single launch                          */
  uint64_t advanced_bytes;  /* bytes hashed before their chunk's commit       */
  uint64_t committed;       /* chunks committed                               */
  uint64_t released;        /* slots released                                 */
  uint64_t deferred;        /* due slots a kick skipped because their previous
                               launch was still in flight                     */
} bt_sha1_intake_stats;
bt_sha1_intake *bt_sha1_intake_create(int device, uint32_t chunk_len, uint32_t nslots,
                                      uint32_t stride);
void bt_sha1_intake_destroy(bt_sha1_intake *r);
/* As bt_sha1_receiver_slot. */
uint8_t *bt_sha1_intake_slot(bt_sha1_intake *r);
/* Bytes [0, filled) of the slot are final; validated as the receiver does.
 * Records only: once the whole blocks not yet hashed reach `stride` bytes the
 * slot is due for the next kick. */
int bt_sha1_intake_advance(bt_sha1_intake *r, uint8_t *slot, uint32_t filled);
/* The chunk is complete at len bytes (hashed so far <= len <= chunk_len,
 * len > 0).  Records only: the slot is due, and the next kick that finds it
 * without a launch in flight queues ONE finishing entry over everything not
 * yet hashed, with the compare against expected[20] fused. */
int bt_sha1_intake_commit(bt_sha1_intake *r, uint8_t *slot, uint32_t len,
                          const uint8_t expected[20], uint64_t tag);
/* Give an outstanding slot back (aborted download): drops a span that was due
 * but not launched, waits only for a launch in flight on this slot. */
int bt_sha1_intake_release(bt_sha1_intake *r, uint8_t *slot);
/* One launch for every due slot that has no launch in flight; a due slot
 * whose previous launch has not finished stays due for a later kick.  Returns
 * the entries launched (0: nothing due), -1 on error.  Does not wait, unless
 * all of its eight launch tables are still in use (then for the oldest). */
int bt_sha1_intake_kick(bt_sha1_intake *r);
/* Wait for every queued launch; launches nothing. */
int bt_sha1_intake_sync(bt_sha1_intake *r);
/* Non-blocking: harvests finished chunks from the completion words (no stream
 * wait), then kicks; copies up to max verdicts out and returns the count. */
int bt_sha1_intake_poll(bt_sha1_intake *r, bt_sha1_verdict *out, int max);
/* Blocking: kicks and waits until nothing committed is unfinished, returns up
 * to max verdicts; -1 if a launch failed. */
int bt_sha1_intake_drain(bt_sha1_intake *r, bt_sha1_verdict *out, int max);
/* Verdicts not yet returned (recorded + in flight + finished-unpolled). */
int64_t bt_sha1_intake_pending(bt_sha1_intake *r);
int bt_sha1_intake_get_stats(bt_sha1_intake *r, bt_sha1_intake_stats *out);
/* A GATHER intake: the same object and life cycle, but a slot holds DATAGRAMS
 * where recvfrom / recvmmsg put them (as the gather verifier's slots), and the
 * chunk is hashed in place over the in-sequence prefix of payloads that has
 * arrived: no memcpy into place (util.c:275), and at commit only the last
 * stride and the padding are left.  kick launches the table-driven chain-form
 * gather kernel; the eight-table ring, the four streams and `deferred` are as
 * above, and slot, release, kick, sync, poll, drain, pending and get_stats work
 * unchanged.  A slot's segment list is empty, and its state the IV, whenever it
 * is handed out.
 * create_gather: slot_len 1 .. 33 MiB (the pitch is slot_len rounded up to 16);
 *   max_segs >= 1 segments per chunk at most; nslots 1..512; nslots x pitch at
 *   most 2 GiB and nslots x max_segs x 24 bytes of pinned segment tables at
 *   most 256 MiB; stride as above.  NULL with a message for arguments out of
 *   range, before any device call.
 * append: the NEXT nseg payload segments in sequence order (off relative to
 *   the slot): the caller holds an out-of-order datagram back until the gap
 *   before it is filled, and never lists a duplicate.  Records only; the slot
 *   is due once the listed whole blocks not yet hashed reach `stride`.  More
 *   than max_segs segments in total, a segment with off + len > slot_len, or a
 *   running total above 32 MiB, is -1 with a message: nothing is recorded and
 *   the intake stays usable.  Legal while a launch on the slot is in flight
 *   (entries carry the segment count of kick time; the kernel reads no
 *   descriptor at or past it).
 * commit_gather: the chunk is complete at the bytes listed (more than 0): the
 *   next kick that finds the slot without a launch in flight queues ONE
 *   finishing entry over everything not yet hashed, the compare fused.
 * bt_sha1_intake_advance / _commit are refused on a gather intake, append /
 * commit_gather on a plain one, with a message.
 * The library exports the three as bt_sha1_dgram_slots_create / _append /
 * _commit (its export lists close the intake_ name family at the functions
 * above); the bt_sha1_intake_ names below are the same calls. */
bt_sha1_intake *bt_sha1_dgram_slots_create(int device, uint32_t slot_len, uint32_t max_segs,
                                           uint32_t nslots, uint32_t stride);
int bt_sha1_dgram_slots_append(bt_sha1_intake *r, uint8_t *slot, const bt_sha1_seg *segs,
                               uint32_t nseg);
int bt_sha1_dgram_slots_commit(bt_sha1_intake *r, uint8_t *slot, const uint8_t expected[20],
                               uint64_t tag);
static inline bt_sha1_intake *bt_sha1_intake_create_gather(int device, uint32_t slot_len,
                                                           uint32_t max_segs, uint32_t nslots,
                                                           uint32_t stride) {
  return bt_sha1_dgram_slots_create(device, slot_len, max_segs, nslots, stride);
}
static inline int bt_sha1_intake_append(bt_sha1_intake *r, uint8_t *slot, const bt_sha1_seg *segs,
                                        uint32_t nseg) {
  return bt_sha1_dgram_slots_append(r, slot, segs, nseg);
}
static inline int bt_sha1_intake_commit_gather(bt_sha1_intake *r, uint8_t *slot,
                                               const uint8_t expected[20], uint64_t tag) {
  return bt_sha1_dgram_slots_commit(r, slot, expected, tag);
}

/* ---- digest lookup (get_chunk_id / find_chunk, util.c:3-39, on the GPU) - */
/* d_index[q] = smallest i with digest d_table[i] == d_queries[q], else -1.
 * Builds a transient open-addressing table in HBM (stream-ordered alloc):
 * a power of two of at least 2 * n_table 32-bit slots, at least 1024.
 * n_table is at most 2^30 (the slot count is a uint32_t: 2^31 slots, 8 GiB);
 * a larger table is refused with -1 and "lookup table too large" before any
 * device call.  Both digest arrays are 4-byte aligned. */
int bt_sha1_lookup_dev(const uint8_t *d_table, uint64_t n_table, const uint8_t *d_queries,
                       uint64_t n_queries, int64_t *d_index, void *stream);

/* ---- .chunks files (host-side text formats around the hash) ------------ */
typedef struct {
  int32_t id;                          /* chunk id as written in the file     */
  uint8_t hash[BT_SHA1_DIGEST_SIZE];   /* binary digest                       */
} bt_chunk_entry;

/* "<id> <40 hex>" lines (has/get files; parse_has_get_chunk_file,
 * util.c:64-111).  *out is malloc'ed (bt_chunks_free).  Returns the count or
 * -1 (bt_chunks_last_error()).  '#' and blank lines are skipped; malformed
 * lines are errors (the reference silently stores garbage). */
int64_t bt_chunks_parse_list(const char *path, bt_chunk_entry **out);
/* Master file: "File: <data file>" / "Chunks:" header then list lines
 * (parse_total_chunk_file, util.c:113-164; peer.c:299-305). */
int64_t bt_chunks_parse_master(const char *path, char *data_file, size_t data_file_cap,
                               bt_chunk_entry **out);
void bt_chunks_free(bt_chunk_entry *entries);
/* Write n digests as make-chunks does ("%d %s\n", make_chunks.c:49-53), ids
 * from first_id; with a master header first when master_data_file != NULL. */
int bt_chunks_write(void *fp /* FILE* */, const char *master_data_file, const uint8_t *digests,
                    int64_t n, int32_t first_id);
/* hex2binary (chunk.c:66-83) that rejects non-hex input: 0 or -1. */
int bt_hex2binary_checked(const char *hex, int len, uint8_t *buf);
const char *bt_chunks_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* BT_SHA1_H */
