// sha1_launch.h -- internal launcher interface between the kernels
// (sha1_kernels.hip) and the host runtime (bt_*.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// n equal chunks of `len` bytes at `pitch` (16-byte multiple, 64*pitch < 4 GiB),
// d_in 16-byte aligned.  d_dig: 20*n bytes (4-byte aligned) or NULL.  When
// d_ok != NULL also compares against d_exp (20*n) and writes one byte per chunk.
// tail_len (0 < tail_len < len, no d_ok): one more chunk of tail_len bytes at
// d_in + n*pitch, digest at d_dig + 20*n, hashed in the same launch.
hipError_t btsha1_launch_fixed(const void *d_in, uint64_t n, uint32_t pitch, uint32_t len, uint8_t *d_dig,
                               const uint8_t *d_exp, uint8_t *d_ok, hipStream_t s, int variant,
                               uint32_t tail_len = 0);
// Diagnostic build of the hot kernel (variant as above, no verify, no tail):
// lane 0 of every wave writes {s_memtime, s_memrealtime} at the start of its
// loop and after it to d_stamps[4*wave ..] (4 u64 per wave of 64 chunks).
hipError_t btsha1_launch_fixed_stamped(const void *d_in, uint64_t n, uint32_t pitch, uint32_t len, uint8_t *d_dig,
                                       uint64_t *d_stamps, hipStream_t s, int variant);
// Name of the kernel btsha1_launch_fixed runs for a batch of n chunks (tail
// included) on the current device with this variant.
const char *btsha1_fixed_kernel_name(uint64_t n, int variant);
// Batches of at most max_chunks chunks (tail included) take the latency kernel
// k_sha1_lat instead of the selected variant; 0 disables it.  The default,
// BT_SHA1_LATENCY_AUTO, is 128 chunks per CU of the launching device (at
// most two two-wave workgroups per CU; past that the latency kernel loses to
// the hot kernel).
#define BT_SHA1_LATENCY_AUTO UINT64_MAX
void btsha1_set_latency_batch(uint64_t max_chunks);
uint64_t btsha1_latency_batch_setting();  // raw setting (may be BT_SHA1_LATENCY_AUTO)
uint64_t btsha1_latency_batch();          // effective threshold on the current device
#define BT_SHA1_CHAIN_AUTO UINT64_MAX  // = 2 x CUs of the launching device
void btsha1_set_chain_batch(uint64_t max_messages);
uint64_t btsha1_chain_batch_setting();
uint64_t btsha1_chain_batch();
// Compute units of the current device (cached per device; 256 on MI355X).
uint32_t btsha1_device_cus();
// Hot-kernel variant code = ring slots*100 + lines per slot*10 + nt flag.
// The product build knows only 310; the experiments build
// (-DBT_SHA1_EXPERIMENTS) also the rejected ring / nt / LDS-staged variants.
bool btsha1_fixed_variant_ok(int code);
bool btsha1_experiments_build();
// n messages at d_base + d_off[i], d_len[i] bytes each; with d_off == NULL,
// message i is at d_base + i*pitch, fixed_len bytes.  Any alignment.  At most
// btsha1_chain_batch() messages take the chain kernel, more the one-message-
// per-lane ragged kernel.
hipError_t btsha1_launch_ragged(const void *d_base, const uint64_t *d_off, const uint32_t *d_len, uint64_t pitch,
                                uint32_t fixed_len, uint64_t n, uint8_t *d_dig, hipStream_t s);
// Chain kernel (one message per two-wave workgroup; lowest single-chain
// latency).  state / data may be device or pinned host memory.
// done != NULL: after the results, *done = seq is stored with a system-scope
// release, so a host can spin on it instead of waiting on the stream.
hipError_t btsha1_launch_chain_midstate(uint32_t *state, const void *data, uint64_t nblocks, hipStream_t s,
                                        uint32_t *done = nullptr, uint32_t seq = 0);
// One message of len bytes at msg (device or pinned host memory), digest to digest.
hipError_t btsha1_launch_chain_one(const void *msg, uint64_t len, uint8_t *digest, hipStream_t s,
                                   uint32_t *done = nullptr, uint32_t seq = 0);
// n messages: message i at base + (offsets ? offsets[i] : i*pitch), length
// lens ? lens[i] : fixed_len; digest i (big-endian bytes) at digests + 20*i
// (digests may be NULL with ok).  tail_len != 0 (no offsets): one more message
// of tail_len bytes at base + n*pitch.  ok != NULL (no offsets, no tail):
// ok[i] = digest i == expected[20*i ..] (util.c:313).
hipError_t btsha1_launch_chain(const void *base, const uint64_t *offsets, const uint32_t *lens, uint64_t pitch,
                               uint64_t fixed_len, uint64_t n, uint8_t *digests, hipStream_t s, uint64_t tail_len = 0,
                               const uint8_t *expected = nullptr, uint8_t *ok = nullptr);
// Resumable chain kernel (k_sha1_resume; one two-wave workgroup per message):
// message i's next lens[i] bytes at base + offsets[i] (any alignment, device or
// pinned host memory; nothing at or past offsets[i] + lens[i] is read), its
// chaining state at states[5*i ..] (SHA1Context.hash order, device or pinned
// host memory).  totals[i] == 0 advances the state over the lens[i] >> 6 whole
// blocks; totals[i] != 0 finishes a totals[i]-byte message whose first
// totals[i] - lens[i] bytes (a 64-byte multiple) were advanced before: digest
// i (big-endian, any alignment) to digests + 20*i when digests != NULL, and
// with ok (needs expected) ok[i] = digest i == expected[20*i ..]; entries of
// advancing messages are left alone.  done != NULL (n == 1 only): the
// completion word of btsha1_launch_chain_midstate.  At most BTSHA1_RESUME_MAX
// messages per launch (the grid).  New launchers are hidden: shared between
// the library's objects, absent from its dynamic symbols.
#define BTSHA1_RESUME_MAX 0x7fffffffull
#define BTSHA1_HIDDEN __attribute__((visibility("hidden")))
BTSHA1_HIDDEN hipError_t btsha1_launch_resume(const void *base, const uint64_t *offsets, const uint32_t *lens,
                                              const uint64_t *totals, uint64_t n, uint32_t *states, uint8_t *digests,
                                              const uint8_t *expected, uint8_t *ok, hipStream_t s,
                                              uint32_t *done = nullptr, uint32_t seq = 0);
// btsha1_launch_ragged with the fused compare (k_sha1_chain<false, true>,
// k_sha1_lat_ragged_verify<2 / 3>, k_sha1_ragged_verify: the same choice by n,
// under the same two settings): d_ok[i] = digest i == d_exp[20*i ..]
// (util.c:313) for i < n.  d_exp, d_ok and d_dig take any alignment and may be
// device or pinned host memory; d_dig may be NULL.  d_off and d_len come
// together or not at all.  hipErrorInvalidValue and no launch for a null
// d_base, d_exp or d_ok, one of d_off / d_len without the other, or n above
// BTSHA1_RAGGED_VERIFY_MAX (the grid of the one-workgroup-per-message form).
#define BTSHA1_RAGGED_VERIFY_MAX 0x7fffffffull
BTSHA1_HIDDEN hipError_t btsha1_launch_ragged_verify(const void *d_base, const uint64_t *d_off, const uint32_t *d_len,
                                                     uint64_t pitch, uint32_t fixed_len, uint64_t n, uint8_t *d_dig,
                                                     const uint8_t *d_exp, uint8_t *d_ok, hipStream_t s);
// Scatter-gather (k_sha1_gather / k_sha1_gather_verify, one message per lane):
// message i is the concatenation, in list order, of the seg_count[i] segments
// segs[seg_first[i] ..] (bt_sha1_seg: {u64 off; u32 len; u32 reserved}), each
// base[off .. off + len), any alignment and length, in any address order,
// shared or overlapping between messages; no byte outside them is read.  base
// and the tables may be device or pinned host memory.  dig / exp / ok as
// btsha1_launch_ragged_verify's (ok == NULL: digests only).
// hipErrorInvalidValue and no launch for a null base, segs, seg_first or
// seg_count, ok without exp, or n above BTSHA1_GATHER_MAX (the grid of its
// 64-thread form).
#define BTSHA1_GATHER_MAX (0x7fffffffull * 64ull)
BTSHA1_HIDDEN hipError_t btsha1_launch_gather(const void *base, const void *segs, const uint64_t *seg_first,
                                              const uint32_t *seg_count, uint64_t n, uint8_t *dig, const uint8_t *exp,
                                              uint8_t *ok, hipStream_t s);
// Its latency form (k_sha1_gather_lat<2 / 3>: one two-wave workgroup per 64
// messages, three LDS slots when the grid exceeds the CU count, else two, as
// btsha1_launch_ragged chooses): the same arguments and results.
// hipErrorInvalidValue and no launch for a null base, segs, seg_first or
// seg_count, n == 0, ok without exp, neither ok nor dig, or a grid above
// 2^31 - 1.
// btsha1_launch_gather takes it for n <= btsha1_seglist_latency_batch():
// 0 (the default) never, BT_SHA1_SEGLIST_LATENCY_AUTO 128 x CUs of the
// launching device.
#define BT_SHA1_SEGLIST_LATENCY_AUTO UINT64_MAX
BTSHA1_HIDDEN hipError_t btsha1_launch_gather_lat(const void *base, const void *segs, const uint64_t *seg_first,
                                                  const uint32_t *seg_count, uint64_t n, uint8_t *dig,
                                                  const uint8_t *exp, uint8_t *ok, hipStream_t s);
BTSHA1_HIDDEN void btsha1_set_seglist_latency_batch(uint64_t max_messages);
BTSHA1_HIDDEN uint64_t btsha1_seglist_latency_batch_setting();
BTSHA1_HIDDEN uint64_t btsha1_seglist_latency_batch();
BTSHA1_HIDDEN const char *btsha1_seglist_kernel_name(uint64_t n);
// Its chain form (k_sha1_gather_chain: one two-wave workgroup per
// message, which builds the position table of the resumable form itself, a
// window of 1024 non-empty segments at a time in LDS): the same arguments and
// results.  `piece` caps the bytes of one pass over a window: a 64-byte
// multiple, at most BTSHA1_SEGCHAIN_PIECE, which is what production passes;
// the result does not depend on it.  hipErrorInvalidValue and no launch for a
// null base, segs, seg_first or seg_count, n == 0, ok without exp, neither ok
// nor dig, such a piece, or n above BTSHA1_RESUME_MAX (the grid).
// btsha1_launch_gather takes it, before the latency form, for
// n <= btsha1_segchain_batch(): 0 (the default) never, BT_SHA1_SEGCHAIN_AUTO
// 2 x CUs of the launching device (256 CUs where there is none).
#define BT_SHA1_SEGCHAIN_AUTO UINT64_MAX
#define BTSHA1_SEGCHAIN_PIECE (1u << 31)
BTSHA1_HIDDEN hipError_t btsha1_launch_gather_chain(const void *base, const void *segs, const uint64_t *seg_first,
                                                    const uint32_t *seg_count, uint64_t n, uint8_t *dig,
                                                    const uint8_t *exp, uint8_t *ok, uint32_t piece, hipStream_t s);
BTSHA1_HIDDEN void btsha1_set_segchain_batch(uint64_t max_messages);
BTSHA1_HIDDEN uint64_t btsha1_segchain_batch_setting();
BTSHA1_HIDDEN uint64_t btsha1_segchain_batch();
// Fixed-size packet buffers (k_sha1_pkts, one message per lane; the walk and
// its read contract are sha1_pkt_walk.h): message i is lens[i] bytes held in
// the slot at base + slot_off[i], sequence position k in packet buffer
// order[order_first[i] + k]; geom = {stride, header, payload, slot_pkts}
// (bt_sha1_pkt_geom).  dig / exp / ok as btsha1_launch_gather's, the compare
// chosen by ok != NULL.  Nothing is checked here: pkts_dev (bt_runtime.cpp),
// the one caller, refuses null arrays, n above BTSHA1_PKTS_MAX (the grid of
// the 64-thread form) and geometries outside the rule before it calls.
#define BTSHA1_PKTS_MAX (0x7fffffffull * 64ull)
BTSHA1_HIDDEN hipError_t btsha1_launch_pkts(const void *base, const uint32_t geom[4], const uint64_t *slot_off,
                                            const uint32_t *lens, const uint32_t *order,
                                            const uint64_t *order_first, uint64_t n, uint8_t *dig, const uint8_t *exp,
                                            uint8_t *ok, hipStream_t s);
// The single-message form (grid 1): offset, length and total are kernel
// arguments, so a host object launches it with no device-side arrays.
BTSHA1_HIDDEN hipError_t btsha1_launch_resume_one(const void *data, uint32_t len, uint64_t total, uint32_t *state,
                                                  uint8_t *digest, const uint8_t *expected, uint8_t *ok, hipStream_t s,
                                                  uint32_t *done = nullptr, uint32_t seq = 0);
// The table-driven form (k_sha1_resume_table; bt_intake.cpp): workgroup w
// serves entry w of `table` (pinned host memory, read with plain loads): bytes
// [from, from + len) of slot `slot` at slots + slot * pitch, the slot's
// 128-byte control block at ctl + slot * BTSHA1_TABLE_CTL (chaining state at
// bytes 0..19, expected hash 20..39, digest 64..83, verdict 84, completion
// word 88..91).  total == 0 advances the state over the len >> 6 whole blocks;
// total != 0 finishes a total-byte chunk whose first total - len bytes (a
// 64-byte multiple) were advanced before, writing the digest and, with verify,
// the verdict.  Either way `seq` is then stored into the slot's completion
// word with a system-scope release.  A slot may appear once per launch.
// hipErrorInvalidValue and no launch for n == 0, n > BTSHA1_TABLE_MAX or a
// null table, slot base or control base.
struct alignas(32) BtSha1TableEntry {
  uint32_t slot;
  uint32_t from, len;
  uint32_t total;  // 0: advance; else the chunk's length (at most 32 MiB)
  uint32_t seq;
  uint32_t pad[3];
};
static_assert(sizeof(BtSha1TableEntry) == 32 && alignof(BtSha1TableEntry) == 32, "table entry layout");
#define BTSHA1_TABLE_MAX 512u
#define BTSHA1_TABLE_CTL 128u
BTSHA1_HIDDEN hipError_t btsha1_launch_resume_table(const BtSha1TableEntry *table, uint32_t n, const uint8_t *slots,
                                                    uint64_t pitch, uint8_t *ctl, bool verify, hipStream_t s);
// Chain-form gather, resumable (k_sha1_gather_resume; one two-wave workgroup
// per message): message i's listed segments are segs[seg_first[i] .. +
// seg_count[i]) (bt_sha1_seg, as btsha1_launch_gather's), seg_pos parallel to
// segs (seg_pos[seg_first[i] + k] = the sum of the lengths of message i's
// segments before k).  Bytes [from[i], from[i] + lens[i]) of the message
// (from[i] a 64-byte multiple, the range inside the listed bytes) are hashed
// into states[5*i ..]; totals / digests / expected / ok as
// btsha1_launch_resume's.  No byte outside the listed segments and no table
// entry past a message's listed ones is read.  hipErrorInvalidValue and no
// launch for a null base or table, n == 0 or n above BTSHA1_RESUME_MAX (the
// grid), or ok without expected.
BTSHA1_HIDDEN hipError_t btsha1_launch_gather_resume(const void *base, const void *segs, const uint64_t *seg_pos,
                                                     const uint64_t *seg_first, const uint32_t *seg_count,
                                                     const uint64_t *from, const uint32_t *lens,
                                                     const uint64_t *totals, uint64_t n, uint32_t *states,
                                                     uint8_t *digests, const uint8_t *expected, uint8_t *ok,
                                                     hipStream_t s);
// Its table-driven form (k_sha1_gather_resume_table; the gather intake of
// bt_intake.cpp): workgroup w serves entry w of `table` (pinned host memory):
// message bytes [from, from + len) of slot `slot`, whose datagrams lie at
// slots + slot * pitch, whose descriptors at segs + slot * max_segs and their
// positions at seg_pos + slot * max_segs; nseg of them were listed when the
// entry was made and only those are read; seg_hint is the segment that holds
// `from`.  total, seq and the control block at ctl + slot * BTSHA1_TABLE_CTL
// are btsha1_launch_resume_table's.  hipErrorInvalidValue and no launch for
// n == 0, n > BTSHA1_TABLE_MAX, max_segs == 0 or a null base.
struct alignas(32) BtSha1GatherEntry {
  uint32_t slot;
  uint32_t from, len;
  uint32_t total;     // 0: advance; else the chunk's length (at most 32 MiB)
  uint32_t seq;
  uint32_t nseg;      // segments listed at kick time
  uint32_t seg_hint;  // the segment that holds `from`
  uint32_t pad;
};
static_assert(sizeof(BtSha1GatherEntry) == 32 && alignof(BtSha1GatherEntry) == 32, "gather table entry layout");
BTSHA1_HIDDEN hipError_t btsha1_launch_gather_resume_table(const BtSha1GatherEntry *table, uint32_t n,
                                                           const uint8_t *slots, uint64_t pitch, const void *segs,
                                                           const uint64_t *seg_pos, uint32_t max_segs, uint8_t *ctl,
                                                           bool verify, hipStream_t s);
// d_states[5*i ..] = the SHA-1 IV (sha.c:149-163) for i < n.
BTSHA1_HIDDEN hipError_t btsha1_launch_states_init(uint32_t *d_states, uint64_t n, hipStream_t s);
// One column of n equal chunks (k_sha1_lat's column forms): chunk i's column
// is `width` bytes (a 64-byte multiple) at d_col + i*pitch; d_state holds
// each chunk's chaining state between columns (5 x n words, word k of chunk i
// at d_state[k*n + i], device memory).  FIRST starts from the SHA-1 IV,
// MIDDLE continues, LAST continues and finishes a message of msg_len bytes
// in all (the column ends the message: msg_len is a 64-byte multiple ending
// at it), writing digest i (big-endian, 4-byte aligned) to d_dig + 20*i, and
// with d_ok (LAST only) also ok[i] = digest i == d_exp[20*i ..] (util.c:313;
// d_dig may then be NULL).
#define BTSHA1_COLUMN_FIRST 0
#define BTSHA1_COLUMN_MIDDLE 1
#define BTSHA1_COLUMN_LAST 2
hipError_t btsha1_launch_column(const void *d_col, uint64_t n, uint32_t pitch, uint32_t width, int part,
                                uint32_t *d_state, uint64_t msg_len, uint8_t *d_dig, hipStream_t s,
                                const uint8_t *d_exp = nullptr, uint8_t *d_ok = nullptr);
// Synthetic stream words [first_word, first_word + nbytes/8) into d_buf (16-byte aligned).
hipError_t btsha1_launch_fill(void *d_buf, uint64_t nbytes, uint64_t first_word, uint64_t seed, hipStream_t s);
// Digest lookup: d_index[q] = smallest i with table[i] == queries[q], else -1.
// d_slots: cap (power of two, > n) u32 scratch.
hipError_t btsha1_launch_lookup(const uint8_t *d_table, uint64_t n, const uint8_t *d_queries, uint64_t m,
                                uint32_t *d_slots, uint32_t cap, int64_t *d_index, hipStream_t s);
// Barrier tallies {waves checked, barriers counted, mismatches} of a
// -DBT_SHA1_DEBUG_BARRIERS build (synchronises the device first; reset != 0
// zeroes them); hipErrorNotSupported in the production build.
hipError_t btsha1_debug_barrier_stats(uint64_t out[3], int reset);
