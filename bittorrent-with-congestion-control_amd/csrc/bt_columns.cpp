// bt_columns.cpp -- the column split: a batch's chunks are copied column by
// column and each column is hashed by k_sha1_lat's column form as soon as it
// has arrived, so the batch ends one column's hash, not one whole chunk's,
// after its last byte crossed PCIe.  Used by the host pipelines' last batch
// (make_chunks' hashing, chunk.c:13-25) and by the verifier's batches
// (save_chunk's hash + memcmp, util.c:304-337).
#include "bt_columns.h"

namespace btsha1 {

namespace {
// Column-split last batch (HostFeed): columns per chunk (8 by default;
// BT_SHA1_COLUMNS overrides, 2..16, 0 or 1 = off), for chunks of at least
// kColumnMinChunk (a chain's latency scales with the chunk) and a split part
// of at least column_min_bytes() (256 MiB; BT_SHA1_COLUMN_MIN_MB overrides:
// below that the columns' copies are shorter than the previous batch's hash,
// which then ends the call anyway).
constexpr uint64_t kColumnMinChunk = 64ull << 10;
uint32_t columns() {
  static const uint32_t v = [] {
    const char *e = getenv("BT_SHA1_COLUMNS");
    const long x = e ? atol(e) : 8;
    return (uint32_t)(x < 2 ? 0 : (x > (long)kMaxColumns ? kMaxColumns : x));
  }();
  return v;
}
}  // namespace

uint64_t column_min_bytes() {
  static const uint64_t v = [] {
    const char *e = getenv("BT_SHA1_COLUMN_MIN_MB");
    const long mb = e ? atol(e) : 256;
    return (uint64_t)(mb < 0 ? 0 : mb) << 20;
  }();
  return v;
}

// Columns a chunk of chunk_len bytes is split into, by the pipelines' tail
// and the verifier's batches alike: columns(), halved until the chunk divides
// into whole 64-byte blocks; 0 (no split: whole-chunk launches) when there is
// no such count, the chunk is under kColumnMinChunk, or the column -- dense,
// pitch == width = chunk_len / parts -- is one btsha1_launch_column refuses:
// no 64-byte multiple, a pitch off 16 bytes, or 64 * pitch >= 4 GiB (a column
// of 64 MiB or more: a workgroup's 64 rows are addressed by 32-bit offsets).
uint32_t split_columns(uint64_t chunk_len) {
  uint32_t parts = columns();
  while (parts >= 2 && chunk_len % (64ull * parts)) parts /= 2;
  if (parts < 2 || chunk_len < kColumnMinChunk) return 0;
  const uint64_t width = chunk_len / parts;
  return width && !(width & 63u) && !(width & 15u) && 64ull * width < (1ull << 32) ? parts : 0;
}

// Column j's copy has just been queued on copy_s: mark its end with the
// column's event, make the hash stream wait for it, and hash the column there
// -- FIRST from the IV, LAST finishing the message (d_dig / d_exp / d_ok are
// read by the LAST launch only) -- while the next column crosses PCIe.
int hash_column(const ColumnRun &r, uint32_t j, uint8_t *d_dig, const uint8_t *d_exp, uint8_t *d_ok) {
  if (!r.cev[j]) BT_CK(hipEventCreateWithFlags(&r.cev[j], hipEventDisableTiming));
  BT_CK(hipEventRecord(r.cev[j], r.copy_s));
  BT_CK(hipStreamWaitEvent(r.hash_s, r.cev[j], 0));
  const int part = j == 0 ? BTSHA1_COLUMN_FIRST : j + 1 == r.parts ? BTSHA1_COLUMN_LAST : BTSHA1_COLUMN_MIDDLE;
  BT_CK(btsha1_launch_column(r.d_cols + j * r.rows * r.width, r.rows, (uint32_t)r.width, (uint32_t)r.width, part,
                             r.d_state, r.msg_len, d_dig, r.hash_s, d_exp, d_ok));
  return 0;
}

}  // namespace btsha1
