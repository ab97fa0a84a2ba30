// bt_columns.h -- the column split shared by the host pipelines' tail
// (bt_pipeline.cpp) and the verifier's batches (bt_verifier.cpp): when a
// chunk is split, and the step that hashes one column once its copy is done.
#pragma once
#include "bt_runtime.h"

namespace btsha1 __attribute__((visibility("hidden"))) {

uint64_t column_min_bytes();
uint32_t split_columns(uint64_t chunk_len);

// One column-split copy: `rows` chunks of msg_len bytes in `parts` columns of
// `width` bytes, column j dense (pitch == width) at d_cols + j * rows * width.
// The caller queues column j's copy on copy_s, then calls hash_column.
struct ColumnRun {
  hipStream_t copy_s, hash_s;
  hipEvent_t *cev;  // kMaxColumns events, one per column copy, created on first use
  uint32_t parts;
  uint64_t rows, width, msg_len;
  uint8_t *d_cols;
  uint32_t *d_state;  // the chunks' chaining state between columns
};
int hash_column(const ColumnRun &r, uint32_t j, uint8_t *d_dig, const uint8_t *d_exp = nullptr,
                uint8_t *d_ok = nullptr);

}  // namespace btsha1
