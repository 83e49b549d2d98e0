// write.hpp — a batch of SQL writes turned into the store's bytes on the
// device (write.hip; the C ABI's cb_rows_write): per row the key, the value
// and the log record of the reference's exec_insert / exec_update /
// exec_delete (src/query.rs:162-261) followed by insert_ns_ts and
// insert_internal (src/lib.rs:96-116, 154-157), by the rule of rowwrite.hpp.
//
// Two kernels, one lane per row, around three exclusive scans
// (launch_scan_u64, sstable.hpp): the first sizes every row's key, value and
// record, the scans turn the sizes into offsets, the host reads the three
// totals once and sizes the outputs from them, the second writes every row's
// three byte strings at their offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rowwrite.hpp"
#include "select.hpp"

namespace cb {

// The batch (device pointers): row i's cell j is cells[cell_off[i * width + j]
// .. cell_off[i * width + j + 1]) (cell_off is not read with a width of 0);
// its timestamp ts[i], or ts_all when ts is null; its old value
// old_vals[old_val_off[i] .. old_val_off[i + 1]) unless old_which[i] < 0 or
// old_which is null (no row has one). ns_ctl: the namespace holds \t or \n.
struct WriteBatch {
  const uint8_t* cells;
  const uint64_t* cell_off;
  const uint64_t* ts;
  uint64_t ts_all;
  const int32_t* old_which;
  const uint8_t* old_vals;
  const uint64_t* old_val_off;
  uint64_t n;
  const uint8_t* ns;
  uint64_t ns_len;
  uint32_t ns_ctl;
};

// Per row: flags[i] (rowwrite.hpp's kWritten*), klen[i], vlen[i], rlen[i];
// per (column c, row i), at slot c * n + i, write_size's slot. counts[0] +=
// the rows with any flag, counts[1] += the rows whose record is
// kWriteMaxRecord bytes or longer (the caller zeroes both).
hipError_t launch_write_size(const WriteBatch& b, const WriteCols* w, uint8_t* flags, uint64_t* klen, uint64_t* vlen,
                             uint64_t* rlen, uint64_t* slot_at, uint64_t* slot_len, uint64_t* counts, hipStream_t s);
// key_off, val_off, log_off: the exclusive scans of klen, vlen and rlen. Row
// i's key, value and record at their offsets in keys, vals and log.
hipError_t launch_write_emit(const WriteBatch& b, const WriteCols* w, const uint8_t* flags, const uint64_t* key_off,
                             const uint64_t* val_off, const uint64_t* log_off, const uint64_t* slot_at,
                             const uint64_t* slot_len, uint8_t* keys, uint8_t* vals, uint8_t* log, hipStream_t s);

}  // namespace cb
