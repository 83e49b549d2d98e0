// select.hpp — rows projected and written out as JSON on the device
// (select.hip; the C ABI's cb_scan_select and cb_rows_select): the response
// bytes of the reference's exec_select_schema (src/query.rs:365-432) over rows
// that are already in device memory, by the rule of rowselect.hpp.
//
// Two kernels, one lane per row, around an exclusive scan (launch_scan_u64,
// sstable.hpp): the first sizes every row's text, the scan turns the sizes
// plus one separator each into offsets, the host reads the total once and
// sizes the text from it, the second writes every text at its offset with the
// separators and brackets between them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rowselect.hpp"

namespace cb {

constexpr uint32_t kSelectBlock = 256;  // rows per block of both kernels

// A row's slots (rowselect.hpp) in column-major arrays: the device's form, for
// the selection's kernels and the write's (write.hip).
struct ColumnSlots {
  uint64_t *at, *len;  // (already at the row)
  uint64_t n;
  __device__ void set(uint32_t c, uint64_t a, uint64_t l) {
    at[c * n] = a;
    len[c * n] = l;
  }
  __device__ void get(uint32_t c, uint64_t* a, uint64_t* l) const {
    *a = at[c * n];
    *l = len[c * n];
  }
};

// The rows: row i's key is keys[key_off[i] .. key_off[i + 1]), its value
// vals[val_off[i] .. val_off[i + 1]); which (nullable: every row is there)
// says with which[i] < 0 that there is no row i. A row's key parts begin
// after skip[r] bytes, r its range by range_off (nr + 1 offsets; a scan
// result's ranges), or after skip_all bytes when skip is null.
struct SelectRows {
  const uint64_t* key_off;
  const uint8_t* keys;
  const int32_t* which;
  const uint64_t* val_off;
  const uint8_t* vals;
  uint64_t n;
  const uint64_t* range_off;
  const uint32_t* skip;
  uint32_t nr, skip_all;
};

// Per row: flags[i] (rowselect.hpp's kRow*), inc[i] = the text's length + 1,
// or 0 without text; per (column c, row i), at slot c * n + i (column-major:
// a wave's stores are neighbours), select_size's slot. *with_text += the rows
// that have text (the caller zeroes it).
hipError_t launch_select_size(const SelectRows& rows, const SelectCols* sel, int mode, uint8_t* flags, uint64_t* inc,
                              uint64_t* slot_at, uint64_t* slot_len, uint64_t* with_text, hipStream_t s);
// off: the exclusive scan of inc (off[n] = its total). The response into
// text: kSelectJson  [ t0 , t1 ... ]  (off[n] + 1 bytes, or the two of [] when
// off[n] is 0), kSelectMeta  t0 \n t1 ...  (off[n] - 1 bytes, or none); row i's
// text lies at row_at[i], row_len[i] bytes long (0 without text).
hipError_t launch_select_write(const SelectRows& rows, const SelectCols* sel, int mode, const uint8_t* flags,
                               const uint64_t* inc, const uint64_t* off, const uint64_t* slot_at,
                               const uint64_t* slot_len, uint64_t* row_at, uint64_t* row_len, uint8_t* text,
                               hipStream_t s);

}  // namespace cb
