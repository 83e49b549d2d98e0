// select.hip — the kernels of cb_scan_select and cb_rows_select (select.hpp):
// one lane per row, the rule of rowselect.hpp over the row's key and its
// decoded value.
//
//   k_select_size — walks the row's payload once (select_size): the row's
//       flags, its text's length plus one separator, and per selected column
//       where the winning value begins and how long it is as written, into
//       column-major global arrays (no per-lane array). A wave adds its rows
//       with text to one counter.
//   k_select_write — writes the row's text at its offset (select_write),
//       each winning string read again from its recorded place, then the
//       separator behind it: , or ] in a JSON array, \n between lines and
//       nothing behind the last. Lane 0 writes the opening bracket.
//
// Byte stores from one lane per row: a block takes as long as its longest
// row, as in k_scan_match.
#include <hip/hip_runtime.h>

#include "compact.hpp"
#include "launch.hpp"
#include "profile.hpp"
#include "select.hpp"

namespace cb {
namespace {

__device__ __forceinline__ uint32_t row_skip(const SelectRows& r, uint64_t i) {
  if (!r.skip) return r.skip_all;
  return r.skip[last_le(r.nr, i, [&](uint32_t g) { return r.range_off[g]; })];  // the row's range (range_off[0] = 0)
}

__global__ __launch_bounds__(kSelectBlock) void k_select_size(SelectRows r, const SelectCols* __restrict__ sel, int mode,
                                                              uint8_t* __restrict__ flags, uint64_t* __restrict__ inc,
                                                              uint64_t* __restrict__ slot_at,
                                                              uint64_t* __restrict__ slot_len,
                                                              uint64_t* __restrict__ with_text) {
  const uint64_t i = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x;
  bool text = false;
  if (i < r.n) {
    const uint64_t ko = r.key_off[i], vo = r.val_off[i];
    DecodedBytes value(r.vals + vo, r.val_off[i + 1] - vo);
    ColumnSlots slots{slot_at + i, slot_len + i, r.n};
    uint8_t f = 0;
    const uint64_t len = select_size(*sel, r.keys + ko, r.key_off[i + 1] - ko, row_skip(r, i),
                                     r.which && r.which[i] < 0, value, mode, slots, &f);
    text = f & kRowText;
    flags[i] = f;
    inc[i] = text ? len + 1 : 0;
  }
  const uint64_t b = __ballot(text);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd((unsigned long long*)with_text, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(kSelectBlock) void k_select_write(SelectRows r, const SelectCols* __restrict__ sel, int mode,
                                                               const uint8_t* __restrict__ flags,
                                                               const uint64_t* __restrict__ inc,
                                                               const uint64_t* __restrict__ off,
                                                               const uint64_t* __restrict__ slot_at,
                                                               const uint64_t* __restrict__ slot_len,
                                                               uint64_t* __restrict__ row_at,
                                                               uint64_t* __restrict__ row_len,
                                                               uint8_t* __restrict__ text) {
  const uint64_t i = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x;
  if (i >= r.n) return;
  const uint64_t total = off[r.n], base = mode == kSelectJson ? 1 : 0;
  if (i == 0 && mode == kSelectJson) {
    text[0] = '[';
    if (!total) text[1] = ']';
  }
  const uint8_t f = flags[i];
  const uint64_t step = inc[i], at = base + off[i], len = step ? step - 1 : 0;
  row_at[i] = at;
  row_len[i] = len;
  if (!(f & kRowText)) return;
  const uint64_t ko = r.key_off[i], vo = r.val_off[i];
  DecodedBytes value(r.vals + vo, r.val_off[i + 1] - vo);
  const ColumnSlots slots{const_cast<uint64_t*>(slot_at) + i, const_cast<uint64_t*>(slot_len) + i, r.n};
  select_write(*sel, r.keys + ko, r.key_off[i + 1] - ko, row_skip(r, i), value, mode, f, slots, text + at);
  const bool last = off[i] + step == total;
  if (mode == kSelectJson) text[at + len] = last ? ']' : ',';
  else if (!last) text[at + len] = '\n';
}

}  // namespace

hipError_t launch_select_size(const SelectRows& rows, const SelectCols* sel, int mode, uint8_t* flags, uint64_t* inc,
                              uint64_t* slot_at, uint64_t* slot_len, uint64_t* with_text, hipStream_t s) {
  if (!rows.n) return hipSuccess;
  ProfScope ps("k_select_size", s);
  hipLaunchKernelGGL(k_select_size, dim3(blocks_for(rows.n, kSelectBlock)), dim3(kSelectBlock), 0, s, rows, sel, mode,
                     flags, inc, slot_at, slot_len, with_text);
  return hipGetLastError();
}

hipError_t launch_select_write(const SelectRows& rows, const SelectCols* sel, int mode, const uint8_t* flags,
                               const uint64_t* inc, const uint64_t* off, const uint64_t* slot_at,
                               const uint64_t* slot_len, uint64_t* row_at, uint64_t* row_len, uint8_t* text,
                               hipStream_t s) {
  if (!rows.n) return hipSuccess;
  ProfScope ps("k_select_write", s);
  hipLaunchKernelGGL(k_select_write, dim3(blocks_for(rows.n, kSelectBlock)), dim3(kSelectBlock), 0, s, rows, sel, mode,
                     flags, inc, off, slot_at, slot_len, row_at, row_len, text);
  return hipGetLastError();
}

}  // namespace cb
