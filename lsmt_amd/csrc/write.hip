// write.hip — the kernels of cb_rows_write (write.hpp): one lane per row, the
// rule of rowwrite.hpp over the row's cells and its old value.
//
//   k_write_size — walks the old payload once (write_size): the row's flags,
//       the lengths of its key, value and log record, and per kept column
//       where the old value's string begins and how long it is escaped, into
//       column-major global arrays (no per-lane array). A wave adds its
//       flagged rows, and its rows with a record too long to replay, to two
//       counters.
//   k_write_emit — writes the key, the value and the record at their offsets
//       (write_emit): the value's bytes go out once, each also into a 24-bit
//       word that leaves as one whole quad of base64.
//
// Byte stores from one lane per row, as in k_select_write: a block takes as
// long as its longest row, and a wave's stores are not neighbours.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "profile.hpp"
#include "write.hpp"

namespace cb {
namespace {

__device__ __forceinline__ bool row_has_old(const WriteBatch& b, uint64_t i) {
  return b.old_which && b.old_which[i] >= 0;
}

__device__ __forceinline__ DecodedBytes row_old(const WriteBatch& b, uint64_t i, bool has) {
  if (!has) return DecodedBytes(nullptr, 0);
  const uint64_t vo = b.old_val_off[i];
  return DecodedBytes(b.old_vals + vo, b.old_val_off[i + 1] - vo);
}

__global__ __launch_bounds__(kSelectBlock) void k_write_size(WriteBatch b, const WriteCols* __restrict__ w,
                                                             uint8_t* __restrict__ flags, uint64_t* __restrict__ klen,
                                                             uint64_t* __restrict__ vlen, uint64_t* __restrict__ rlen,
                                                             uint64_t* __restrict__ slot_at,
                                                             uint64_t* __restrict__ slot_len,
                                                             uint64_t* __restrict__ counts) {
  const uint64_t i = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x;
  bool flagged = false, toolong = false;
  if (i < b.n) {
    const bool has = row_has_old(b, i);
    DecodedBytes old = row_old(b, i, has);
    ColumnSlots slots{slot_at + i, slot_len + i, b.n};
    uint8_t f = 0;
    uint64_t kl = 0, vl = 0, rl = 0;
    write_size(*w, b.ns_len, b.ns_ctl != 0, b.cells, b.cell_off + i * w->width, has, old, slots, &f, &kl, &vl, &rl);
    flags[i] = f;
    klen[i] = kl;
    vlen[i] = vl;
    rlen[i] = rl;
    flagged = f != 0;
    toolong = rl >= kWriteMaxRecord;
  }
  const uint64_t bf = __ballot(flagged), bl = __ballot(toolong);
  if ((threadIdx.x & 63u) == 0) {
    if (bf) atomicAdd((unsigned long long*)counts, (unsigned long long)__popcll(bf));
    if (bl) atomicAdd((unsigned long long*)counts + 1, (unsigned long long)__popcll(bl));
  }
}

__global__ __launch_bounds__(kSelectBlock) void k_write_emit(WriteBatch b, const WriteCols* __restrict__ w,
                                                             const uint8_t* __restrict__ flags,
                                                             const uint64_t* __restrict__ key_off,
                                                             const uint64_t* __restrict__ val_off,
                                                             const uint64_t* __restrict__ log_off,
                                                             const uint64_t* __restrict__ slot_at,
                                                             const uint64_t* __restrict__ slot_len,
                                                             uint8_t* __restrict__ keys, uint8_t* __restrict__ vals,
                                                             uint8_t* __restrict__ log) {
  const uint64_t i = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x;
  if (i >= b.n) return;
  DecodedBytes old = row_old(b, i, row_has_old(b, i));
  const ColumnSlots slots{const_cast<uint64_t*>(slot_at) + i, const_cast<uint64_t*>(slot_len) + i, b.n};
  write_emit(*w, b.ns, b.ns_len, b.cells, b.cell_off + i * w->width, b.ts ? b.ts[i] : b.ts_all, old, flags[i], slots,
             keys + key_off[i], vals + val_off[i], log + log_off[i]);
}

}  // namespace

hipError_t launch_write_size(const WriteBatch& b, const WriteCols* w, uint8_t* flags, uint64_t* klen, uint64_t* vlen,
                             uint64_t* rlen, uint64_t* slot_at, uint64_t* slot_len, uint64_t* counts, hipStream_t s) {
  if (!b.n) return hipSuccess;
  ProfScope ps("k_write_size", s);
  hipLaunchKernelGGL(k_write_size, dim3(blocks_for(b.n, kSelectBlock)), dim3(kSelectBlock), 0, s, b, w, flags, klen,
                     vlen, rlen, slot_at, slot_len, counts);
  return hipGetLastError();
}

hipError_t launch_write_emit(const WriteBatch& b, const WriteCols* w, const uint8_t* flags, const uint64_t* key_off,
                             const uint64_t* val_off, const uint64_t* log_off, const uint64_t* slot_at,
                             const uint64_t* slot_len, uint8_t* keys, uint8_t* vals, uint8_t* log, hipStream_t s) {
  if (!b.n) return hipSuccess;
  ProfScope ps("k_write_emit", s);
  hipLaunchKernelGGL(k_write_emit, dim3(blocks_for(b.n, kSelectBlock)), dim3(kSelectBlock), 0, s, b, w, flags, key_off,
                     val_off, log_off, slot_at, slot_len, keys, vals, log);
  return hipGetLastError();
}

}  // namespace cb
