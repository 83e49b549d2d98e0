// boolcodec.hip — a filter's packed words to and from the reference's
// Vec<bool> layout (one byte per bit, /root/reference/src/bloom.rs:6,12:
// BloomFilter's and BloomProto's `bits`), and the tail mask of a packed import.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch.hpp"

namespace cb {
namespace {

// packed words -> m bytes of 0/1 (the Vec<bool> layout). Thread per word.
__global__ __launch_bounds__(kBlock) void k_export_bools(const uint32_t* __restrict__ words,
                                                         uint64_t m, uint8_t* __restrict__ out) {
  const uint64_t nw = (m + 31) / 32;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < nw; w += stride) {
    const uint32_t v = words[w];
    const uint64_t p0 = w * 32;
    if (p0 + 32 <= m && !(reinterpret_cast<uintptr_t>(out + p0) & 15)) {
      uint32_t o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t nib = (v >> (4 * i)) & 15u;
        o[i] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
      }
      uint4* dst = reinterpret_cast<uint4*>(out + p0);
      dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
      dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
    } else {
      for (uint64_t p = p0; p < m && p < p0 + 32; ++p) out[p] = (v >> (p - p0)) & 1u;
    }
  }
}

// m bytes (nonzero = set) -> packed words; bits >= m are cleared.
__global__ __launch_bounds__(kBlock) void k_import_bools(uint32_t* __restrict__ words, uint64_t m,
                                                         const uint8_t* __restrict__ in) {
  const uint64_t nw = (m + 31) / 32;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < nw; w += stride) {
    const uint64_t p0 = w * 32;
    uint32_t v = 0;
    if (p0 + 32 <= m && !(reinterpret_cast<uintptr_t>(in + p0) & 15)) {
      const uint4* src = reinterpret_cast<const uint4*>(in + p0);
      const uint4 x0 = src[0], x1 = src[1];
      const uint32_t xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t x = xs[i];
        const uint32_t nib = ((x & 0xFFu) != 0) | (((x >> 8) & 0xFFu) != 0) << 1 |
                             (((x >> 16) & 0xFFu) != 0) << 2 | ((x >> 24) != 0) << 3;
        v |= nib << (4 * i);
      }
    } else {
      for (uint64_t p = p0; p < m && p < p0 + 32; ++p) v |= (uint32_t)(in[p] != 0) << (p - p0);
    }
    words[w] = v;
  }
}

// Clears the bits >= m of the last word (packed imports must not carry bits
// the reference's Vec<bool> of length m cannot hold).
__global__ void k_mask_tail(uint32_t* words, uint64_t m) {
  if (threadIdx.x == 0) words[m >> 5] &= (1u << (m & 31)) - 1u;
}

}  // namespace

hipError_t launch_mask_tail(uint32_t* words, uint64_t m, hipStream_t s) {
  if (!(m & 31)) return hipSuccess;
  hipLaunchKernelGGL(k_mask_tail, dim3(1), dim3(64), 0, s, words, m);
  return hipGetLastError();
}

hipError_t launch_export_bools(const uint32_t* words, uint64_t m, uint8_t* out, hipStream_t s) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_export_bools, dim3(grid_for((m + 31) / 32, 8192)), dim3(kBlock), 0, s,
                     words, m, out);
  return hipGetLastError();
}

hipError_t launch_import_bools(uint32_t* words, uint64_t m, const uint8_t* in, hipStream_t s) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_import_bools, dim3(grid_for((m + 31) / 32, 8192)), dim3(kBlock), 0, s,
                     words, m, in);
  return hipGetLastError();
}

}  // namespace cb
