// devutil.hpp — the few device-side pieces the tiled kernels share
// (direct.hip, tilebuild.hip, tileprobe.hip, densefs.hip): the lane index,
// global-pointer and 16-byte vector types, the 16-B stores with a cache
// policy, the XCD-aware block order, and the launchers' LDS opt-in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cb {

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// Global (address space 1) pointer types: loads through them are global_load
// with counted vmcnt waits, never flat_load (which also waits on lgkmcnt).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4* gptr_u4;
typedef const __attribute__((address_space(1))) uint32_t* gptr_u32;

// Non-temporal 16-B store, for data written once and read only by later
// launches: no L2 allocation to write back at the kernel's end.
__device__ __forceinline__ void store16_nt(uint4* p, const uint4& v) {
  u32x4 w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(p));
}

// Write-through (sc1) 16-B store at byte offset off of a buffer resource.
__device__ __forceinline__ void store16_wt(__amdgpu_buffer_rsrc_t r, uint32_t off, const uint4& v) {
  const i32x4 w = {(int)v.x, (int)v.y, (int)v.z, (int)v.w};
  __builtin_amdgcn_raw_buffer_store_b128(w, r, off, 0, 16);
}

// XCD-aware order of a grid's N blocks over N tiles (or regions): workgroups
// are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md, "Workgroup
// dispatch"), so blocks b and b+8 share an L2. Giving each XCD a contiguous
// range of tiles lets the 128-B lines that adjacent tiles' runs and run-table
// entries share be fetched once per XCD instead of once per tile. Placement
// only affects speed, never results.
__device__ __forceinline__ uint32_t xcd_order(uint32_t bid, uint32_t N) {
  if (N & 7u) return bid;
  return (bid & 7u) * (N >> 3) + (bid >> 3);
}

// Dynamic LDS past the 64 KiB a launch gets without asking. (Set on every
// such launch and its result dropped; setting it once per instantiation, as
// densefs.hip's dense_part does, would be a change of behaviour.)
template <class K>
inline void allow_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace cb
