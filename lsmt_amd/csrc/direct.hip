// direct.hip — the direct build and probe of one or a few Bloom filters: one
// lane per key, no partition pass.
//
// Reference semantics: /root/reference/src/bloom.rs:26-51 (hashes / insert /
// may_contain). Filter layout in HBM: packed uint32 words, bit p at word p>>5,
// bit p&31 (LSB-first).
//
// One lane per key: hash, then global atomicOr (build) or word gathers
// (probe). Latency-optimal for small batches; filters of
// at most 2^19 bits are built in LDS instead. Large batches take the tiled
// passes (tilebuild.hip, tileprobe.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devutil.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "profile.hpp"

namespace cb {
namespace {

template <int KEYK, int MODE>
__global__ __launch_bounds__(kBlock) void k_insert_direct(uint32_t* __restrict__ words, KeySrc ks,
                                                          uint64_t n, ModP mp) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
    uint64_t a, b;
    key_positions<KEYK, MODE>(ks, k, mp, a, b);
    atomicOr(&words[a >> 5], 1u << (a & 31));  // src/bloom.rs:42
    atomicOr(&words[b >> 5], 1u << (b & 31));  // src/bloom.rs:43
  }
}

// Filters of at most 2^19 bits (the product's m = 1024 flushes): the filter
// kept in LDS per block, so 2n ORs land in LDS instead of contending on
// m/32 words of HBM (1024 keys into m = 1024 by global atomics took 27.5 us,
// every word taking ~64 serialised memory-side atomics). store_all: one
// block on a fresh filter writes every allocated word (zeros past nw), so the
// filter needs no fill first; otherwise each block ORs its non-zero words in.
template <int KEYK, int MODE>
__global__ __launch_bounds__(1024) void k_insert_lds(uint32_t* __restrict__ words, uint32_t nw, uint32_t nw_alloc,
                                                    KeySrc ks, uint64_t n, ModP mp, uint32_t store_all) {
  extern __shared__ uint32_t lw[];
  for (uint32_t i = threadIdx.x; i < nw; i += 1024) lw[i] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * 1024;
  for (uint64_t k = (uint64_t)blockIdx.x * 1024 + threadIdx.x; k < n; k += stride) {
    uint64_t a, b;
    key_positions<KEYK, MODE>(ks, k, mp, a, b);
    atomicOr(&lw[a >> 5], 1u << (a & 31));  // src/bloom.rs:42
    atomicOr(&lw[b >> 5], 1u << (b & 31));  // src/bloom.rs:43
  }
  __syncthreads();
  if (store_all) {
    for (uint32_t i = threadIdx.x; i < nw_alloc; i += 1024) words[i] = i < nw ? lw[i] : 0u;
  } else {
    for (uint32_t i = threadIdx.x; i < nw; i += 1024) {
      const uint32_t v = lw[i];
      if (v) atomicOr(&words[i], v);
    }
  }
}

// One wave handles 64 consecutive keys (one hits word per filter). Lane f
// collects the ballot for filter f and stores it: one store per wave.
template <int KEYK, int MODE>
__global__ __launch_bounds__(kBlock) void k_probe_direct(FilterPtrs fp, uint32_t nf, KeySrc ks,
                                                         uint64_t n, ModP mp,
                                                         uint64_t* __restrict__ hits,
                                                         uint64_t hwords) {
  const uint32_t lane = lane_id();
  const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
  for (uint64_t wv = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; wv < hwords;
       wv += nwaves) {
    const uint64_t k = wv * 64 + lane;
    const bool valid = k < n;
    uint64_t a = 0, b = 0;
    if (valid) key_positions<KEYK, MODE>(ks, k, mp, a, b);
    const uint64_t wa = a >> 5, wb = b >> 5;
    const uint32_t sa = (uint32_t)(a & 31), sb = (uint32_t)(b & 31);
    uint64_t mine = 0;
    for (uint32_t f0 = 0; f0 < nf; f0 += 8) {
      uint32_t va[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) va[i] = (valid && f0 + i < nf) ? fp.w[f0 + i][wa] : 0u;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        bool hit = false;
        if ((va[i] >> sa) & 1u) hit = (fp.w[f0 + i][wb] >> sb) & 1u;  // `&&` short-circuit
        const uint64_t bal = __ballot(hit);
        if (lane == f0 + i) mine = bal;
      }
    }
    if (lane < nf) hits[(uint64_t)fp.row[lane] * hwords + wv] = mine;
  }
}

}  // namespace

hipError_t launch_insert_direct(int keyk, int mode, uint32_t* words, const KeySrc& ks, uint64_t n,
                                const ModP& mp, hipStream_t s) {
  if (!n) return hipSuccess;
  const uint32_t grid = grid_for(n);
  ProfScope ps("k_insert_direct", s);
  CB_KEY_MODE_DISPATCH(keyk, mode,
                       hipLaunchKernelGGL((k_insert_direct<KK, MM>), dim3(grid), dim3(kBlock), 0, s, words, ks, n, mp));
  return hipGetLastError();
}

template <int KK, int MM>
static void insert_lds(uint32_t* words, uint32_t nw, uint32_t nw_alloc, const KeySrc& ks, uint64_t n, const ModP& mp,
                       bool store_all, uint32_t grid, size_t lds, hipStream_t s) {
  allow_lds(k_insert_lds<KK, MM>, lds);
  hipLaunchKernelGGL((k_insert_lds<KK, MM>), dim3(grid), dim3(1024), lds, s, words, nw, nw_alloc, ks, n, mp,
                     store_all ? 1u : 0u);
}

hipError_t launch_insert_lds(int keyk, int mode, uint32_t* words, uint64_t m, uint64_t nw_alloc, const KeySrc& ks,
                             uint64_t n, const ModP& mp, bool store_all, hipStream_t s) {
  if (!n) return hipSuccess;
  const uint64_t nw = (m + 31) / 32;
  if (m > kInsertLdsMaxBits || nw_alloc < nw) return hipErrorInvalidValue;
  const uint32_t grid = store_all ? 1u : (uint32_t)std::min<uint64_t>(128, (n + 8191) / 8192);
  const size_t lds = nw * 4;
  ProfScope ps("k_insert_lds", s);
  CB_KEY_MODE_DISPATCH(keyk, mode, (insert_lds<KK, MM>(words, (uint32_t)nw, (uint32_t)nw_alloc, ks, n, mp, store_all, grid, lds, s)));
  return hipGetLastError();
}

hipError_t launch_probe_direct(int keyk, int mode, const FilterPtrs& fp, uint32_t nf,
                               const KeySrc& ks, uint64_t n, const ModP& mp, uint64_t* hits,
                               uint64_t hwords, hipStream_t s) {
  if (!n || !nf) return hipSuccess;
  const uint64_t nw = (n + 63) / 64;
  const uint32_t grid = grid_for(nw * 64, 4096);
  ProfScope ps("k_probe_direct", s);
  CB_KEY_MODE_DISPATCH(keyk, mode,
                       hipLaunchKernelGGL((k_probe_direct<KK, MM>), dim3(grid), dim3(kBlock), 0, s, fp, nf, ks, n, mp,
                                          hits, hwords));
  return hipGetLastError();
}

}  // namespace cb
