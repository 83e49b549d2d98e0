// b64decode.hip — the value tail of the read path: the found values' offsets
// (tile sums, then a block scan) and their base64 decode (see sstable.hpp).
// Values were validated at index time (LineRec::vdl), so the decode only
// translates.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "launch.hpp"
#include "profile.hpp"
#include "sstable.hpp"
#include "tablebytes.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = 256;

}  // namespace

namespace {

// In-place exclusive scan of the nt tile sums a producer kernel left (one
// block: a few thousand values), *total_out = their sum. The consumer kernel
// then reads its block's base in one load; see launch_tile_scan.
__global__ __launch_bounds__(1024) void k_tile_scan(uint64_t* __restrict__ tsum, uint64_t nt,
                                                    uint64_t* __restrict__ total_out) {
  // 4 consecutive values per thread: 4096 tiles (1M keys at 256 per tile) in
  // one round of loads, one block scan and one round of stores
  constexpr uint64_t kPer = 4, kChunk = 1024 * kPer;
  uint64_t carry = 0;
  for (uint64_t c0 = 0; c0 < nt; c0 += kChunk) {
    const uint64_t i0 = c0 + threadIdx.x * kPer;
    uint64_t v[kPer], sum = 0;
#pragma unroll
    for (uint64_t j = 0; j < kPer; ++j) {
      v[j] = i0 + j < nt ? tsum[i0 + j] : 0;
      sum += v[j];
    }
    uint64_t total;
    uint64_t p = carry + block_scan<1024>(sum, &total);
#pragma unroll
    for (uint64_t j = 0; j < kPer; ++j) {
      if (i0 + j < nt) tsum[i0 + j] = p;
      p += v[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

}  // namespace

hipError_t launch_tile_scan(uint64_t* tsum, uint64_t nt, uint64_t* total_out, hipStream_t s) {
  ProfScope ps("k_tile_scan", s);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(1024), 0, s, tsum, nt, total_out);
  return hipGetLastError();
}

// ---- base64 decode of the found values ----

namespace {

// Decode 4 base64 chars (canonical, validated at index time) to 3 bytes.
__device__ __forceinline__ uint32_t b64_quad(const uint8_t c[4]) {
  return (uint32_t)(b64v(c[0]) & 63) << 18 | (uint32_t)(b64v(c[1]) & 63) << 12 |
         (uint32_t)(b64v(c[2]) & 63) << 6 | (uint32_t)(b64v(c[3]) & 63);
}

// dl bytes decoded from src (4*ceil(dl/3) canonical chars), written through
// put(j, byte).
template <class Put>
__device__ __forceinline__ void b64_decode_into(const uint8_t* src, uint64_t dl, Put put) {
  const uint64_t len = (dl + 2) / 3 * 4;
  uint64_t j = 0;
  for (uint64_t q = 0; q < len; q += 8) {  // two quads per step
    const uint64_t x = ld8(src + q);
    uint8_t c[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) c[i] = (uint8_t)(x >> (8 * i));
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t w = b64_quad(c + 4 * h);
      if (j < dl) put(j++, (uint8_t)(w >> 16));
      if (j < dl) put(j++, (uint8_t)(w >> 8));
      if (j < dl) put(j++, (uint8_t)w);
    }
  }
}

// Values of up to 18 bytes (24 chars): the dwords their chars span, loaded
// unconditionally (indices clamped to the last one, so every load stays inside
// the span) so the caller can issue them before other work.
struct SmallB64 {
  uint32_t x[7];
  uint32_t sh;
};
constexpr uint64_t kSmallB64Bytes = 18;

__device__ __forceinline__ void b64_small_load(const uint8_t* src, uint64_t dl, SmallB64& v) {
  const uint64_t len = (dl + 2) / 3 * 4;
  const uintptr_t a = (uintptr_t)src;
  v.sh = (uint32_t)(a & 3);
#ifndef CB_B64_DWORD_LOADS
  // three 16-B loads of the aligned 48 B holding the chars (each clamped to
  // the last 16 B the chars reach, so no load leaves their span), then the 7
  // dwords from dword (a & 15) / 4 on: 3 load instructions per value instead
  // of 7 (the loads' random lines are the kernel's cost)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) u32x4* gq;
  const gq q = (gq)(a & ~(uintptr_t)15);
  const uint32_t lastq = ((uint32_t)(a & 15) + (uint32_t)len - 1) >> 4;
  const u32x4 q0 = q[0], q1 = q[lastq < 1 ? lastq : 1], q2 = q[lastq < 2 ? lastq : 2];
  const uint32_t d[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
  const uint32_t o = (uint32_t)(a & 12) >> 2;
#pragma unroll
  for (uint32_t i = 0; i < 7; ++i)
    v.x[i] = o == 0 ? d[i] : o == 1 ? d[i + 1] : o == 2 ? d[i + 2] : d[i + 3];
#else
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint32_t last = (v.sh + (uint32_t)len + 3) / 4 - 1;
#pragma unroll
  for (uint32_t i = 0; i < 7; ++i) v.x[i] = w[i < last ? i : last];
#endif
}

// dl <= 18 bytes decoded from the loaded dwords (realigned: y = one quad).
template <class Put>
__device__ __forceinline__ void b64_small_decode(const SmallB64& v, uint64_t dl, Put put) {
  uint64_t j = 0;
#pragma unroll
  for (uint32_t i = 0; i < 6; ++i) {
    const uint32_t y = __builtin_amdgcn_alignbyte(v.x[i + 1], v.x[i], v.sh);
    const uint8_t c[4] = {(uint8_t)y, (uint8_t)(y >> 8), (uint8_t)(y >> 16), (uint8_t)(y >> 24)};
    const uint32_t q = b64_quad(c);
    if (j < dl) put(j++, (uint8_t)(q >> 16));
    if (j < dl) put(j++, (uint8_t)(q >> 8));
    if (j < dl) put(j++, (uint8_t)q);
  }
}

constexpr uint32_t kDecodeLds = 16384;  // staged output bytes per block

// Value offsets: the block's base is the scanned value-byte tile sum (tsum:
// k_get_many, then k_tile_scan, which also wrote voff[n] = the total), plus
// the scan of its own lengths; voff[k] is written here. out ==
// nullptr, or a total above cap: offsets only. Otherwise the block's values
// are one contiguous output range; when it fits in LDS, lanes decode into LDS
// and the block writes the range with aligned dword stores, else lanes write
// their bytes directly.
// (Two adjacent keys per thread, so all of a 1M-key batch's value loads are
// in flight in one round, measured slower: read path 14.3 against 14.8-14.9 G
// gets/s, wide fan-out 1.97-2.00 against 2.04-2.06; experiment r05_b64kpt, HISTORY.md.)
// RAW (grids of at most kRawTiles blocks): tsum holds the producer's
// unscanned tile sums, and every block sums the ones before it (and all of
// them, for the total; block 0 stores it as voff[n]) from one round of loads
// issued with its other loads, in place of a k_tile_scan launch between the
// two kernels.
constexpr uint32_t kRawPer = 4, kRawTiles = kNT * kRawPer;
static_assert(kNT == kDecodeTile && (uint64_t)kRawTiles * kNT == 262144, "decode_raw_max()");
template <bool RAW>
__global__ __launch_bounds__(kNT) void k_b64_decode(const uint64_t* __restrict__ vsrc,
                                                    const uint64_t* __restrict__ dlen,
                                                    const uint64_t* __restrict__ tsum, uint64_t n,
                                                    uint64_t* __restrict__ voff,
                                                    uint8_t* __restrict__ out, uint64_t cap) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kDecodeLds + 4];  // +4: the last dword pair
  const uint64_t b0 = (uint64_t)blockIdx.x * kNT;
  const uint64_t k = b0 + threadIdx.x;
  // Every independent load first (lengths, sources, the block's base, the
  // total), then small values' chars, so one memory wait covers each round
  // and the block scan runs while the chars arrive.
  const uint64_t dl = k < n ? dlen[k] : 0;
  const uint8_t* src = (const uint8_t*)(uintptr_t)(k < n ? vsrc[k] : 0);
  uint64_t base = 0, vn = 0, ts[kRawPer];
  if constexpr (RAW) {
#pragma unroll
    for (uint32_t j = 0; j < kRawPer; ++j) {
      const uint32_t i = threadIdx.x * kRawPer + j;
      ts[j] = i < gridDim.x ? tsum[i] : 0;
    }
  } else {
    base = tsum[blockIdx.x];  // k_tile_scan: the tiles before
    vn = voff[n];             // k_tile_scan's total
  }
  SmallB64 sv;
  const bool small = dl && dl <= kSmallB64Bytes;
  // (RAW: the total is not known yet, so the chars load whenever there is an
  // output; a total above cap then leaves them unused)
  const bool want = out && (RAW || vn <= cap);
  if (want && small) b64_small_load(src, dl, sv);
  uint64_t total, pre;
  if constexpr (RAW) {
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRawPer; ++j) {
      all += ts[j];
      before += threadIdx.x * kRawPer + j < blockIdx.x ? ts[j] : 0;
    }
    pre = block_scan_sum2<kNT>(dl, before, all, &total, &base, &vn);
    if (blockIdx.x == 0 && threadIdx.x == 0) voff[n] = vn;
  } else {
    pre = block_scan<kNT>(dl, &total);
  }
  const bool write = out && vn <= cap;  // uniform
  const uint64_t o = base + pre;
  if (k < n) voff[k] = o;
  if (!write) return;
  if (total > kDecodeLds) {  // uniform: large values, direct byte stores
    if (small) b64_small_decode(sv, dl, [&](uint64_t j, uint8_t v) { out[o + j] = v; });
    else if (dl) b64_decode_into(src, dl, [&](uint64_t j, uint8_t v) { out[o + j] = v; });
    return;
  }
  if (small) b64_small_decode(sv, dl, [&](uint64_t j, uint8_t v) { stage[o - base + j] = v; });
  else if (dl) b64_decode_into(src, dl, [&](uint64_t j, uint8_t v) { stage[o - base + j] = v; });
  __syncthreads();
  // out[base .. base+total): bytes before the first 4-aligned address, then
  // aligned dwords, then the tail
  uint8_t* g = out + base;
  const uint64_t mis = (4 - ((uintptr_t)g & 3)) & 3;
  const uint64_t head = mis < total ? mis : total;
  if (threadIdx.x < head) g[threadIdx.x] = stage[threadIdx.x];
  const uint64_t body = (total - head) / 4;
  uint32_t* gw = reinterpret_cast<uint32_t*>(g + head);
  for (uint64_t i = threadIdx.x; i < body; i += kNT) {
    const uint32_t p = (uint32_t)(head + 4 * i);  // two aligned LDS dwords, realigned
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(stage) + (p >> 2);
    gw[i] = __builtin_amdgcn_alignbyte(sw[1], sw[0], p & 3);
  }
  const uint64_t tail0 = head + 4 * body;
  if (tail0 + threadIdx.x < total) g[tail0 + threadIdx.x] = stage[tail0 + threadIdx.x];
}

}  // namespace

hipError_t launch_b64_decode(const uint64_t* vsrc, const uint64_t* dlen, const uint64_t* tsum,
                             uint64_t n, uint64_t* voff, uint8_t* out, uint64_t cap, hipStream_t s, bool raw) {
  if (!n) return hipSuccess;
  const uint32_t nb = blocks_for(n, kNT);
  if (raw && nb > kRawTiles) return hipErrorInvalidValue;
  ProfScope ps("k_b64_decode", s);
  if (raw)
    hipLaunchKernelGGL(k_b64_decode<true>, dim3(nb), dim3(kNT), 0, s, vsrc, dlen, tsum, n, voff, out, cap);
  else
    hipLaunchKernelGGL(k_b64_decode<false>, dim3(nb), dim3(kNT), 0, s, vsrc, dlen, tsum, n, voff, out, cap);
  return hipGetLastError();
}

}  // namespace cb
