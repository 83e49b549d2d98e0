// tablebytes.hpp — device-only byte helpers over a table's data buffer: the
// unaligned 8-byte load and the base64 alphabet, shared by the index build
// (sstable.hip), the search (tablesearch.hpp) and the decode (b64decode.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cb {

// 8 bytes at any address p of a table's data buffer (allocated with 16 bytes
// of slack past the file), little-endian: three aligned dword loads and two
// byte-aligns instead of eight byte loads.
__device__ __forceinline__ uint64_t ld8(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t x = w[0], y = w[1], z = w[2];
  const uint32_t lo = __builtin_amdgcn_alignbyte(y, x, sh);
  const uint32_t hi = __builtin_amdgcn_alignbyte(z, y, sh);
  return (uint64_t)hi << 32 | lo;
}

// Up to 8 data bytes as a big-endian word, zero-padded past m.
__device__ __forceinline__ uint64_t ld8_be(const uint8_t* p, uint64_t m) {
  const uint64_t v = __builtin_bswap64(ld8(p));
  return m >= 8 ? v : (m ? v & ~(~0ull >> (8 * m)) : 0);
}

// Standard-alphabet value of a byte, -1 if outside it.
__device__ __forceinline__ int b64v(uint32_t c) {
  int v = -1;
  v = (c - 'A' < 26u) ? (int)(c - 'A') : v;
  v = (c - 'a' < 26u) ? (int)(c - 'a') + 26 : v;
  v = (c - '0' < 10u) ? (int)(c - '0') + 52 : v;
  v = c == '+' ? 62 : v;
  v = c == '/' ? 63 : v;
  return v;
}

// base64 0.21.7 STANDARD (canonical padding, zero trailing bits): decoded
// length of p[0..len) (table data), or -1 if STANDARD.decode would fail.
__device__ __forceinline__ int64_t b64_len(const uint8_t* p, uint64_t len) {
  if (len & 3) return -1;
  if (!len) return 0;
  const uint32_t pad = p[len - 1] == '=' ? (p[len - 2] == '=' ? 2 : 1) : 0;
  const uint64_t body = len - pad;
  int last = 0;
  for (uint64_t i = 0; i < body; i += 8) {
    const uint64_t w = ld8(p + i);
    int bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const int v = i + j < body ? b64v((uint32_t)(w >> (8 * j)) & 0xFF) : 0;
      bad |= v;  // negative iff some v < 0
      if (i + j == body - 1) last = v;
    }
    if (bad < 0) return -1;
  }
  if (pad == 2 && (last & 0x0F)) return -1;
  if (pad == 1 && (last & 0x03)) return -1;
  return (int64_t)(len / 4 * 3 - pad);
}

}  // namespace cb
