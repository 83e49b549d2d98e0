// replay.hip — the two kernels of cb_log_replay (replay.hpp) between the line
// index's count -> scan -> emit -> finish chain, which splits the log as it
// splits a data file, and the merge's sort, select and format, which run over
// the gathered entries as they run over a compaction's lines.
//
//   k_log_mark — one lane per non-empty piece: the verdict of logline.hpp over
//       the piece's bytes (the TAB is k_line_finish's), has / klen for the two
//       scans that place the keys, vdl for the side records, and an atomicMin
//       of the first failing piece. A lane reads its own piece only, byte by
//       byte: a log is read once, and records are tens of bytes.
//   k_log_gather — one lane per piece again: an entry's key goes to its slot
//       counted from the END of the batch, so the batch is in reverse log
//       order without a second pass, and its side record beside it.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "logline.hpp"
#include "profile.hpp"
#include "replay.hpp"
#include "tablebytes.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = 256;

__global__ __launch_bounds__(kNT) void k_log_mark(const uint8_t* __restrict__ data, const LineRec* __restrict__ rec,
                                                  const uint32_t* __restrict__ llen, uint64_t nl,
                                                  const uint32_t* __restrict__ err, uint64_t* __restrict__ has,
                                                  uint64_t* __restrict__ klen, uint32_t* __restrict__ vdl,
                                                  unsigned long long* __restrict__ bad) {
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= nl || *err) return;  // (a piece of 4 GiB or more has no record: the call is refused)
  const LineRec r = rec[l];
  const uint32_t n = llen[l];
  const LogLine v = log_line_at(data + r.start, n, r.klen == kNoSep ? (uint64_t)n : (uint64_t)r.klen);
  const bool tab = v.kind != kLogSkipped;
  has[l] = tab ? 1 : 0;
  klen[l] = tab ? r.klen : 0;
  vdl[l] = v.kind == kLogEntry ? (uint32_t)v.vdl : kBadValue;
  if (v.kind < 0) atomicMin(bad, (unsigned long long)log_bad_pack(l, v.kind == kLogBadValue));
}

__global__ __launch_bounds__(kNT) void k_log_gather(const uint8_t* __restrict__ data, const LineRec* __restrict__ rec,
                                                    const uint32_t* __restrict__ llen,
                                                    const uint32_t* __restrict__ vdl, uint64_t nl,
                                                    const uint64_t* __restrict__ has_scan,
                                                    const uint64_t* __restrict__ len_scan, uint8_t* __restrict__ kb,
                                                    uint64_t* __restrict__ ko, CompactSide* __restrict__ side,
                                                    uint64_t* __restrict__ dmask) {
  // (whole blocks: the first kSampleBlocks of them)
  sample_pfx_masks(nl, [&](uint64_t q) -> uint64_t {
    const LineRec r = rec[q];
    return r.klen == kNoSep ? 0 : ld8_be(data + r.start, r.klen < 8 ? r.klen : 8);
  }, dmask);
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= nl) return;
  const uint64_t E = has_scan[nl], K = len_scan[nl];
  if (l == 0) ko[E] = K;
  const LineRec r = rec[l];
  if (r.klen == kNoSep) return;
  const uint64_t i = E - 1 - has_scan[l];       // the last entry is key 0
  const uint64_t o = K - len_scan[l] - r.klen;  // and its key the batch's first bytes
  ko[i] = o;
  CompactSide sd;
  sd.src = data + r.start;
  sd.llen = llen[l];
  sd.klen = r.klen;
  sd.vdl = vdl[l];
  sd.pad = 0;
  side[i] = sd;
  uint8_t* dst = kb + o;
  for (uint32_t j = 0; j < r.klen; ++j) dst[j] = sd.src[j];
}

}  // namespace

hipError_t launch_log_mark(const uint8_t* data, const LineRec* rec, const uint32_t* llen, uint64_t nl,
                           const uint32_t* err, uint64_t* has, uint64_t* klen, uint32_t* vdl, uint64_t* bad,
                           hipStream_t s) {
  if (!nl) return hipSuccess;
  ProfScope ps("k_log_mark", s);
  hipLaunchKernelGGL(k_log_mark, dim3(blocks_for(nl, kNT)), dim3(kNT), 0, s, data, rec, llen, nl, err, has, klen, vdl,
                     reinterpret_cast<unsigned long long*>(bad));
  return hipGetLastError();
}

hipError_t launch_log_gather(const uint8_t* data, const LineRec* rec, const uint32_t* llen, const uint32_t* vdl,
                             uint64_t nl, const uint64_t* has_scan, const uint64_t* len_scan, uint8_t* kb,
                             uint64_t* ko, CompactSide* side, uint64_t* dmask, hipStream_t s) {
  if (!nl) return hipSuccess;
  ProfScope ps("k_log_gather", s);
  hipLaunchKernelGGL(k_log_gather, dim3(blocks_for(nl, kNT)), dim3(kNT), 0, s, data, rec, llen, vdl, nl, has_scan,
                     len_scan, kb, ko, side, dmask);
  return hipGetLastError();
}

}  // namespace cb
