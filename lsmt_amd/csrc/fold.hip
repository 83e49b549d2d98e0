// fold.hip — the four kernels of cb_replies_fold (fold.hpp) around the line
// index's count -> scan -> emit -> finish chain, which splits the staged
// replies as it splits a data file, and the merge's stable key sort and LWW
// select, which run over the gathered entries as they run over the lines of
// replica tables.
//
//   k_reply_mark — one lane per piece: its reply by a binary search of the
//       staged offsets (a few entries, L2-resident), whether a '\n' of its own
//       reply ended it (else its reply's separator did), then replyline.hpp's
//       verdict over the piece's bytes (the first TAB is k_line_finish's). A
//       lane reads its own piece only, byte by byte, as k_log_mark does. A
//       wave adds its lines and others to the counters with one atomic each.
//   k_reply_gather — one lane per piece again: an entry's key goes to its
//       scanned slot of the batch in (reply, line) order, so an entry's place
//       in the batch is lww_beats' idx, with its side record and timestamp.
//   k_fold_size — one lane per sorted record, winners only: the canonical walk
//       of the val (one lane per row, as k_select_size walks a payload), its
//       flag and its text's length plus separator.
//   k_fold_write — one block per tile of sorted records: the tile's texts and
//       separators copied by the whole block (copy_tile_bytes: aligned dwords
//       of the response assembled from the replies' bytes), and each winner's
//       row of cb_fold_rows.
#include <hip/hip_runtime.h>

#include "blockscan.hpp"
#include "fold.hpp"
#include "launch.hpp"
#include "profile.hpp"
#include "replyline.hpp"
#include "tablebytes.hpp"

namespace cb {
namespace {

constexpr uint32_t kNT = kCompactTile;

// One atomic per wave for a counter that many lanes bump.
__device__ __forceinline__ void wave_count(bool mine, uint64_t* counter) {
  const uint64_t b = __ballot(mine);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(b));
}

// The reply that staged byte x lies in (soff[0] = 0 <= x < soff[nr]).
__device__ __forceinline__ uint32_t reply_of(const uint64_t* __restrict__ soff, uint32_t nr, uint64_t x) {
  return last_le(nr, x, [&](uint32_t r) { return soff[r]; });
}

__global__ __launch_bounds__(kNT) void k_reply_mark(const uint8_t* __restrict__ data, const LineRec* __restrict__ rec,
                                                    const uint32_t* __restrict__ llen, uint64_t nl,
                                                    const uint32_t* __restrict__ err,
                                                    const uint64_t* __restrict__ soff, uint32_t nr,
                                                    ReplyPiece* __restrict__ pc, uint64_t* __restrict__ has,
                                                    uint64_t* __restrict__ klen, FoldCounts* __restrict__ cnt) {
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  bool line = false, other = false;
  if (l < nl && !*err) {  // (a piece of 4 GiB or more has no record: the call is refused)
    const LineRec r = rec[l];
    const uint32_t n = llen[l];
    const uint32_t rp = reply_of(soff, nr, r.start);
    const bool terminated = r.start + n != soff[rp + 1] - 1;  // (not at its reply's separator)
    const ReplyLine v = reply_line_at(data + r.start, n, terminated, r.klen == kNoSep ? (uint64_t)n : (uint64_t)r.klen);
    const bool entry = v.kind == kReplyEntry;
    pc[l] = ReplyPiece{v.ts, (uint32_t)v.len, (uint32_t)v.tab2, rp, v.kind};
    has[l] = entry ? 1 : 0;
    klen[l] = entry ? v.tab1 : 0;
    line = entry || v.kind == kReplyOther;
    other = v.kind == kReplyOther;
    if (v.kind < 0) atomicMin((unsigned long long*)&cnt->bad, (unsigned long long)l);
  }
  wave_count(line, &cnt->lines);
  wave_count(other, &cnt->others);
}

__global__ __launch_bounds__(kNT) void k_reply_gather(const uint8_t* __restrict__ data, const LineRec* __restrict__ rec,
                                                      const ReplyPiece* __restrict__ pc, uint64_t nl,
                                                      const uint64_t* __restrict__ has_scan,
                                                      const uint64_t* __restrict__ len_scan, uint8_t* __restrict__ kb,
                                                      uint64_t* __restrict__ ko, CompactSide* __restrict__ side,
                                                      uint64_t* __restrict__ ts, uint64_t* __restrict__ dmask) {
  // (whole blocks: the first kSampleBlocks of them)
  sample_pfx_masks(nl, [&](uint64_t q) -> uint64_t {
    if (pc[q].kind != kReplyEntry) return 0;
    const LineRec r = rec[q];
    return ld8_be(data + r.start, r.klen < 8 ? r.klen : 8);
  }, dmask);
  const uint64_t l = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= nl) return;
  if (l == 0) ko[has_scan[nl]] = len_scan[nl];
  const ReplyPiece p = pc[l];
  if (p.kind != kReplyEntry) return;
  const LineRec r = rec[l];
  const uint64_t i = has_scan[l], o = len_scan[l];
  ko[i] = o;
  ts[i] = p.ts;
  CompactSide sd;
  sd.src = data + r.start;
  sd.llen = p.len;
  sd.klen = r.klen;
  sd.vdl = 16;  // decodable and no tombstone: the select takes every entry
  sd.pad = p.tab2;
  side[i] = sd;
  uint8_t* dst = kb + o;
  for (uint32_t j = 0; j < r.klen; ++j) dst[j] = sd.src[j];
}

__global__ __launch_bounds__(kNT) void k_fold_size(const SortKey* __restrict__ order,
                                                   const CompactSide* __restrict__ side,
                                                   const uint64_t* __restrict__ slen, uint64_t n,
                                                   uint8_t* __restrict__ flags, uint64_t* __restrict__ inc,
                                                   uint64_t* __restrict__ win, FoldCounts* __restrict__ cnt) {
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  uint8_t f = 0;
  if (p < n) {
    uint64_t step = 0;
    const bool w = slen[p] != 0;
    if (w) {
      const CompactSide sd = side[order[p].idx];
      const uint64_t vl = (uint64_t)sd.llen - sd.pad - 1;
      f = reply_val_flags(sd.src + sd.pad + 1, vl);
      if (f == kFoldText) step = vl + 1;
    }
    flags[p] = f;
    inc[p] = step;
    win[p] = w ? 1 : 0;
  }
  wave_count(f == kFoldText, &cnt->with_text);
  wave_count(f == kFoldDead, &cnt->dead);
  wave_count(f == kFoldHost, &cnt->host);
}

__global__ __launch_bounds__(kNT) void k_fold_write(const SortKey* __restrict__ order,
                                                    const CompactSide* __restrict__ side,
                                                    const uint64_t* __restrict__ ts, const uint8_t* __restrict__ flags,
                                                    const uint64_t* __restrict__ inc, const uint64_t* __restrict__ off,
                                                    const uint64_t* __restrict__ win,
                                                    const uint64_t* __restrict__ wrow, uint64_t n,
                                                    const uint8_t* __restrict__ data,
                                                    const uint64_t* __restrict__ soff,
                                                    const uint64_t* __restrict__ coff, uint32_t nr, FoldRows rows,
                                                    uint8_t* __restrict__ text) {
  __shared__ uint64_t s_off[kNT + 1];    // text i's first byte in the tile
  __shared__ const uint8_t* s_src[kNT];  // its val
  __shared__ uint32_t s_vl[kNT];         // that many bytes, then the separator
  const uint64_t p = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  const uint64_t total = off[n];
  if (p == 0) {
    text[0] = '[';
    if (!total) text[1] = ']';
  }
  const uint64_t step = p < n ? inc[p] : 0;
  CompactSide sd{};
  if (p < n && win[p]) {
    const uint32_t idx = order[p].idx;
    sd = side[idx];
    // the winner's row, its places in the caller's bytes
    const uint64_t at = (uint64_t)(sd.src - data), row = wrow[p];
    const uint32_t rp = reply_of(soff, nr, at);
    const uint64_t line = at - soff[rp] + coff[rp];
    if (rows.key_at) rows.key_at[row] = line;
    if (rows.key_len) rows.key_len[row] = sd.klen;
    if (rows.ts) rows.ts[row] = ts[idx];
    if (rows.val_at) rows.val_at[row] = line + sd.pad + 1;
    if (rows.val_len) rows.val_len[row] = (uint64_t)sd.llen - sd.pad - 1;
    if (rows.reply) rows.reply[row] = rp;
    if (rows.flags) rows.flags[row] = flags[p];
  }
  uint64_t tc;
  const uint64_t ci = block_scan<(int)kNT>(step ? 1 : 0, &tc);
  if (!tc) return;  // (uniform)
  const uint64_t tile0 = (uint64_t)blockIdx.x * kNT, tend = tile0 + kNT < n ? tile0 + kNT : n;
  const uint64_t base = off[tile0], tl = off[tend] - base;
  if (step) {
    s_off[ci] = off[p] - base;
    s_src[ci] = sd.src + sd.pad + 1;
    s_vl[ci] = (uint32_t)(step - 1);
  }
  if (threadIdx.x == 0) s_off[tc] = tl;
  __syncthreads();
  const uint32_t sep = base + tl == total ? ']' : ',';  // behind the tile's last text
  copy_tile_bytes(text + 1 + base, tl, (uint32_t)tc, s_off, [&](uint32_t i, uint64_t j) -> uint32_t {
    const uint64_t b = j - s_off[i];
    return b < s_vl[i] ? s_src[i][b] : (j + 1 == tl ? sep : (uint32_t)',');
  });
}

}  // namespace

hipError_t launch_reply_mark(const uint8_t* data, const LineRec* rec, const uint32_t* llen, uint64_t nl,
                             const uint32_t* err, const uint64_t* soff, uint32_t nr, ReplyPiece* pc, uint64_t* has,
                             uint64_t* klen, FoldCounts* cnt, hipStream_t s) {
  if (!nl) return hipSuccess;
  ProfScope ps("k_reply_mark", s);
  hipLaunchKernelGGL(k_reply_mark, dim3(blocks_for(nl, kNT)), dim3(kNT), 0, s, data, rec, llen, nl, err, soff, nr, pc,
                     has, klen, cnt);
  return hipGetLastError();
}

hipError_t launch_reply_gather(const uint8_t* data, const LineRec* rec, const ReplyPiece* pc, uint64_t nl,
                               const uint64_t* has_scan, const uint64_t* len_scan, uint8_t* kb, uint64_t* ko,
                               CompactSide* side, uint64_t* ts, uint64_t* dmask, hipStream_t s) {
  if (!nl) return hipSuccess;
  ProfScope ps("k_reply_gather", s);
  hipLaunchKernelGGL(k_reply_gather, dim3(blocks_for(nl, kNT)), dim3(kNT), 0, s, data, rec, pc, nl, has_scan, len_scan,
                     kb, ko, side, ts, dmask);
  return hipGetLastError();
}

hipError_t launch_fold_size(const SortKey* order, const CompactSide* side, const uint64_t* slen, uint64_t n,
                            uint8_t* flags, uint64_t* inc, uint64_t* win, FoldCounts* cnt, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_fold_size", s);
  hipLaunchKernelGGL(k_fold_size, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, slen, n, flags, inc, win,
                     cnt);
  return hipGetLastError();
}

hipError_t launch_fold_write(const SortKey* order, const CompactSide* side, const uint64_t* ts, const uint8_t* flags,
                             const uint64_t* inc, const uint64_t* off, const uint64_t* win, const uint64_t* wrow,
                             uint64_t n, const uint8_t* data, const uint64_t* soff, const uint64_t* coff, uint32_t nr,
                             FoldRows rows, uint8_t* text, hipStream_t s) {
  if (!n) return hipSuccess;
  ProfScope ps("k_fold_write", s);
  hipLaunchKernelGGL(k_fold_write, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, order, side, ts, flags, inc, off, win,
                     wrow, n, data, soff, coff, nr, rows, text);
  return hipGetLastError();
}

}  // namespace cb
