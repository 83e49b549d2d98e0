// fold.hpp — the coordinator's read merge on the device (fold.hip; the C
// ABI's cb_replies_fold): the replicas' `key \t ts \t val` replies folded by
// timestamp into the JSON array the client gets (src/cluster.rs:394-473,
// is_write false). The rule is replyline.hpp's.
//
// The replies are staged into one buffer, each followed by one '\n' of the
// library's own (reply r begins at soff[r] = off[r] - off[0] + r, its
// separator stands at soff[r + 1] - 1), so the line index's count -> scan ->
// emit -> finish chain yields exactly the pieces of every reply by itself: no
// piece crosses a reply, and a piece that ends at its reply's separator is
// that reply's unterminated last line, which keeps its '\r'. k_reply_mark
// gives every piece its verdict, two scans place the entries, k_reply_gather
// makes them the merge's records with their parsed timestamps in Merge::ts,
// the merge runs as it stands (the stable key sort and the LWW select), and
// k_fold_size / a scan / k_fold_write turn the winners into the response the
// way the select's size / scan / write pair does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compact.hpp"
#include "sstable.hpp"

namespace cb {

// k_reply_mark's verdict of one piece (replyline.hpp ReplyLine, packed): kind
// is kReply*, len the line's length after the strip, tab2 the second TAB's
// place (an entry's), reply the reply it lies in.
struct ReplyPiece {
  uint64_t ts;
  uint32_t len, tab2, reply;
  int32_t kind;
};

// k_reply_mark's counters (the caller zeroes them, bad to all-ones).
struct FoldCounts {
  uint64_t bad;     // min of the failing pieces' indices
  uint64_t lines;   // pieces that are not empty after the strip
  uint64_t others;  // of those with fewer than two TABs
  uint64_t with_text, dead, host;  // k_fold_size's: the winners by flag
};

// A winner as cb_fold_rows hands it out: places in the caller's bytes.
struct FoldRows {
  uint64_t *key_at, *key_len, *ts, *val_at, *val_len;
  uint32_t* reply;
  uint8_t* flags;
};

// Per piece l of nl (rec / llen as launch_line_finish left them; *err its
// 4-GiB flag: nothing is read when it is up) in the staged buffer of nr
// replies (soff: nr + 1 offsets, device): pc[l], has[l] = it is an entry,
// klen[l] = its key's bytes (0 otherwise), and the counters.
hipError_t launch_reply_mark(const uint8_t* data, const LineRec* rec, const uint32_t* llen, uint64_t nl,
                             const uint32_t* err, const uint64_t* soff, uint32_t nr, ReplyPiece* pc, uint64_t* has,
                             uint64_t* klen, FoldCounts* cnt, hipStream_t s);
// From the exclusive scans of has / klen (nl + 1 entries each; E entries with
// K key bytes): the entries' keys as a ragged batch (kb, ko) in (reply, line)
// order, side[e] (src the line, llen its stripped length, klen the first TAB,
// pad the second, vdl a length that decodes and is no tombstone's), ts[e] the
// parsed timestamp, and dmask as launch_log_gather leaves it.
hipError_t launch_reply_gather(const uint8_t* data, const LineRec* rec, const ReplyPiece* pc, uint64_t nl,
                               const uint64_t* has_scan, const uint64_t* len_scan, uint8_t* kb, uint64_t* ko,
                               CompactSide* side, uint64_t* ts, uint64_t* dmask, hipStream_t s);
// Per sorted record p of n (slen as the LWW select left it: non-zero marks a
// key's winner): flags[p] = replyline.hpp's verdict of the winner's val (0 for
// a loser), inc[p] = a kFoldText val's length + 1 (else 0), win[p] = 1 for a
// winner, and cnt's three winner counters.
hipError_t launch_fold_size(const SortKey* order, const CompactSide* side, const uint64_t* slen, uint64_t n,
                            uint8_t* flags, uint64_t* inc, uint64_t* win, FoldCounts* cnt, hipStream_t s);
// off / wrow: the exclusive scans of inc / win (n + 1 entries each). The
// response into text: [ v0 , v1 ... ] (off[n] + 1 bytes, or the two of [] when
// off[n] is 0), one block per kCompactTile records copying its tile's bytes
// together (copy_tile_bytes), and winner wrow[p]'s row into rows, its places
// moved from the staged buffer into the caller's bytes (reply r's bytes begin
// at coff[r] there; device, nr + 1 offsets).
hipError_t launch_fold_write(const SortKey* order, const CompactSide* side, const uint64_t* ts, const uint8_t* flags,
                             const uint64_t* inc, const uint64_t* off, const uint64_t* win, const uint64_t* wrow,
                             uint64_t n, const uint8_t* data, const uint64_t* soff, const uint64_t* coff, uint32_t nr,
                             FoldRows rows, uint8_t* text, hipStream_t s);

}  // namespace cb
