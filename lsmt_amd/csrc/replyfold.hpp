// replyfold.hpp — the coordinator's read merge on the host: replyline.hpp's
// rule over replies in host memory, for cb_replies_fold's device == -1 (a
// point read of three replicas, where a device round trip alone costs more
// than the work) and the stand-alone driver (tests/cpp/replyline_driver.cpp).
// Host only, no HIP dependency. It states no rule of its own: what a piece
// is, what its timestamp is, which row wins and what a val becomes are
// replyline.hpp's and rowts.hpp's.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "replyline.hpp"

namespace cb {

struct HostFold {
  // cb_fold_stats, in its order
  uint64_t replies = 0, lines = 0, entries = 0, others = 0, keys = 0, with_text = 0, dead = 0, host_rows = 0,
           bytes = 0, bad_reply = ~0ull, bad_offset = ~0ull;
  // the winners in key order: places in the caller's bytes
  std::vector<uint64_t> key_at, key_len, ts, val_at, val_len;
  std::vector<uint32_t> reply;
  std::vector<uint8_t> flags;
  std::vector<uint8_t> text;                 // the response
  uint64_t other_at = ~0ull, other_len = 0;  // the least other line, when no entry exists
};

// Bytewise order of two byte strings, a prefix before its extension.
inline int bytes_order(const uint8_t* a, uint64_t al, const uint8_t* b, uint64_t bl) {
  const uint64_t m = al < bl ? al : bl;
  const int c = m ? std::memcmp(a, b, m) : 0;
  return c ? c : (al < bl ? -1 : al > bl ? 1 : 0);
}

// The fold of replies bytes[off[r] .. off[r + 1]), r < nr, into *f. 0, or
// kReplyBadUtf8 with f->bad_reply / bad_offset set (the first byte of the
// first failing piece, in bytes) and every count but replies 0, or -1 with
// *why for a piece of 4 GiB or more and for 2^32 or more entries.
inline int fold_host(const uint8_t* bytes, const uint64_t* off, uint32_t nr, HostFold* f, const char** why) {
  struct Entry {
    uint64_t at, ts;
    uint32_t len, tab1, tab2, reply;
  };
  std::vector<Entry> es;
  *f = HostFold{};
  f->replies = nr;
  for (uint32_t r = 0; r < nr; ++r) {
    const uint8_t* p = bytes + off[r];
    const uint64_t n = off[r + 1] - off[r];
    for (uint64_t i = 0; i < n;) {
      const void* nlp = std::memchr(p + i, '\n', n - i);
      const bool terminated = nlp != nullptr;
      const uint64_t plen = terminated ? (uint64_t)((const uint8_t*)nlp - (p + i)) : n - i;
      if (plen >= 0xFFFFFFFFull) {
        *why = "a piece of a reply is 4 GiB or longer";
        return -1;
      }
      if (plen) {
        const ReplyLine v = reply_line(p + i, plen, terminated);
        if (v.kind < 0) {
          *f = HostFold{};  // (the counts of a refused fold say nothing)
          f->replies = nr;
          f->bad_reply = r;
          f->bad_offset = off[r] + i;
          return kReplyBadUtf8;
        }
        if (v.kind == kReplyEntry) {
          es.push_back(Entry{off[r] + i, v.ts, (uint32_t)v.len, (uint32_t)v.tab1, (uint32_t)v.tab2, r});
        } else if (v.kind == kReplyOther) {
          ++f->others;
          if (f->other_at == ~0ull || bytes_order(p + i, v.len, bytes + f->other_at, f->other_len) < 0) {
            f->other_at = off[r] + i;
            f->other_len = v.len;
          }
        }
        f->lines += v.kind != kReplyIgnored;
      }
      i += plen + 1;
    }
  }
  f->entries = es.size();
  if (es.size() > 0xFFFFFFFFull) {
    *why = "too many entries for one fold";
    return -1;
  }
  if (es.empty()) {
    if (f->other_at == ~0ull) {
      f->text = {'[', ']'};
    } else {
      f->text.assign(bytes + f->other_at, bytes + f->other_at + f->other_len);
    }
    f->bytes = f->text.size();
    return 0;
  }
  // (the others decide nothing once an entry exists: the least is not reported)
  f->other_at = ~0ull;
  f->other_len = 0;
  // a key's entries adjacent, in (reply, line) order; the keys ascending
  std::vector<uint32_t> ord(es.size());
  for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
  std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
    const int c = bytes_order(bytes + es[a].at, es[a].tab1, bytes + es[b].at, es[b].tab1);
    return c ? c < 0 : a < b;
  });
  f->text.push_back('[');
  for (size_t i = 0; i < ord.size();) {
    uint32_t best = ord[i];
    size_t j = i + 1;
    for (; j < ord.size(); ++j) {
      const uint32_t e = ord[j];
      if (bytes_order(bytes + es[best].at, es[best].tab1, bytes + es[e].at, es[e].tab1)) break;
      if (lww_replaces(es[best].ts, best, es[e].ts, e)) best = e;
    }
    i = j;
    const Entry& w = es[best];
    const uint8_t* val = bytes + w.at + w.tab2 + 1;
    const uint64_t vl = (uint64_t)w.len - w.tab2 - 1;
    const uint8_t fl = reply_val_flags(val, vl);
    f->key_at.push_back(w.at);
    f->key_len.push_back(w.tab1);
    f->ts.push_back(w.ts);
    f->val_at.push_back(w.at + w.tab2 + 1);
    f->val_len.push_back(vl);
    f->reply.push_back(w.reply);
    f->flags.push_back(fl);
    f->with_text += fl == kFoldText;
    f->dead += fl == kFoldDead;
    f->host_rows += fl == kFoldHost;
    if (fl == kFoldText) {
      if (f->text.size() > 1) f->text.push_back(',');
      f->text.insert(f->text.end(), val, val + vl);
    }
  }
  f->text.push_back(']');
  f->keys = f->key_at.size();
  f->bytes = f->text.size();
  return 0;
}

}  // namespace cb
