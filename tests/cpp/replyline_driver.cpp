// replyline_driver.cpp — prints what lsmt_amd/csrc/replyline.hpp decides of a
// piece of a reply and what lsmt_amd/csrc/replyfold.hpp folds replies into
// (the rule behind cb_replies_fold and cb_reply_line) without a device. Built
// by tests/test_fold_cpu.py under the address and undefined-behaviour
// sanitizers and run as a child process.
//
// stdin, one request per line (bytes travel as hex, "-" for none):
//   L TERMINATED HEX  -> "kind key_len ts val_at val_len val_flags" of the piece
//   F HEX...          -> the fold of the replies, in order:
//                        "rc | the 11 stats | text | other_at other_len | rows"
//                        with a row as key_at:key_len:ts:val_at:val_len:reply:flags
// stdout: one line per request. Every byte string is copied into a heap block
// of exactly its size first, so a read past it is the sanitizer's.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "replyfold.hpp"
#include "replyline.hpp"

namespace {

std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[v.size() ? v.size() : 1]);
  if (!v.empty()) std::memcpy(b.get(), v.data(), v.size());
  return b;
}

int hex(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

bool unhex(const std::string& s, std::vector<uint8_t>* out) {
  out->clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    const int h = hex(s[i]), l = hex(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out->push_back((uint8_t)(h << 4 | l));
  }
  return true;
}

void line(std::istringstream& in) {
  int terminated = 0;
  std::string h;
  std::vector<uint8_t> v;
  if (!(in >> terminated >> h) || !unhex(h, &v)) {
    std::printf("ERR request\n");
    return;
  }
  const auto p = exact(v);
  const cb::ReplyLine r = cb::reply_line(p.get(), (uint64_t)v.size(), terminated != 0);
  const bool entry = r.kind == cb::kReplyEntry;
  const uint64_t va = entry ? r.tab2 + 1 : 0, vl = entry ? r.len - va : 0;
  std::printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", r.kind, entry ? r.tab1 : 0, entry ? r.ts : 0,
              va, vl, entry ? (unsigned)cb::reply_val_flags(p.get() + va, vl) : 0u);
}

void fold(std::istringstream& in) {
  std::vector<uint8_t> all, v;
  std::vector<uint64_t> off{0};
  std::string h;
  while (in >> h) {
    if (!unhex(h, &v)) {
      std::printf("ERR request\n");
      return;
    }
    all.insert(all.end(), v.begin(), v.end());
    off.push_back(all.size());
  }
  const auto p = exact(all);
  cb::HostFold f;
  const char* why = "";
  const int rc = cb::fold_host(p.get(), off.data(), (uint32_t)(off.size() - 1), &f, &why);
  if (rc == -1) {
    std::printf("ERR %s\n", why);
    return;
  }
  std::printf("%d | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
              " %" PRIu64 " %" PRIu64 " %" PRIu64 " | ",
              rc, f.replies, f.lines, f.entries, f.others, f.keys, f.with_text, f.dead, f.host_rows, f.bytes,
              f.bad_reply, f.bad_offset);
  if (f.text.empty()) std::printf("-");
  for (uint8_t b : f.text) std::printf("%02x", b);
  std::printf(" | %" PRIu64 " %" PRIu64 " |", f.other_at, f.other_len);
  for (size_t i = 0; i < f.key_at.size(); ++i)
    std::printf(" %" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%u:%u", f.key_at[i], f.key_len[i],
                f.ts[i], f.val_at[i], f.val_len[i], f.reply[i], (unsigned)f.flags[i]);
  std::printf("\n");
}

}  // namespace

int main() {
  std::string req;
  while (std::getline(std::cin, req)) {
    std::istringstream in(req);
    std::string op;
    in >> op;
    if (op == "L") line(in);
    else if (op == "F") fold(in);
    else std::printf("ERR request\n");
  }
  return 0;
}
