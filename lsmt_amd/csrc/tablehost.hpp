// tablehost.hpp — host-only arithmetic behind the SSTable entries (no device
// code and no HIP include: tested on the CPU under sanitizers,
// tests/cpp/tablehost_driver.cpp): the carver of 16-byte-aligned parts, the
// wide walk's group classification, a scan result's layout, and the flush's
// file bound and staged block.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cb {

// One block carved into 16-byte-aligned parts: take() gives the offset of the
// next part, total() the bytes measured so far.
struct Carver {
  size_t at = 0;
  size_t take(uint64_t bytes) {
    const size_t o = at;
    at += (size_t)((bytes + 15) & ~15ull);
    return o;
  }
  size_t total() const { return at; }
};

// How a group of up to 64 tables (newest first, t0 .. t0 + gn - 1) maps to
// the set's slots, so the kernel can take the group's candidate bits from a
// window of the rows instead of one bit per table:
//   kind 0: slot(t0 + i) = lo + i          (ascending)
//   kind 1: slot(t0 + i) = lo + gn - 1 - i (descending: the LSM's age order,
//           slot = position in Vec<SsTable>, walked with .rev())
//   kind 2: any other mapping, one bit read per table (slots[t0 + i]).
struct WideGroup {
  uint32_t kind, lo, gn, pad;
};

// The groups of nt tables whose slots are slots[0..nt) (nullptr: table t is
// slot t) into groups[0..wide_group_count(nt)). A group of one table is
// ascending (kind 0, lo = its slot). Returns whether any group is kind 2
// (the walk then reads the slots themselves).
inline uint32_t wide_group_count(uint32_t nt) { return (nt + 63) / 64; }
inline bool wide_groups(const uint32_t* slots, uint32_t nt, WideGroup* groups) {
  bool need_slots = false;
  for (uint32_t g = 0; g < wide_group_count(nt); ++g) {
    const uint32_t t0 = 64 * g, gn = nt - t0 < 64 ? nt - t0 : 64;
    auto slot = [&](uint32_t i) { return slots ? slots[t0 + i] : t0 + i; };
    bool asc = true, desc = true;
    for (uint32_t i = 1; i < gn; ++i) {
      asc = asc && slot(i) == slot(0) + i;
      desc = desc && slot(i) + i == slot(0);
    }
    const uint32_t kind = asc ? 0 : desc ? 1 : 2;
    groups[g] = WideGroup{kind, kind == 0 ? slot(0) : kind == 1 ? slot(gn - 1) : 0, gn, 0};
    need_slots = need_slots || kind == 2;
  }
  return need_slots;
}

// A scan result's block: key_off | val_off | which | keys | vals, for count
// entries and room for kb key bytes and vb value bytes. o receives the parts'
// offsets; returns the block's bytes.
inline size_t scan_layout(uint64_t count, uint64_t kb, uint64_t vb, size_t (&o)[5]) {
  Carver c;
  const uint64_t part[5] = {(count + 1) * 8, (count + 1) * 8, count * 4, kb + 16, vb + 16};
  for (int i = 0; i < 5; ++i) o[i] = c.take(part[i]);
  return c.total();
}

// A bound on the file SsTable::create writes for n entries of K key bytes and
// V value bytes: sum(k + 2 + 4 ceil(v / 3)) <= K + 2n + (4V + 8n) / 3, plus
// the file's 16 bytes of slack and one more.
inline uint64_t flush_file_bound(uint64_t n, uint64_t kbytes, uint64_t vbytes) {
  return kbytes + 2 * n + (4 * vbytes + 8 * n) / 3 + 1 + 16;
}

// The block a flush stages its host inputs into: key offsets | value offsets
// | key bytes | value bytes, a part only for an input that is host memory
// (host[i]; bytes[i] its size). off[i] is meaningful where host[i].
struct FlushStage {
  size_t off[4];
  size_t total;
};
inline FlushStage flush_stage_layout(const bool (&host)[4], const uint64_t (&bytes)[4]) {
  Carver c;
  FlushStage st{};
  for (int i = 0; i < 4; ++i)
    if (host[i]) st.off[i] = c.take(bytes[i]);
  st.total = c.total();
  return st;
}

}  // namespace cb
