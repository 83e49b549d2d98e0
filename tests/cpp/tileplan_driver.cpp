// tileplan_driver.cpp — prints the tile planner's answers
// (lsmt_amd/csrc/tileplan.cpp) without a device. Built by
// tests/test_tileplan_cpu.py together with tileplan.cpp under the address and
// undefined-behaviour sanitizers and run as a child process.
//
// stdin: lines "kind m n nb", kind b (plan_build) or p (plan_probe, nb unused).
// stdout, one line per input line:
//   kind tb T kpt C nblk sub plan_ok seg ent lkey lds_part lds_tile long_runs
// seg / ent / lkey: the pass's workspace bytes (lkey 0 for a build); lds_part
// / lds_tile: the dynamic LDS of its partition and tile kernels.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "tileplan.hpp"

int main() {
  char kind;
  uint64_t m, n;
  uint32_t nb;
  while (scanf(" %c %" SCNu64 " %" SCNu64 " %" SCNu32, &kind, &m, &n, &nb) == 4) {
    if (kind != 'b' && kind != 'p') return 2;
    const bool build = kind == 'b';
    const cb::TilePlan p = build ? cb::plan_build(m, n, nb) : cb::plan_probe(m, n);
    const size_t seg = build ? cb::build_seg_bytes(p) : cb::probe_seg_bytes(p);
    const size_t ent = build ? cb::build_ent_bytes(p) : cb::probe_ent_bytes(p);
    const size_t lkey = build ? 0 : cb::probe_lkey_bytes(p);
    const size_t lds_part = build ? cb::build_part_lds(p) : cb::probe_part_lds(p);
    const size_t lds_tile = build ? cb::build_tile_lds(p) : cb::probe_tile_lds(p);
    printf("%c %u %u %u %u %u %u %d %zu %zu %zu %zu %zu %d\n", kind, p.tb, p.T, p.kpt, p.C, p.nblk, p.sub,
           (int)cb::plan_ok(p), seg, ent, lkey, lds_part, lds_tile, (int)cb::long_runs(p.C, p.T));
  }
  return feof(stdin) ? 0 : 2;
}
