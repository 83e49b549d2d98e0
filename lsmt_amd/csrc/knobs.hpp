// knobs.hpp — every tuning knob of the library, and the only file here that
// names CB_EXPERIMENTS or reads the environment.
//
// The shipped library has no knobs: knob_int() returns its default without
// reading anything, and a compile-time override without -DCB_EXPERIMENTS is
// an error. An experiment build (make EXTRA="-DCB_EXPERIMENTS ..." into its
// own BUILD= and OUT=, A/B'd against another build by tools/gpu/ab.sh) has two
// kinds:
//   runtime       host-side planning and dispatch overrides between paths
//                 the product compiles anyway, read once from the environment
//                 through knob_int();
//   compile-time  device-side variants: a -D constant per build, so no
//                 product kernel carries an argument or a branch for them.
//
// Runtime (environment of an experiment build):
//   CB_POOL_SLAB=0      capi_runtime.cpp: small pool requests get their own blocks
//   CB_POOL_CONTIG=1    capi_runtime.cpp: pool memory physically contiguous
//   CB_BUILD_BATCH=n    capi_filter.cpp: filters per batched build launch pair
//   CB_NO_BUCKETS=1     capi_get.cpp: reads without the key buckets
//   CB_NO_SCREEN=1      capi_get.cpp: wide reads without the screen
//   CB_SCREEN_HBITS=h   capi_get.cpp: the wide screen's hash bits (0..8)
//   CB_WIDE_MAPS=0      capi_get.cpp: wide reads find the maps through the views
//   CB_DECODE_RAW=0     capi_get.cpp: always the k_tile_scan launch before the decode (gets and scans)
//   CB_BIN_T=t          capi_flush.cpp: bin-sort group target (0: no bin sort)
//   CB_ORDER_FENCE=1    comm.cpp: the order event with its system-scope fence
//   CB_BUILD_TB=b       tileplan.cpp plan_build: tile bits
//   CB_BUILD_KPT=k      tileplan.cpp plan_build: partition keys per thread (1, 2, 4)
//   CB_BUILD_SUB=0|1    tileplan.cpp plan_build: never / always 16-bit sub-tile entries
//   CB_PROBE_TB=b       tileplan.cpp plan_probe: tile bits
//   CB_PROBE_KPT=k      tileplan.cpp plan_probe: partition keys per thread (4, 8)
//
// Compile-time (-D of an experiment build; the defaults below are the product):
//   CB_BUILD_STORES       tilebuild.hip: build store policy bits (1 write-through
//                         partition entries, 2 non-temporal tile write-back)
//   CB_DENSE_KPT          densefs.hip: partition keys per thread and batch
//   CB_DENSE_NB           densefs.hip: key batches per partition block
//   CB_DENSE_PART_W       densefs.hip: k_dense_part's minimum waves per SIMD
//   CB_DENSE_PART_LB8     densefs.hip: shorthand for CB_DENSE_PART_W=8
//   CB_DENSE_ST           densefs.hip: entry stores 0 plain, 1 write-through, 2 non-temporal
//   CB_DENSE_HST          densefs.hip: 0 the zeroed hit words stored plain
//   CB_DENSE_X            densefs.hip: k_dense_probe timing-only variant (wrong
//                         hits): bit 0 skips the set[b] gathers, bit 1 the hit atomics
//   CB_WIDE_SCREEN_BATCH  getmany.hip: summary words loaded together in the wide walk
//   CB_WIDE_THREADS       getmany.hip: k_wide_get_many's workgroup size
#pragma once
#include <cstdlib>

#if !defined(CB_EXPERIMENTS) &&                                                                   \
    (defined(CB_BUILD_STORES) || defined(CB_DENSE_KPT) || defined(CB_DENSE_NB) ||                 \
     defined(CB_DENSE_PART_W) || defined(CB_DENSE_PART_LB8) || defined(CB_DENSE_ST) ||            \
     defined(CB_DENSE_HST) || defined(CB_DENSE_X) || defined(CB_WIDE_SCREEN_BATCH) ||             \
     defined(CB_WIDE_THREADS))
#error "compile-time knob overrides (-DCB_...) need -DCB_EXPERIMENTS: the shipped library takes the defaults"
#endif

#ifndef CB_BUILD_STORES
#define CB_BUILD_STORES 3
#endif
#ifndef CB_DENSE_KPT
#define CB_DENSE_KPT 4
#endif
#ifndef CB_DENSE_NB
#define CB_DENSE_NB 3
#endif
#if defined(CB_DENSE_PART_LB8) && !defined(CB_DENSE_PART_W)
#define CB_DENSE_PART_W 8
#endif
#ifndef CB_DENSE_PART_W
#define CB_DENSE_PART_W 1
#endif
#ifndef CB_DENSE_ST
#define CB_DENSE_ST 2
#endif
#ifndef CB_DENSE_HST
#define CB_DENSE_HST 1
#endif
#ifndef CB_DENSE_X
#define CB_DENSE_X 0
#endif
#ifndef CB_WIDE_SCREEN_BATCH
#define CB_WIDE_SCREEN_BATCH 8
#endif
#ifndef CB_WIDE_THREADS
#define CB_WIDE_THREADS 512
#endif

namespace cb {

// A runtime knob: its value in the environment of an experiment build, dflt
// when unset or empty; always dflt in the shipped library. Read it once per
// site (static const int x = knob_int(...)).
inline int knob_int(const char* name, int dflt) {
#ifdef CB_EXPERIMENTS
  const char* v = getenv(name);
  return v && *v ? atoi(v) : dflt;
#else
  (void)name;
  return dflt;
#endif
}

}  // namespace cb
