#!/bin/bash
# A/B driver for the GPU box. Every rep runs each variant once, in turn, so
# clock and thermal drift fall on all variants alike; the first failure ends
# the call. Usage:
#   LEG=<leg> [REPS=2] [STEPS=20] [WARMUP=3] [TESTS="tests/x.py ..."] [ARGS="..."] \
#     bash tools/gpu/ab.sh VARIANT [VARIANT ...]
# LEG: c5 | wide (bench.py --leg), c3 | c4 (bench.py --workload, the whole
#   default line for c3), c2_lane (build/tools/c2_lane: one-lane C2
#   device time of the given library, tools/c2_lane.hip), or scan
#   (tools/ubench_scan.py, --reps STEPS --warmup WARMUP: single scans against
#   their yardstick compaction). For scan a variant's lib is the root of
#   another checkout built in place (e.g. `git archive <commit> | tar -x -C
#   build/x<name>/tree`, then make -C build/x<name>/tree/lsmt_amd/csrc), whose
#   own tools/ubench_scan.py runs over its own package: another commit's
#   library lacks the symbols this commit's loader prototypes.
# VARIANT = label[,lib][,ENV=value ...]. lib is the directory of another
#   build of the library (an experiment build, or another commit's), made with
#     make -C lsmt_amd/csrc EXTRA="-DCB_EXPERIMENTS ..." BUILD=../../build/x<name>/obj \
#          OUT=../../build/x<name>/libcassbloom.so
#   and run through tools/expbench.py; without one, the product library runs
#   through bench.py. The knobs are of two kinds (lsmt_amd/csrc/knobs.hpp
#   indexes them): device-side variants are -D constants in EXTRA, so each
#   value is its own lib; host-side overrides are the ENV settings, which
#   apply to that variant only and are read by experiment builds alone.
# TESTS run first (pytest -m gpu). Output: gpurun_out/ab/<label>_<rep>.json
# and .err, each summarised by tools/bench_brief.py as it lands.
# Examples (HISTORY.md lists the round-5 ones):
#   LEG=wide bash tools/gpu/ab.sh h6,build/xw,CB_SCREEN_HBITS=6 h8,build/xw,CB_SCREEN_HBITS=8
#   LEG=c2_lane bash tools/gpu/ab.sh dflt,lsmt_amd sub18,build/xc2,CB_BUILD_SUB=1
set -o pipefail
O=gpurun_out/ab
mkdir -p $O
: "${LEG:?LEG is required}" "${REPS:=2}" "${STEPS:=20}" "${WARMUP:=3}"
if [ -n "$TESTS" ]; then
  timeout -k 10 600 python -u -m pytest $TESTS -m gpu -x -q --timeout 300 --timeout-method thread > $O/pytest.log 2>&1 || { tail -30 $O/pytest.log; exit 1; }
  tail -1 $O/pytest.log
fi
for rep in $(seq 1 $REPS); do
  for v in "$@"; do
    IFS=, read -r label lib envs <<< "$v"
    envs=${envs//,/ }
    out=$O/${label}_$rep
    case $LEG in
      c2_lane) cmd=(./build/tools/c2_lane "${lib:-lsmt_amd}/libcassbloom.so") ;;
      scan) cmd=(python "${lib:-.}/tools/ubench_scan.py" --reps $STEPS --warmup $WARMUP $ARGS) ;;
      c3) cmd=(bench.py --full --no-cpu --steps $STEPS --warmup $WARMUP $ARGS) ;;
      c4) cmd=(bench.py --workload c4 --no-cpu --steps $STEPS --warmup $WARMUP $ARGS) ;;
      *) cmd=(bench.py --leg $LEG --no-cpu --steps $STEPS --warmup $WARMUP $ARGS) ;;
    esac
    if [ $LEG != c2_lane ] && [ $LEG != scan ]; then
      if [ -n "$lib" ]; then cmd=(python tools/expbench.py "${cmd[@]:1}"); envs="EXPBENCH_LIB=$lib/libcassbloom.so $envs"
      else cmd=(python "${cmd[@]}"); fi
    fi
    env $envs timeout -k 10 300 "${cmd[@]}" > $out.json 2> $out.err || { echo "[$label rep $rep] failed"; tail -20 $out.err; exit 1; }
    echo "== $label rep $rep"
    if [ $LEG = c2_lane ] || [ $LEG = scan ]; then cat $out.json; else python tools/bench_brief.py $out.json; fi
  done
done
