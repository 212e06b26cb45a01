#!/bin/bash
# GPU box, from the repository root: the Doppler launch of the headline workload under rocprofv3, product library beside
# variant builds in tools/ab/ (tools/build_variant.sh; `parent` = the parent commit's sources built the same way):
#   bash tools/prof_doppler_ab.sh parent [more variants...]
# Per leg: kernel statistics, then FETCH_SIZE, WRITE_SIZE, the L2's write requests to the fabric (all / 64-byte) and its
# hits and misses, each counter pass in a run of its own with no trace domain beside it; then the byte and request counters
# on known byte counts in the kernels' access widths (tools/membench/pmccal, built beforehand).  Output under
# $PROF_OUT/prof/amb (product) and $PROF_OUT/prof/amb_<variant>, calibration under $PROF_OUT/cal: the layout that
# tools/summarize_prof.py reads when PROF_OUT is the output directory it looks in.
# Every step has its own time limit and the script stops at the first one that fails.
set -o pipefail
REPO=$(pwd); OUT=$(realpath -m "${PROF_OUT:?set PROF_OUT to the output directory}"); mkdir -p $OUT/prof
cd /tmp && export TMPDIR=/tmp
B="python $REPO/bench.py --full --steps 12 --warmup 3 --no-cpu-baseline --no-parity --no-configs --long-s 0 --no-replay"
prune() { # keep what tools/summarize_prof.py reads: the stats table and the counter rows of our kernels
  find "$1" -name "*kernel_trace.csv" -delete 2>/dev/null
  for f in $(find "$1" -name "*_counter_collection.csv" 2>/dev/null); do
    { head -1 "$f"; grep -E 'blah2|cal_' "$f" | grep -v '^"Correlation_Id"'; } > "$f.tmp" && mv "$f.tmp" "$f"
  done
}
for v in "" "$@"; do
  tag=amb${v:+_$v}
  if [ -z "$v" ]; then unset BLAH2HIP_LIBRARY; else export BLAH2HIP_LIBRARY=$REPO/tools/ab/libblah2hip_$v.so; fi
  mkdir -p $OUT/prof/$tag
  # (a variant's file never matches bench.py's lookup of roofline.traffic: its chain is not "amb")
  echo "{\"config\": \"cfg2\", \"batch\": 256, \"fmt\": \"c32\", \"chain\": \"amb${v:+-$v}\"}" > $OUT/prof/$tag/bench_config.json
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof/$tag/trace -o bench --output-format csv -- $B > $OUT/prof/$tag/trace.log 2>&1 ||
    { echo "kernel statistics failed ($tag)"; tail -5 $OUT/prof/$tag/trace.log; exit 1; }
  for pass in "FETCH_SIZE" "WRITE_SIZE" "TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum" "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum"; do
    ptag=$(echo $pass | tr ' ' '_' | cut -c1-40)
    timeout -k 10 300 rocprofv3 --pmc $pass -d $OUT/prof/$tag/pmc_$ptag -o bench --output-format csv -- $B > $OUT/prof/$tag/pmc_$ptag.log 2>&1 ||
      { echo "counter pass $pass failed ($tag)"; tail -5 $OUT/prof/$tag/pmc_$ptag.log; exit 1; }
  done
  prune $OUT/prof/$tag
done
unset BLAH2HIP_LIBRARY
mkdir -p $OUT/cal
for d in fetch write wrreq; do
  case $d in fetch) pass="FETCH_SIZE";; write) pass="WRITE_SIZE";; *) pass="TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum";; esac
  timeout -k 10 200 rocprofv3 --pmc $pass -d $OUT/cal/$d -o cal --output-format csv -- $REPO/tools/membench/pmccal > $OUT/cal/$d.log 2>&1 ||
    { echo "calibration pass $pass failed"; tail -5 $OUT/cal/$d.log; exit 1; }
done
prune $OUT/cal
